"""Pitched destinations at full size: x_c4_1799x1059 (HRRR's 1799 x 1059 mass points under configuration 4's 3.0 M-cell mesh, 55 levels),
float32 big-endian file order in and out -- what the Fortran driver's device flow writes -- through the library's own kernel choice.
The pitched result is the dense one bit for bit, the pad of every plane keeps its NaN, and a few levels agree with the oracle's
orc_apply_fixed (float32 rounding of the float64 reference, tests/_oracle_compare.py)."""
import numpy as np
import pytest

from _oracle_compare import assert_f32_ulp

pytestmark = pytest.mark.gpu


def test_fullsize_file_order_f32be_pitched(gpu_lib, oracle):
    import torch
    from mpassit_amd import regrid as R, workloads
    m, g, nlev, _ = workloads.workload("x_c4_1799x1059")
    assert (g.nx, g.ny, nlev) == (1799, 1059, 55)
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
    rh = R.regrid_store(mesh, grid, R.REGRIDMETHOD_BILINEAR)
    P = g.nx * g.ny
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1799)
    s32 = ((torch.rand((nlev, m.nCells), dtype=torch.float64, device="cuda", generator=gen) - 0.5) * 60.0).to(torch.float32)
    # MPAS file order [cell][level], big-endian bytes as the NetCDF classic variable holds them
    src_be = s32.t().contiguous().view(torch.int32).view(torch.uint8).view(-1, 4).flip(1).contiguous().view(torch.float32).view(-1)
    be = dict(nlev=nlev, layout=R.LAYOUT_LEV_FAST, out_dtype=torch.float32, src_be=True, dst_be=True)
    dense = rh.regrid_typed(src_be, **be)
    ld = rh.level_stride(torch.float32)
    assert ld == 1905152
    raw = torch.full((nlev * ld,), float("nan"), dtype=torch.float32, device="cuda")
    out = raw.as_strided((1, nlev, g.ny, g.nx), (nlev * ld, ld, g.nx, 1))
    rh.regrid_typed(src_be, out=out, **be)
    torch.cuda.synchronize()
    planes = raw.view(nlev, ld).view(torch.int32)
    assert torch.equal(planes[:, :P], dense.view(nlev, P).view(torch.int32)), "pitched planes differ from the dense result"
    nan_bits = int(torch.tensor([float("nan")], dtype=torch.float32).view(torch.int32)[0])
    assert bool((planes[:, P:] == nan_bits).all()), "the pad was written"
    # three levels against the oracle (the result byte-swapped back to native float32)
    idx, w = rh.weights()
    levels = [0, 27, 54]
    want = torch.as_tensor(oracle.apply_fixed(idx, w, s32[levels].to(torch.float64).cpu().numpy(), len(levels)), device="cuda").view(len(levels), P)
    got = raw.view(nlev, ld)[levels, :P].contiguous().view(torch.uint8).view(-1, 4).flip(1).contiguous().view(torch.float32).view(len(levels), P)
    assert_f32_ulp(got, want, "pitched f32-BE file order vs oracle", eps=1e-13 * 30.0)
    rh.release()
    mesh.destroy()
    grid.destroy()
