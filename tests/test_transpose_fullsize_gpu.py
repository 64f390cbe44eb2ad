"""Transpose Regrid at full size: configuration 4's bilinear handle (3.0 M cells <- 1800 x 1060, 55 levels) in float64 cell-fast and
float32 level-fast, and configuration 5's periodic 3600 x 1800 lat-lon grid's EDGE2 handle with its pole caps, against A^T g from
the handles' own weight lists."""
import numpy as np
import pytest

from _transpose_ref import assert_f32_close, assert_f64_close, transpose_ref

pytestmark = pytest.mark.gpu


def test_c4_bilinear_55_levels(gpu_lib):
    import torch
    from mpassit_amd import regrid as R, workloads
    m, g, nlev, _ = workloads.workload("c4_3m_regional")
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
    rh = R.regrid_store(mesh, grid, R.REGRIDMETHOD_BILINEAR)
    nref, mx = rh.transpose_stats()
    assert 0 < nref <= rh.n_src == m.nCells and 1 <= mx <= 64
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1060)
    src = (torch.rand((nlev, rh.n_dst), dtype=torch.float64, device="cuda", generator=gen) - 0.5) * 80.0
    cf = rh.regrid_transpose(src, nlev=nlev)
    lf32 = rh.regrid_transpose(src, nlev=nlev, layout=R.LAYOUT_LEV_FAST, out_dtype=torch.float32)
    torch.cuda.synchronize()
    # every level: float32 file order is the float64 cell-fast result rounded once
    assert torch.equal(lf32[0].t(), cf[0].to(torch.float32))
    levels = [0, 27, 54]
    want, bound = transpose_ref(rh, src[levels].cpu().numpy())
    assert_f64_close(cf[0, levels].cpu().numpy(), want, bound, "c4 float64 cell-fast")
    assert_f32_close(lf32[0][:, levels].t().cpu().numpy(), want, bound, "c4 float32 level-fast")
    assert rh.transpose_build_ms() > 0.0
    rh.release()
    mesh.destroy()
    grid.destroy()


def test_c5_edge2_pole_caps(gpu_lib):
    import torch
    from mpassit_amd import regrid as R, target_grid as T
    t = T.define_target_grid_params("lat-lon", 3601, 1801, stand_lon=0.0, is_regional=False)
    grid = R.Grid.from_target(t)
    rh = R.regrid_store_grid(grid, R.STAGGERLOC_EDGE2)
    dst, _, wp, row_len = rh.pole()
    assert row_len == 3600 and (wp != 0).sum() > 0
    nlev = 3
    src = torch.randn((2, nlev, rh.n_dst), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    cf = rh.regrid_transpose(src, nlev=nlev, nfields=2)
    lf = rh.regrid_transpose(src, nlev=nlev, nfields=2, layout=R.LAYOUT_LEV_FAST)
    torch.cuda.synchronize()
    assert torch.equal(lf.transpose(1, 2), cf)
    for f in range(2):
        want, bound = transpose_ref(rh, src[f].cpu().numpy())
        assert_f64_close(cf[f].cpu().numpy(), want, bound, "c5 EDGE2 field %d" % f)
    rh.release()
    grid.destroy()
