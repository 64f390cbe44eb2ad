"""Grid -> Mesh at full size: configuration 4 turned round -- the 1800 x 1060 CENTER points of the 3-km Lambert grid onto the 3.0 M-cell
regional mesh.  Store parity on a fixed random sample of 200 000 cells against the numpy restatement of the rule (candidates from the
oracle's inverse projection), and one 55-level float32 field whose [cell][lev] result must be the transposed regrid_typed result byte
for byte -- a cell count that is no multiple of the kernel's 64-cell block, a level count (55) that is no multiple of a line."""
import numpy as np
import pytest

import _to_mesh_ref as TR
from _parity_helpers import assert_fixed_weights_equal

pytestmark = pytest.mark.gpu

SAMPLE = 200_000
TIE_CAP = 1e-4


def test_config4_turned_round(gpu_lib, oracle):
    import torch
    from mpassit_amd import regrid as R, workloads
    o = oracle
    m, g, nlev, _ = workloads.workload("c4_3m_regional")
    assert nlev == 55
    grid, mesh = R.Grid.from_proj(g, fill_target=False), R.Mesh.from_mpas(m)
    rh = R.regrid_store_to_mesh(grid, mesh)
    assert rh.store_path == 1, "the inverse route ran"
    assert (rh.n_src, rh.n_dst, rh.nnz_per_row) == (1800 * 1060, m.nCells, 4) and m.nCells % 64 != 0
    print("store %.3f ms, %d of %d points took the pyramid" % (rh.store_ms, rh.store_stats[1], rh.store_stats[2]))

    # ---- Store parity on a sample -------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(2025)
    pick = np.sort(rng.choice(m.nCells, SAMPLE, replace=False))
    lon_d, lat_d = o.mesh_coords_deg(m.lonCell[pick], m.latCell[pick])
    pts = o.lonlat_deg_to_xyz(lon_d, lat_d)
    p = g.proj
    po = o.Proj.lambert(p.truelat1, p.truelat2, p.stdlon, p.lat1, p.lon1, p.knowni, p.knownj, p.dx)
    ij = np.array([po.latlon_to_ij(float(la), float(lo)) for la, lo in zip(lat_d, lon_d)])
    lon, lat = grid.coords(R.STAGGERLOC_CENTER)
    sxyz = o.lonlat_deg_to_xyz(lon, lat).reshape(g.ny, g.nx, 3)
    ri, rw, edge = TR.to_mesh_bilinear(sxyz, pts, cand=(ij[:, 0] - 1.0, ij[:, 1] - 1.0))      # 1-based (i, j) -> 0-based CENTER index
    share = TR.edge_share(edge)
    print("reference: %d mapped of %d, share within 1e-9 of a quad edge %.3g" % (int((ri[:, 0] >= 0).sum()), SAMPLE, share))
    assert share <= TIE_CAP
    gi, gw = rh.weights()
    ties = assert_fixed_weights_equal(ri, rw, gi[pick], gw[pick])
    print("ties %d" % ties)
    assert ties <= TIE_CAP * SAMPLE
    assert (ri[:, 0] >= 0).mean() > 0.8
    del gi, gw

    # ---- one 55-level float32 field ---------------------------------------------------------------------------------------------
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4)
    src = (torch.rand((nlev, rh.n_src), dtype=torch.float32, device="cuda", generator=gen) - 0.5) * 60.0
    want = rh.regrid_typed(src.reshape(-1), nlev=nlev, out_dtype=torch.float32).reshape(nlev, rh.n_dst)
    lf = rh.regrid_to_mesh(src, nlev=nlev, layout=R.LAYOUT_LEV_FAST)
    assert tuple(lf.shape) == (1, rh.n_dst, nlev)
    assert torch.equal(lf[0].view(torch.int32), want.t().contiguous().view(torch.int32)), "LEV_FAST is not the transposed regrid_typed result"
    cf = rh.regrid_to_mesh(src, nlev=nlev, layout=R.LAYOUT_CELL_FAST)
    assert torch.equal(cf[0].view(torch.int32), want.view(torch.int32))
    rh.release()
    mesh.destroy()
    grid.destroy()
