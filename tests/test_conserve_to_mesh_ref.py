"""The numpy reference of the conservative Grid -> Mesh Store (tests/_conserve_to_mesh_ref.py) checked on the CPU before any GPU is
involved: known areas, B_ref built from the oracle's Mesh -> Grid matrix AND from the 50-digit brute-force entries of
tests/golden/store_hp.json agreeing within the bar the GPU test uses, rows of wholly covered cells summing to 1, and next to no
sliver-sized entries (which could legitimately exist on one side only)."""
import numpy as np
import pytest

import _conserve_to_mesh_ref as CR
from _parity_helpers import assert_csr_equal
from conftest import mesh_xyz
from test_store_goldens import cases


def test_octant_triangle_has_area_half_pi():
    e = np.eye(3)
    assert abs(CR.tri_area(e[0], e[1], e[2]) - np.pi / 2) < 1e-15
    assert abs(CR.tri_area(e[0], e[2], e[1]) + np.pi / 2) < 1e-15          # signed
    assert abs(CR.poly_area(e) - np.pi / 2) < 1e-15
    # a lune cut into a quad: lon 0 .. 90, lat 0 .. 90 with a collapsed pole side is the same octant
    quad = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [0, 0, 1.0]])
    assert abs(CR.poly_area(quad) - np.pi / 2) < 1e-15
    assert abs(CR.grid_cell_areas(np.array([[e[0], e[1]], [e[2], e[2]]]), 1, 1)[0] - np.pi / 2) < 1e-15


def test_global_grid_and_mesh_areas_sum_to_the_sphere(global_mesh, oracle):
    from mpassit_amd import target_grid as tg
    g = tg.define_target_grid_params("lat-lon", nx=73, ny=37, stand_lon=0.0, is_regional=False)
    ga = CR.grid_cell_areas(oracle.lonlat_deg_to_xyz(g.lon_c, g.lat_c), g.nx, g.ny)
    assert abs(ga.sum() - 4 * np.pi) < 1e-11          # (great-circle sides: a cell is not its lat-lon box, the cells still tile the sphere)
    _, vxyz = mesh_xyz(oracle, global_mesh)
    assert abs(CR.mesh_cell_areas(global_mesh.verticesOnCell, vxyz).sum() - 4 * np.pi) < 1e-10


def _inside_interior(vxyz, corner, nx, ny):
    """bool per vertex: it lies in a grid cell that is not on the grid's outermost ring."""
    c = corner.reshape(ny + 1, nx + 1, 3)
    q = np.stack([c[1:-2, 1:-2], c[1:-2, 2:-1], c[2:-1, 2:-1], c[2:-1, 1:-2]], axis=2).reshape(-1, 4, 3)     # cells 1 .. n - 2
    sign = np.sign(CR.tri_area(q[:, 0], q[:, 1], q[:, 2]) + CR.tri_area(q[:, 0], q[:, 2], q[:, 3]))
    nrm = np.cross(q, np.roll(q, -1, axis=1)) * sign[:, None, None]          # [cells][4][3], inward side positive
    ok = np.zeros(vxyz.shape[0], bool)
    for v0 in range(0, vxyz.shape[0], 512):
        d = np.einsum("vk,cek->vce", vxyz[v0:v0 + 512], nrm)
        ok[v0:v0 + 512] = (d >= -1e-15).all(axis=2).any(axis=1)
    return ok


def wholly_inside(voc, vxyz, corner, nx, ny):
    ok = _inside_interior(vxyz, corner, nx, ny)
    voc = np.asarray(voc)
    return (np.where(voc > 0, ok[np.maximum(voc, 1) - 1], True)).all(axis=1) & ((voc > 0).sum(axis=1) >= 3)


@pytest.mark.parametrize("norm", [CR.NORM_DSTAREA, CR.NORM_FRACAREA], ids=["dstarea", "fracarea"])
@pytest.mark.parametrize("case", cases(), ids=lambda c: c.name)
def test_reference_from_oracle_and_from_the_goldens_agree(oracle, case, norm):
    o, m = oracle, case.mesh
    _, vxyz = mesh_xyz(o, m)
    kxyz = o.lonlat_deg_to_xyz(case.lon_c, case.lat_c)
    area_g, area_c = CR.grid_cell_areas(kxyz, case.nx, case.ny), CR.mesh_cell_areas(m.verticesOnCell, vxyz)
    rowptr, col, val = o.conserve(m.verticesOnCell, vxyz, case.nx, case.ny, kxyz)[:3]
    bo = CR.b_ref_from_csr(rowptr, col, val, area_g, area_c, norm)
    gold = np.array(case.expect["conserve"], np.float64)
    bg = CR.b_ref(gold[:, 0].astype(np.int64), gold[:, 1].astype(np.int64), gold[:, 2], area_g, area_c, norm)
    tol = CR.tol_both(kxyz, case.nx, case.ny, m.verticesOnCell, vxyz)
    n_src = case.nx * case.ny
    common, only_o, only_g = assert_csr_equal(bo[0], bo[1], bo[2], bg[0], bg[1], bg[2], n_src, tol=tol)
    dfrac = np.abs(bo[3] - bg[3]).max()
    print("%s: %d common entries, %d / %d on one side only, bar %.1e, frac %.1e apart" % (case.name, common, only_o, only_g, tol, dfrac))
    assert common > 100 and dfrac < tol
    # a grid cell's area from the helper x the golden weight reproduces the overlap: the overlaps of a wholly covered mesh cell add up
    # to the cell's own area from the other helper
    inside = wholly_inside(m.verticesOnCell, vxyz, kxyz, case.nx, case.ny)
    cover = np.bincount(gold[:, 1].astype(np.int64), weights=gold[:, 2] * area_g[gold[:, 0].astype(np.int64)], minlength=m.nCells)
    if inside.any():
        assert np.abs(cover[inside] / area_c[inside] - 1.0).max() < tol
    # in the reference alone: rows of wholly covered cells sum to 1 (DSTAREA; FRACAREA: every covered row does), and next to no slivers
    for b in (bo, bg):
        rows = np.bincount(np.repeat(np.arange(m.nCells), np.diff(b[0])), weights=b[2], minlength=m.nCells)
        sel = inside if norm == CR.NORM_DSTAREA else np.diff(b[0]) > 0
        assert np.abs(rows[sel] - 1.0).max() < tol if sel.any() else True
        assert CR.sliver_share(b[2]) <= CR.SLIVER_CAP, "the reference itself holds sliver-sized entries"
    print("%s: %d of %d cells wholly inside the grid" % (case.name, int(inside.sum()), m.nCells))


def test_some_golden_cells_are_wholly_inside(oracle):
    n = 0
    for case in cases():
        _, vxyz = mesh_xyz(oracle, case.mesh)
        n += int(wholly_inside(case.mesh.verticesOnCell, vxyz, oracle.lonlat_deg_to_xyz(case.lon_c, case.lat_c), case.nx, case.ny).sum())
    assert n >= 20
