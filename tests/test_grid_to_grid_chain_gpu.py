"""The handle-to-handle calls on the handles of the Stores between two grids (mpg_regrid_store_grid_to_grid,
mpg_regrid_store_conserve_grid_to_grid): extrapolate, creep, mask_handle, patch, conserve_2nd and compose, one small test each, held to
the BITS of the numpy mirrors in mpassit_amd/target_grid.py fed with the library's own exports (weights(), csr(), Grid.xyz).  Nothing of
these calls is new here: the tests show that a Grid -> Grid handle with its [dny][dnx] destination is served like every other one.

Grids: L (Lambert 40 x 30 cells) and G (lat-lon 60 x 40 cells, partly outside L) of tests/_grid_to_grid_ref.py."""
import numpy as np
import pytest

import _grid_to_grid_ref as GR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(gpu_lib):
    from mpassit_amd import regrid as R
    d = dict(L=R.Grid.from_target(GR.target("L")), G=R.Grid.from_target(GR.target("G")))
    d["bil"] = R.regrid_store_grid_to_grid(d["L"], d["G"])
    d["cons"] = R.regrid_store_conserve_grid_to_grid(d["L"], d["G"])
    yield d
    d["bil"].release()
    d["cons"].release()
    d["L"].destroy()
    d["G"].destroy()


def _csr_of(h):
    from mpassit_amd import target_grid as tg
    return h.csr() if h.nnz_per_row == 0 else tg.fixed_to_csr(*h.weights())


def _same_csr(got, want):
    assert np.array_equal(got[0], want[0]), "rowptr differs"
    assert np.array_equal(got[1], want[1]), "col differs"
    g, w = np.asarray(got[2], np.float64).reshape(-1), np.asarray(want[2], np.float64).reshape(-1)
    assert g.size == w.size and np.array_equal(g.view(np.int64), w.view(np.int64)), "%d of %d values differ" % ((g != w).sum(), g.size)


def _shape_kept(new, old):
    assert (new.n_src, new.n_dst, new.nx_dst, new.ny_dst) == (old.n_src, old.n_dst, old.nx_dst, old.ny_dst) == (1200, 2400, 60, 40)


def test_extrapolate_fills_the_unmapped_points(world):
    from mpassit_amd import regrid as R, target_grid as tg
    rh = world["bil"]
    idx, w = rh.weights()
    un = idx[:, 0] < 0
    assert 0 < un.sum() < rh.n_dst
    filled = R.extrapolate(rh, world["L"], world["G"], R.EXTRAPMETHOD_NEAREST_STOD)
    _shape_kept(filled, rh)
    rowlen, ids, wn = tg.extrapolate_rows(world["L"].xyz(), world["G"].xyz(), un, tg.EXTRAPMETHOD_NEAREST_STOD)
    assert (rowlen == 1).all()
    # STOD fits the slots, so the handle stays fixed: mapped rows are copied; a filled row holds its nearest source with weight 1 in slot 0
    # and the same source with +0.0 in the slots behind it (the layout tests/test_extrapolate_gpu.py holds every fixed result to)
    want_idx, want_w = idx.copy(), w.copy()
    want_idx[un] = ids[:, :1]
    want_w[un] = 0.0
    want_w[un, 0] = wn[:, 0]
    got_idx, got_w = filled.weights()
    assert filled.nnz_per_row == 4 and np.array_equal(got_idx, want_idx)
    assert np.array_equal(np.ascontiguousarray(got_w).view(np.int64), np.ascontiguousarray(want_w).view(np.int64)), "weights differ in their bits"
    assert (wn[:, 0] == 1.0).all() and (got_idx[:, 0] >= 0).all(), "every point is mapped now"
    assert filled.store_stats[1] == int(un.sum())
    filled.release()


def test_creep_two_levels(world):
    from mpassit_amd import regrid as R, target_grid as tg
    rh = world["bil"]
    crept = R.creep(rh, world["G"], num_levels=2)
    _shape_kept(crept, rh)
    level, rowptr, col, val = tg.creep_rows(*_csr_of(rh), tg.creep_neighbours_grid(60, 40), 2)
    assert (level == 1).any() and (level == 2).any() and (level < 0).any()
    _same_csr(crept.csr(), (rowptr, col, val))
    assert crept.store_stats[1] == int((level > 0).sum()) and crept.store_stats[3] == int((level < 0).sum())
    crept.release()


def test_mask_handle(world):
    from mpassit_amd import regrid as R, target_grid as tg
    rh = world["bil"]
    rng = np.random.default_rng(8)
    sm, dm = (rng.random(rh.n_src) < 0.1).astype(np.uint8), (rng.random(rh.n_dst) < 0.2).astype(np.uint8)
    masked = R.mask_handle(rh, sm, dm, R.MASKRULE_ROW)
    _shape_kept(masked, rh)
    rowptr, col, val = _csr_of(rh)
    rp, c, v, f, stats = tg.mask_rows(rowptr, col, val, None, sm, dm, tg.MASKRULE_ROW)
    assert stats[0] > 0 and stats[1] > 0
    _same_csr(_csr_of(masked), (rp, c, v))
    assert list(masked.store_stats[1:4]) == [int(s) for s in stats]
    masked.release()


def test_patch(world):
    from mpassit_amd import regrid as R, target_grid as tg
    rh = world["bil"]
    patched = R.patch(rh, world["L"], world["G"])
    _shape_kept(patched, rh)
    idx, w = rh.weights()
    rowptr, col, val, stats = tg.patch_rows(idx, w, world["L"].xyz(), world["G"].xyz(), tg.patch_neighbours_grid(40, 30))
    _same_csr(patched.csr(), (rowptr, col, val))
    assert patched.nnz_per_row == 0 and list(patched.store_stats[1:7]) == [int(s) for s in stats]
    again = R.regrid_store_patch(world["L"], world["G"])          # the wrapper's Grid -> Grid branch for two different grids
    _same_csr(again.csr(), (rowptr, col, val))
    again.release()
    patched.release()


@pytest.mark.parametrize("norm", [GR.NORM_DSTAREA, GR.NORM_FRACAREA])
def test_conserve_2nd(world, norm):
    from mpassit_amd import regrid as R, target_grid as tg
    rh = world["cons"] if norm == GR.NORM_DSTAREA else R.regrid_store_conserve_grid_to_grid(world["L"], world["G"], norm)
    second = R.conserve_2nd(rh, world["L"], world["G"], norm)
    _shape_kept(second, rh)
    rp, col, _ = rh.csr()
    polys = lambda g, nx, ny: tg.conserve2nd_polygons_grid(g.xyz(R.STAGGERLOC_CORNER), nx, ny, g.xyz(R.STAGGERLOC_CENTER))   # noqa: E731
    want = tg.conserve2nd_rows(rp, col, polys(world["L"], 40, 30), polys(world["G"], 60, 40), tg.patch_neighbours_grid(40, 30), norm)
    _same_csr(second.csr(), want)
    again = R.regrid_store_conserve_2nd(world["L"], world["G"], norm)          # the wrapper's Grid -> Grid branch
    _same_csr(again.csr(), want)
    again.release()
    second.release()
    if norm != GR.NORM_DSTAREA:
        rh.release()


def test_compose_with_a_mesh_handle(world):
    """Mesh -> L, then L -> G, folded into one Mesh -> G handle."""
    from mpassit_amd import regrid as R, synth, target_grid as tg
    m = synth.regional_mesh_for_lambert(GR.target("L").proj, 41, 31, 3001, margin=0.3, seed=3)
    mesh = R.Mesh.from_mpas(m)
    inner = R.regrid_store(mesh, world["L"])
    for outer in (world["bil"], world["cons"]):
        both = R.compose(outer, inner)
        assert (both.n_src, both.n_dst, both.nx_dst, both.ny_dst) == (inner.n_src, 2400, 60, 40)
        ca, cb = _csr_of(outer), _csr_of(inner)
        rowptr, col, vals = tg.compose_csr(ca[0], ca[1], ca[2], cb[0], cb[1], cb[2])
        _same_csr(both.csr(), (rowptr, col, vals[0]))
        both.release()
    inner.release()
    mesh.destroy()
