"""The conservative Store between two grids on the GPU (mpg_regrid_store_conserve_grid_to_grid, k_store_conserve_grid.hip) against the
float64 reference of its rule (tests/_grid_to_grid_ref.py over tests/_mesh_conserve_ref.py): both norms on every case, the dst fraction,
the row properties, conservation between two global grids, the reciprocity of the two directions, determinism, cache and refusals.

Cases (tests/_grid_to_grid_ref.py; qualified without a GPU by tests/test_grid_to_grid_ref.py): L <-> G in general position, the
aligned pairs L <-> N (a 3 : 1 nest), A1 <-> A2 (lat-lon 1 : 2) and L -> L, whose cells share sides, the global grids W <-> W2 and W <-> P
with P's pole cell.  tol = max(1e-11, 64 eps / min h), h = area / diameter over BOTH grids' cells.  The reference clips the CORNER unit
vectors the device grids hold (Grid.xyz), not its own lon / lat -> xyz: both sides see the same polygons."""
import ctypes as C

import numpy as np
import pytest

import _grid_to_grid_ref as GR
from _parity_helpers import assert_csr_equal

pytestmark = pytest.mark.gpu

GENERAL = (("L", "G"), ("G", "L"), ("W", "W2"), ("W2", "W"), ("W", "P"), ("P", "W"))
ALIGNED = (("L", "N"), ("N", "L"), ("A1", "A2"), ("A2", "A1"), ("L", "L"))


@pytest.fixture(scope="module")
def grids(gpu_lib):
    """One device grid per case name, made on first use from its TargetGrid (CORNER coordinates included), destroyed at the end."""
    from mpassit_amd import regrid as R
    made = {}

    def get(name):
        if name not in made:
            made[name] = R.Grid.from_target(GR.target(name))
        return made[name]
    get.corners = _Corners(get)
    yield get
    for g in made.values():
        g.destroy()


class _Corners(dict):
    """name -> [(ny + 1) * (nx + 1)][3]: the CORNER unit vectors the device grid of a case holds (Grid.xyz), read on first use.  The
    reference clips these, so that both sides see the same polygons: a strip of relative width 1e-8 along an almost-shared side (N's
    outline on L's cell lines) has an area that the last bit of a coordinate decides."""

    def __init__(self, get):
        super().__init__()
        self._get = get

    def __missing__(self, name):
        from mpassit_amd import regrid as R
        xyz = np.ascontiguousarray(self._get(name).xyz(R.STAGGERLOC_CORNER).T)
        xyz.setflags(write=False)
        self[name] = xyz
        return xyz


def _csr_bytes(rh):
    rp, col, val = rh.csr()
    return rp.tobytes(), col.tobytes(), val.tobytes(), rh.dst_frac().tobytes()


def _check(oracle, grids, s, d, norm, aligned):
    from mpassit_amd import regrid as R
    rh = R.regrid_store_conserve_grid_to_grid(grids(s), grids(d), norm)
    ts, td = GR.target(s), GR.target(d)
    assert (rh.n_src, rh.n_dst, rh.nx_dst, rh.ny_dst, rh.nnz_per_row) == (ts.nx * ts.ny, td.nx * td.ny, td.nx, td.ny, 0)
    assert rh.store_path == 0 and rh.store_ms > 0.0
    rp, col, val = rh.csr()
    frac = rh.dst_frac()
    ref = GR.conserve(oracle, s, d, norm, grids.corners)
    tol = GR.tol_grids(oracle, s, d, grids.corners)
    if not aligned:   # (the aligned pairs are full of legitimate one-sided noise entries: the one-sided rule SLIVER separates them instead)
        assert float((ref[2] < GR.SLIVER).sum()) / ref[2].size <= GR.SLIVER_CAP
    common, only_r, only_g = assert_csr_equal(ref[0], ref[1], ref[2], rp, col, val, rh.n_src, tol=tol)
    dd, ss, inter = GR.conserve_pairs(oracle, s, d, grids.corners)
    st = rh.store_stats
    print("%s -> %s norm %d: nnz %d (reference %d), common %d, only reference %d, only gpu %d, pairs clipped %d (reference's positive %d), "
          "slots %d, tol %.3g, max |frac diff| %.3g, %.3f ms" % (s, d, norm, col.size, ref[1].size, common, only_r, only_g, st[1], int((inter > 0).sum()),
                                                                  st[6], tol, np.abs(frac - ref[3]).max(), rh.store_ms))
    assert common > 0.5 * ref[1].size
    if not aligned:
        assert only_r == 0 and only_g == 0
    assert st[1] >= int((inter > 0).sum()) and st[6] >= 8
    assert np.abs(frac - ref[3]).max() < tol
    inside = np.ones(max(col.size - 1, 0), bool)               # pairs (q, q + 1) of one row
    cuts = rp[1:-1]
    inside[cuts[(cuts > 0) & (cuts < col.size)] - 1] = False
    assert np.all(np.diff(col)[inside] > 0), "columns strictly ascending within a row"
    rows = np.repeat(np.arange(rh.n_dst), np.diff(rp))
    sums = np.bincount(rows, weights=val, minlength=rh.n_dst)
    full = np.diff(rp) > 0
    if norm == GR.NORM_FRACAREA:
        assert np.abs(sums[full] - 1.0).max() < 1e-12
    else:
        assert np.abs(sums - frac).max() < 1e-12
    assert np.all(frac[~full] == 0.0), "an uncovered cell has an empty row and no fraction"
    real = lambda rowptr, v: np.bincount(np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr)), weights=v >= GR.SLIVER, minlength=rowptr.size - 1) > 0   # noqa: E731
    assert np.array_equal(real(rp, val), real(ref[0], ref[2])), "the same cells are covered"
    if not aligned:
        assert np.array_equal(np.diff(rp) == 0, np.diff(ref[0]) == 0)
    return rh, (rp, col, val, frac)


@pytest.mark.parametrize("norm", [GR.NORM_DSTAREA, GR.NORM_FRACAREA])
@pytest.mark.parametrize("pair", GENERAL, ids=["%s-%s" % p for p in GENERAL])
def test_parity_general_position(oracle, grids, pair, norm):
    rh, _ = _check(oracle, grids, pair[0], pair[1], norm, aligned=False)
    rh.release()


@pytest.mark.parametrize("norm", [GR.NORM_DSTAREA, GR.NORM_FRACAREA])
@pytest.mark.parametrize("pair", ALIGNED, ids=["%s-%s" % p for p in ALIGNED])
def test_parity_aligned_pairs(oracle, grids, pair, norm):
    """Cells that share sides: every clip meets vertices ON its plane.  The Store must serve them (MPG_ERR_OVERFLOW here would be a finding
    about the clip's vertex slots), and what differs from the reference must be noise below SLIVER."""
    rh, (rp, col, val, frac) = _check(oracle, grids, pair[0], pair[1], norm, aligned=True)
    if pair == ("L", "L"):
        diag = val[val > 0.5]
        assert diag.size == rh.n_dst and np.abs(frac - 1.0).max() < 1e-11, "a grid onto itself: the diagonal"
    rh.release()


def test_pole_cell_and_empty_rows(oracle, grids):
    from mpassit_amd import regrid as R
    rh = R.regrid_store_conserve_grid_to_grid(grids("W"), grids("P"))
    rp, col, val = rh.csr()
    assert np.diff(rp).max() == 72 and np.diff(rp).min() > 0, "P's pole cell takes all 72 cells of W's last row"
    rh.release()
    rh = R.regrid_store_conserve_grid_to_grid(grids("P"), grids("W"))
    assert int((np.diff(rh.csr()[0]) == 0).sum()) == 2242
    rh.release()


@pytest.mark.parametrize("pair", [("W", "W2"), ("W2", "W")], ids=["W-W2", "W2-W"])
def test_conservation_between_global_grids(oracle, grids, pair):
    import torch
    from mpassit_amd import regrid as R
    s, d = pair
    rh = R.regrid_store_conserve_grid_to_grid(grids(s), grids(d))
    a_s, a_d = GR.cell_areas(oracle, s, grids.corners), GR.cell_areas(oracle, d, grids.corners)
    x = np.random.default_rng(3).standard_normal(rh.n_src)
    y = rh.regrid_typed(torch.as_tensor(x, device="cuda")).cpu().numpy().reshape(-1)
    tol = GR.tol_grids(oracle, s, d, grids.corners)
    lhs, rhs = float((a_d * y).sum()), float((a_s * x).sum())
    print("%s -> %s: integral %.17g vs %.17g, bar %.3g" % (s, d, lhs, rhs, tol * float((a_s * np.abs(x)).sum())))
    assert abs(lhs - rhs) <= tol * float((a_s * np.abs(x)).sum())
    rh.release()


def test_reciprocity_of_the_two_directions(oracle, grids):
    """area_d A[d][s] and area_s B[s][d] are the same intersection I(d, s) clipped the other way round."""
    from mpassit_amd import regrid as R
    a, b = R.regrid_store_conserve_grid_to_grid(grids("L"), grids("G")), R.regrid_store_conserve_grid_to_grid(grids("G"), grids("L"))
    area_l, area_g = GR.cell_areas(oracle, "L", grids.corners), GR.cell_areas(oracle, "G", grids.corners)
    tol = GR.tol_grids(oracle, "L", "G", grids.corners)
    (rpa, ca, va), (rpb, cb, vb) = a.csr(), b.csr()
    ra, rb = np.repeat(np.arange(a.n_dst), np.diff(rpa)), np.repeat(np.arange(b.n_dst), np.diff(rpb))
    ka, kb = ra.astype(np.int64) * b.n_dst + ca, cb.astype(np.int64) * b.n_dst + rb          # (G cell, L cell) on both sides
    oa, ob = np.argsort(ka), np.argsort(kb)
    assert np.array_equal(ka[oa], kb[ob]), "the two directions hold the same pairs"
    ia, ib = area_g[ra[oa]] * va[oa], area_l[rb[ob]] * vb[ob]
    worst = np.abs(ia - ib) / np.maximum(area_g[ra[oa]], area_l[rb[ob]])
    print("reciprocity: worst |area_d A - area_s B| / area %.3g (bar %.3g) over %d pairs" % (worst.max(), tol, ka.size))
    assert worst.max() < tol
    a.release()
    b.release()


def test_determinism_cache_and_refusals(gpu_lib, oracle, grids):
    from mpassit_amd import _lib as L, regrid as R
    lib = L.load()
    # fresh objects twice: the same bytes
    got = []
    for trial in range(2):
        gs, gd = R.Grid.from_target(GR.target("G")), R.Grid.from_target(GR.target("L"))
        rh = R.regrid_store_conserve_grid_to_grid(gs, gd, GR.NORM_FRACAREA)
        got.append(_csr_bytes(rh))
        rh.release()
        gs.destroy()
        gd.destroy()
    assert got[0] == got[1]
    # the second Store returns the cached handle; norms and directions are distinct handles
    gl, gg = grids("L"), grids("G")
    a, a2 = R.regrid_store_conserve_grid_to_grid(gl, gg), R.regrid_store_conserve_grid_to_grid(gl, gg)
    f, back = R.regrid_store_conserve_grid_to_grid(gl, gg, GR.NORM_FRACAREA), R.regrid_store_conserve_grid_to_grid(gg, gl)
    assert a._h.value == a2._h.value and len({a._h.value, f._h.value, back._h.value}) == 3
    addr = a._h.value
    for rh in (a, a2, f, back):
        rh.release()
    again = R.regrid_store_conserve_grid_to_grid(gl, gg)
    assert again._h.value == addr, "a released handle stays parked"
    again.release()
    # destroying EITHER grid drops the parked entry: a new grid, at whatever address (a recycled one must never hit), stores anew -- the
    # replacement has the OTHER grid's shape, so a stale entry would show in the handle's sizes
    for which in (0, 1):
        gs, gd = R.Grid.from_target(GR.target("A1")), R.Grid.from_target(GR.target("A2"))
        first = R.regrid_store_conserve_grid_to_grid(gs, gd)
        assert (first.n_src, first.n_dst) == (24 * 16, 48 * 32)
        first.release()
        (gs, gd)[which].destroy()
        fresh = R.Grid.from_target(GR.target("A2" if which == 0 else "A1"))
        pair = (fresh, gd) if which == 0 else (gs, fresh)
        second = R.regrid_store_conserve_grid_to_grid(*pair)
        assert (second.n_src, second.n_dst) == ((48 * 32, 48 * 32) if which == 0 else (24 * 16, 24 * 16))
        assert np.abs(second.dst_frac() - 1.0).max() < 1e-11, "the same cells on both sides"
        second.release()
        for g in pair:
            g.destroy()
    # refusals
    def refused(rc, want, *words):
        msg = lib.mpg_last_error().decode()
        assert rc == want and msg.startswith("mpg_regrid_store_conserve_grid_to_grid"), (rc, want, msg)
        for w in words:
            assert w in msg, msg

    h = C.c_void_p()
    refused(L.regrid_store_conserve_grid_to_grid(None, gg._h, 0, C.byref(h)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(L.regrid_store_conserve_grid_to_grid(gl._h, None, 0, C.byref(h)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(L.regrid_store_conserve_grid_to_grid(gl._h, gg._h, 0, None), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(L.regrid_store_conserve_grid_to_grid(gl._h, gg._h, 2, C.byref(h)), L.MPG_ERR_INVALID_ARG, "MPG_NORM_DSTAREA or MPG_NORM_FRACAREA")
    t = GR.target("L")
    bare = R.Grid(t.lon, t.lat)
    refused(L.regrid_store_conserve_grid_to_grid(bare._h, gg._h, 0, C.byref(h)), L.MPG_ERR_INVALID_ARG, "source grid", "CORNER", "create the grid with them")
    refused(L.regrid_store_conserve_grid_to_grid(gg._h, bare._h, 0, C.byref(h)), L.MPG_ERR_INVALID_ARG, "destination grid", "CORNER")
    assert h.value is None, "a refused call leaves *out alone"
    bare.destroy()
    fx = R.regrid_store_grid_to_grid(gl, gg)
    with pytest.raises(L.MpgError) as e:
        fx.dst_frac()
    assert "mpg_regrid_store_conserve_grid_to_grid" in str(e.value)
    fx.release()
