"""The references of the Stores between two grids (tests/_grid_to_grid_ref.py) on the cases of tests/test_grid_to_grid_gpu.py and
tests/test_grid_to_grid_conserve_gpu.py, without a GPU: the conditions that keep a comparison from hiding a failure hold on these
inputs, and deliberately wrong variants -- exchanged slots, the other normalisation, caps tried before quads -- fail the comparisons
the GPU tests make.

The counts below are what the references give for the grids as stated.  (The issue that set these cases quotes 71 / 55 partly covered
and 1290 / 468 empty rows for the conservative L <-> G pair; those are the counts of the UNSHIFTED lat-lon grid, ref_lat = 40, ref_lon =
-92.  The shifted grid G of the cases, the one whose bilinear counts 1031 .. 1095 the same text states, gives 70 / 55 and 1295 / 451.)"""
import numpy as np
import pytest

import _grid_to_grid_ref as GR
import _periodic_to_mesh_ref as PR
import _to_mesh_ref as TR
from _parity_helpers import assert_csr_equal, assert_fixed_weights_equal

ALIGNED = (("L", "N"), ("N", "L"), ("A1", "A2"), ("A2", "A1"), ("L", "L"))


def test_cases_are_the_stated_grids():
    shapes = {n: (GR.target(n).nx, GR.target(n).ny) for n in GR.CASES}
    assert shapes == {"L": (40, 30), "G": (60, 40), "N": (36, 30), "A1": (24, 16), "A2": (48, 32), "W": (72, 36), "W2": (50, 26), "P": (40, 40),
                      "D": (40, 30)}
    assert not GR.target("W").is_regional and not GR.target("W2").is_regional and GR.target("G").is_regional
    # N is a 3 : 1 nest of L with its corners on L's corners: its CORNER point (3 i, 3 j) is L's CORNER point (14 + i, 10 + j)
    l, n = GR.target("L"), GR.target("N")
    assert np.abs(n.lon_c[::3, ::3] - l.lon_c[10:21, 14:27]).max() < 1e-10 and np.abs(n.lat_c[::3, ::3] - l.lat_c[10:21, 14:27]).max() < 1e-10


def test_bilinear_l_g_has_no_ties_and_maps_part_of_the_points(oracle):
    for ss in range(4):
        for ds in range(3):
            idx, w, edge = GR.bilinear(oracle, "L", "G", ss, ds)
            mapped = int((idx[:, 0] >= 0).sum())
            assert 2400 <= idx.shape[0] <= 2460 and 1031 <= mapped <= 1095, (ss, ds, mapped)
            assert TR.edge_share(edge) == 0.0 <= GR.TIE_CAP
            assert np.abs(w[idx[:, 0] >= 0].sum(axis=1) - 1.0).max() < 1e-12
    for ds in range(4):
        idx, w, edge = GR.bilinear(oracle, "G", "L", GR.CENTER, ds)
        assert TR.edge_share(edge) == 0.0 and 0 < int((idx[:, 0] >= 0).sum()) < idx.shape[0]


def test_an_unshifted_g_would_sit_on_the_central_meridian(oracle):
    """Why G is shifted: with ref_lat = 40, ref_lon = -92 its EDGE1 points would lie on L's central meridian -97.5, which is a line of L's
    EDGE1 and CORNER points: 3 % of the mapped points would sit on a quad edge."""
    from mpassit_amd import target_grid as tg
    g0 = tg.define_target_grid_params("lat-lon", 61, 41, dx=0.25, dy=0.25, ref_lat=40.0, ref_lon=-92.0)
    pts = oracle.lonlat_deg_to_xyz(g0.lon_u, g0.lat_u)
    for ss in (GR.EDGE1, GR.CORNER):
        idx, w, edge = TR.to_mesh_bilinear(GR.stagger_xyz(oracle, "L", ss), pts)
        assert 0.02 < TR.edge_share(edge) < 0.04


def test_periodic_sources_have_no_ties_and_the_stated_rows(oracle):
    want = {"P": ((21, 22, 22), (24, 24, 24)), "D": ((0, 0, 0), (114, 124, 118))}
    for dst, (caps, seams) in want.items():
        for ds in range(3):
            for pm in (PR.POLE_NONE, PR.POLE_ALLAVG):
                r = GR.periodic(oracle, "W", dst, ds, pm)
                assert PR.edge_share(r) == 0.0
                assert int((r["kind"] == PR.KIND_CAP).sum()) == (caps[ds] if pm == PR.POLE_ALLAVG else 0)
                assert PR.seam_rows(r).size == seams[ds]
            # under NONE the cap points are empty rows, everything else is the same row
            a, n = GR.periodic(oracle, "W", dst, ds, PR.POLE_ALLAVG), GR.periodic(oracle, "W", dst, ds, PR.POLE_NONE)
            assert np.array_equal(n["kind"] == PR.KIND_NONE, (a["kind"] == PR.KIND_NONE) | (a["kind"] == PR.KIND_CAP))


def test_conservative_l_g_has_no_slivers(oracle):
    counts = {}
    for s, d in (("L", "G"), ("G", "L")):
        rp, col, val, frac = GR.conserve(oracle, s, d)
        assert val.min() >= 1e-9, "no reference entry below 1e-9: SLIVER_CAP holds trivially"
        assert float((val < GR.SLIVER).sum()) / val.size <= GR.SLIVER_CAP
        counts[s] = (int(((frac > 0) & (frac < 1 - 1e-9)).sum()), int((np.diff(rp) == 0).sum()))
    assert counts == {"L": (70, 1295), "G": (55, 451)}, counts


def test_aligned_pairs_separate_noise_from_entries(oracle):
    for s, d in ALIGNED:
        rp, col, val, frac = GR.conserve(oracle, s, d)
        assert not ((val >= 1e-13) & (val < 1e-10)).any(), (s, d)
        assert (val >= 1e-10).sum() > 0.5 * val.size


def test_global_pairs_cover_the_sphere_and_conserve(oracle):
    for n in ("W", "W2"):
        assert abs(GR.cell_areas(oracle, n).sum() - 4.0 * np.pi) < 1e-12
    for s, d in (("W", "W2"), ("W2", "W")):
        dd, ss, inter = GR.conserve_pairs(oracle, s, d)
        a_s, a_d = GR.cell_areas(oracle, s), GR.cell_areas(oracle, d)
        assert np.abs(np.bincount(ss, weights=inter, minlength=a_s.size) - a_s).max() < 2e-16
        assert np.abs(np.bincount(dd, weights=inter, minlength=a_d.size) - a_d).max() < 2e-16
    rp, col, val, frac = GR.conserve(oracle, "W", "P")
    assert np.diff(rp).max() == 72 and (np.diff(rp) == 0).sum() == 0, "P's pole cell has a row of all 72 cells of W's last row"
    rp, col, val, frac = GR.conserve(oracle, "P", "W")
    assert (np.diff(rp) == 0).sum() == 2242


def test_aligned_bilinear_points_sit_on_edges_and_do_not_depend_on_the_tolerance(oracle):
    for s, d in (("L", "N"), ("N", "L"), ("L", "L")):
        idx, w, edge = GR.bilinear(oracle, s, d)
        assert 0.12 <= TR.edge_share(edge) <= 1.0, (s, d)
        x = np.random.default_rng(5).standard_normal(GR.target(s).nx * GR.target(s).ny)
        f = (w * x[np.maximum(idx, 0)]).sum(axis=1)
        for tol in (1e-10 - 1e-11, 1e-10 + 1e-11):
            i2, w2, e2 = GR.bilinear(oracle, s, d, tol=tol)
            assert np.array_equal(idx, i2) and np.array_equal(w, w2)
            assert np.array_equal(f, (w2 * x[np.maximum(i2, 0)]).sum(axis=1))


# ---- wrong variants fail the comparisons of the GPU tests ---------------------------------------------------------------------------
def test_exchanged_slots_fail(oracle):
    idx, w, edge = GR.bilinear(oracle, "L", "G")
    assert assert_fixed_weights_equal(idx, w, idx.copy(), w.copy()) == 0
    wrong = w.copy()
    wrong[:, 1], wrong[:, 2] = w[:, 2], w[:, 1]             # B and C exchanged
    with pytest.raises(AssertionError):
        assert_fixed_weights_equal(idx, w, idx, wrong)
    near = GR.nearest(oracle, "L", "G")
    assert near.min() >= 0 and near.max() < 1200 and np.unique(near).size > 100


def test_the_other_normalisation_fails(oracle):
    for s, d in (("L", "G"), ("G", "L")):
        a, b = GR.conserve(oracle, s, d, GR.NORM_DSTAREA), GR.conserve(oracle, s, d, GR.NORM_FRACAREA)
        n_src = GR.target(s).nx * GR.target(s).ny
        tol = GR.tol_grids(oracle, s, d)
        assert_csr_equal(a[0], a[1], a[2], a[0], a[1], a[2].copy(), n_src, tol=tol)
        with pytest.raises(AssertionError):
            assert_csr_equal(a[0], a[1], a[2], b[0], b[1], b[2], n_src, tol=tol)
        rows = np.repeat(np.arange(a[0].size - 1), np.diff(a[0]))
        assert np.abs(np.bincount(rows, weights=b[2], minlength=a[0].size - 1)[np.diff(a[0]) > 0] - 1.0).max() < 1e-12
        assert np.abs(np.bincount(rows, weights=a[2], minlength=a[0].size - 1) - a[3]).max() < 1e-12


def test_caps_before_quads_fail(oracle):
    """A cap tried before the quads takes the points ON the chord between two neighbours of an end row (a quad passes there, so the row is
    a quad row); away from every edge the order cannot matter, which is why the cases above have no ties."""
    cen = GR.stagger_xyz(oracle, "W", GR.CENTER)
    ny, nx, _ = cen.shape
    a = np.array([0, 1, nx // 2, nx - 1])
    mid = np.concatenate([cen[ny - 1, a] + cen[ny - 1, (a + 1) % nx], cen[0, a] + cen[0, (a + 1) % nx]])
    mid /= np.linalg.norm(mid, axis=1, keepdims=True)
    good, wrong = PR.periodic_to_mesh(oracle, cen, mid), PR.periodic_to_mesh(oracle, cen, mid, mutate="caps_first")
    assert np.all(good["kind"] == PR.KIND_QUAD) and np.all(wrong["kind"] == PR.KIND_CAP)
    # (as sparse vectors the two rows agree -- the pole's share is zero on the chord --, so it is the row KINDS the GPU test holds)
    assert np.all(np.diff(good["rowptr"]) == 4) and np.all(np.diff(wrong["rowptr"]) == nx)
    same = GR.periodic(oracle, "W", "P", mutate="caps_first")
    assert np.array_equal(same["rowptr"], GR.periodic(oracle, "W", "P")["rowptr"])
