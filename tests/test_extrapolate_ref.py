"""The numpy mirror of mpg_handle_extrapolate (target_grid.extrapolate_rows) on the CPU: nearest-source-to-destination equals the oracle's
brute-force nearest search; the inverse-distance weights agree with a 50-digit mpmath evaluation of (1/d^e) / sum(1/d^e) from the same
squared distances within a derived bound; the rules at the edges (coincident points, fewer sources than N, exact ties); and the unmapped
counts of the Stores the GPU tests extrapolate, from the CPU oracle: the numbers the feature was asked for with.

The bound.  w_i = t_i / S with r_i = d2_0 / d2_i (one rounding: 0.5 eps relative, e / 2 times that after the power: 0.25 e eps), t_i =
pow(r_i, e / 2) (B eps, B the ulp bound of the platform's pow; exact for e == 2), S the ordered sum (0.5 (K - 1) eps on top of its terms'
B + 0.25 e) and the division (0.5 eps): (2 B + 0.5 e + 0.5 K) eps relative, eps = 2^-52.  B_HOST = 1: glibc documents pow within 1 ulp."""
import numpy as np
import pytest

from conftest import LAMBERT

EPS = 2.0 ** -52
B_HOST = 1


def _unit(rng, n):
    v = rng.normal(size=(3, n))
    return v / np.sqrt((v * v).sum(axis=0))


def _d2(src, p):
    dx, dy, dz = (p[k] - src[k] for k in range(3))
    return (dx * dx + dy * dy) + dz * dz


def test_stod_is_the_oracles_brute_force_nearest(oracle):
    from mpassit_amd import target_grid as tg
    rng = np.random.default_rng(27)
    src, dst = _unit(rng, 700), _unit(rng, 300)
    src[:, 5] = src[:, 2]                                   # an exact duplicate: the lower id wins
    dst[:, 7] = src[:, 5]
    unmapped = rng.random(300) < 0.4
    unmapped[[0, 7, 299]] = True
    rowlen, ids, w = tg.extrapolate_rows(src, dst, unmapped, tg.EXTRAPMETHOD_NEAREST_STOD)
    rows = np.flatnonzero(unmapped)
    want = oracle.nearest(np.ascontiguousarray(src.T), np.ascontiguousarray(dst.T[rows]), brute=True)
    assert ids.shape == (rows.size, 1) and np.array_equal(ids[:, 0], want) and (rowlen == 1).all() and (w == 1.0).all()
    assert ids[np.searchsorted(rows, 7), 0] == 2
    # row numbers instead of a mask, in any order: the same rows in ascending order
    again = tg.extrapolate_rows(src, dst, rows[::-1].copy(), tg.EXTRAPMETHOD_NEAREST_STOD)
    assert all(np.array_equal(a, b) for a, b in zip(again, (rowlen, ids, w)))


@pytest.mark.parametrize("e", [2.0, 1.0, 3.5, 0.5])
@pytest.mark.parametrize("N", [1, 2, 3, 4, 8])
def test_idavg_against_mpmath(N, e):
    import mpmath
    from mpassit_amd import target_grid as tg
    mpmath.mp.dps = 50
    rng = np.random.default_rng(100 + N)
    src, dst = _unit(rng, 400), _unit(rng, 60)
    rowlen, ids, w = tg.extrapolate_rows(src, dst, np.ones(60, bool), tg.EXTRAPMETHOD_NEAREST_IDAVG, N, e)
    assert ids.shape == (60, N) and (rowlen == N).all()
    bar = (2 * B_HOST + 0.5 * e + 0.5 * N) * EPS if e != 2.0 else (0.5 * 2.0 + 0.5 * N) * EPS
    worst = 0.0
    for u in range(60):
        d2 = _d2(src, dst[:, u])
        order = np.lexsort((np.arange(400), d2))[:N]
        assert np.array_equal(ids[u], order)
        t = [mpmath.mpf(1) / mpmath.power(mpmath.mpf(float(d2[c])), mpmath.mpf(e) / 2) for c in order]     # 1 / d^e, d = sqrt(d2)
        S = mpmath.fsum(t)
        for i in range(N):
            exact = t[i] / S
            worst = max(worst, float(abs(mpmath.mpf(float(w[u, i])) - exact) / exact))
        assert (np.diff(w[u]) <= 0).all() and abs(w[u].sum() - 1.0) <= N * EPS
    print("N = %d, e = %g: worst relative error %.3g eps, bar %.3g eps" % (N, e, worst / EPS, bar / EPS))
    assert worst <= bar


def test_the_rules_at_the_edges():
    from mpassit_amd import target_grid as tg
    rng = np.random.default_rng(3)
    src, dst = _unit(rng, 5), _unit(rng, 9)
    # fewer sources than N: every row takes them all
    rowlen, ids, w = tg.extrapolate_rows(src, dst, np.ones(9, bool), tg.EXTRAPMETHOD_NEAREST_IDAVG, 8, 2.0)
    assert ids.shape == (9, 5) and (rowlen == 5).all() and all(sorted(r) == [0, 1, 2, 3, 4] for r in ids.tolist())
    # a coincident point: one entry of weight 1, the ids behind it -1 and the weights 0
    dst[:, 4] = src[:, 3]
    rowlen, ids, w = tg.extrapolate_rows(src, dst, np.ones(9, bool), tg.EXTRAPMETHOD_NEAREST_IDAVG, 3, 1.0)
    assert rowlen[4] == 1 and ids[4].tolist() == [3, -1, -1] and w[4].tolist() == [1.0, 0.0, 0.0] and (np.delete(rowlen, 4) == 3).all()
    # exact ties: equal distances to duplicated sources go to the lower id, at the last rank too
    dup = np.concatenate([src, src, src], axis=1)                       # ids c, c + 5, c + 10 coincide
    rowlen, ids, w = tg.extrapolate_rows(dup, _unit(rng, 6), np.ones(6, bool), tg.EXTRAPMETHOD_NEAREST_IDAVG, 4, 2.0)
    for r, ww in zip(ids.tolist(), w):
        assert r[1] == r[0] + 5 and r[2] == r[0] + 10 and r[0] < 5 and r[3] < 5 and r[3] != r[0]
        assert ww[0] == ww[1] == ww[2] and ww[3] < ww[2]
    # nothing to fill, nothing to fill from, an unknown method
    rowlen, ids, w = tg.extrapolate_rows(src, dst, np.zeros(9, bool))
    assert rowlen.size == 0 and ids.shape == (0, 1)
    rowlen, ids, w = tg.extrapolate_rows(np.empty((3, 0)), dst, np.ones(9, bool), tg.EXTRAPMETHOD_NEAREST_IDAVG, 4)
    assert (rowlen == 0).all() and ids.shape == (9, 0)
    with pytest.raises(ValueError):
        tg.extrapolate_rows(src, dst, np.ones(9, bool), method=7)


def test_the_gaps_the_feature_fills(oracle):
    """The unmapped counts of the CPU oracle's Stores on the 61 x 41 Lambert grid (60 x 40 mass points) and the two meshes of
    tests/test_to_mesh_gpu.py, and the mirror's rows for them: as many as are unmapped, each with a nearest source."""
    from mpassit_amd import synth, target_grid as tg
    o = oracle
    g = tg.define_target_grid_params("lambert", 61, 41, dx=30000.0, dy=30000.0, **LAMBERT)
    m_in = synth.regional_mesh_for_lambert(g.proj, 61, 41, 5003, margin=-0.08, seed=12)
    m_over = synth.regional_mesh_for_lambert(g.proj, 61, 41, 6001, margin=0.05, seed=11)
    assert (m_in.nCells, m_over.nCells) == (5084, 6030)
    cell = lambda m: o.lonlat_deg_to_xyz(*o.mesh_coords_deg(m.lonCell, m.latCell))     # noqa: E731
    centre = o.lonlat_deg_to_xyz(g.lon, g.lat)
    xin, xover = cell(m_in), cell(m_over)
    tri, _ = o.dual_triangles(m_in.verticesOnCell, m_in.nVertices, xin)
    counts = {}
    gaps = {}
    for name, pts in (("mesh to grid", centre), ("mesh to mesh", xover)):
        idx, _ = o.bilinear_weights(xin, tri, pts)[:2]
        gaps[name] = (xin, pts, idx[:, 0] < 0)
    for name, st, lon, lat in (("edge1", 1, g.lon_u, g.lat_u), ("edge2", 2, g.lon_v, g.lat_v)):
        pts = o.lonlat_deg_to_xyz(lon, lat)
        idx, _ = o.grid_bilinear(g.nx, g.ny, centre, st, pts)[:2]
        gaps[name] = (centre, pts, idx[:, 0] < 0)
    for name, (src, pts, unmapped) in gaps.items():
        counts[name] = (int(unmapped.sum()), unmapped.size)
        rowlen, ids, w = tg.extrapolate_rows(src.T, pts.T, unmapped)
        assert rowlen.size == unmapped.sum() and (rowlen == 1).all() and (ids >= 0).all() and (ids < src.shape[0]).all()
        assert np.array_equal(ids[:, 0], o.nearest(src, np.ascontiguousarray(pts[unmapped]), brute=True))
    print(counts)
    assert counts == {"mesh to grid": (717, 2400), "mesh to mesh": (2577, 6030), "edge1": (80, 2440), "edge2": (156, 2460)}
    u1 = gaps["edge1"][2].reshape(g.ny, g.nx + 1)
    assert u1[:, [0, g.nx]].all() and not u1[:, 1:g.nx].any(), "the outermost U columns, and only they"
    u2 = gaps["edge2"][2].reshape(g.ny + 1, g.nx)
    assert u2[[0, g.ny], :].all(), "the outermost V rows (and part of the end columns)"
