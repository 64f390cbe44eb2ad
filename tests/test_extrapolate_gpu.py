"""Extrapolation on the GPU at small sizes (mpg_handle_extrapolate): the new rows against the numpy mirror (target_grid.extrapolate_rows and
its two halves) fed with the library's own unit vectors (Mesh.xyz / Grid.xyz) -- columns exactly, values BIT FOR BIT for
nearest-source-to-destination and for e == 2.0, within the derived bound of a 50-digit mpmath evaluation for other exponents -- on every
geometry pairing, at the smallest shapes, under every consumer, through the wind chain, and the refusals.

The bound for e != 2.0 (tests/test_extrapolate_ref.py derives it): (2 B + 0.5 e + 0.5 K) eps relative, eps = 2^-52, B the ulp bound of the
device pow.  The ROCm installation documents no ulp bound for pow, so B was measured: tools/extrapolate_probe.py --pow-ulp evaluates the
device pow (through torch.pow, not through the library) over the r_i of these very pairings against mpmath; the largest error was
1.25 ulp (e = 3.5; 0.5 ulp for e = 1.0: profiles/r27_extrapolate.md), rounded up: B = 2."""
import ctypes as C

import numpy as np
import pytest

import _contract_ref as cr
from conftest import LAMBERT

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
B_DEVICE_POW = 2
OPTIONS = [("stod", 1, 2.0)] + [("idavg", N, e) for N in (1, 3, 4, 8) for e in (2.0, 1.0, 3.5)]
PAIRINGS = ("m2g", "m2m", "g2m cells", "g2m edges", "g2g e1", "g2g e2", "cons", "pole none")
A3 = (-1, -2, 0, 1, 2)           # the "a3_staged" and "lf_variant" settings of tests/test_contract_gpu.py
LFV = (-1, 0, 1, 2)


def _method(R, name):
    return R.EXTRAPMETHOD_NEAREST_STOD if name == "stod" else R.EXTRAPMETHOD_NEAREST_IDAVG


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _rows_of(rh):
    """(unmapped mask, rowptr, col, val) of any handle without pole terms; a fixed one's slots in slot order, -1 entries dropped"""
    from mpassit_amd import target_grid as tg
    if rh.nnz_per_row == 0:
        rowptr, col, val = rh.csr()
        return np.diff(rowptr) == 0, rowptr, col, val
    idx, w = rh.weights()
    rowptr, col, val = tg.fixed_to_csr(idx, w)
    return idx[:, 0] < 0, rowptr, col, val


def _expected_csr(rh, rows, rowlen, ids, w):
    """the CSR output: mapped rows as they are, row rows[u] = ids[u, :rowlen[u]] with w"""
    unmapped, rowptr, col, val = _rows_of(rh)
    lens = np.diff(rowptr).astype(np.int64)
    lens[rows] = rowlen
    out_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    out_col, out_val = np.empty(out_ptr[-1], np.int32), np.empty(out_ptr[-1])
    keep = np.ones(rh.n_dst, bool)
    keep[rows] = False
    src_pos = np.concatenate([np.arange(rowptr[i], rowptr[i + 1]) for i in np.flatnonzero(keep)] or [np.empty(0, np.int64)]).astype(np.int64)
    dst_pos = np.concatenate([np.arange(out_ptr[i], out_ptr[i + 1]) for i in np.flatnonzero(keep)] or [np.empty(0, np.int64)]).astype(np.int64)
    out_col[dst_pos], out_val[dst_pos] = col[src_pos], val[src_pos]
    for u, i in enumerate(rows):
        out_col[out_ptr[i]:out_ptr[i + 1]] = ids[u, :rowlen[u]]
        out_val[out_ptr[i]:out_ptr[i + 1]] = w[u, :rowlen[u]]
    return out_ptr, out_col, out_val


def _expected_fixed(rh, rows, rowlen, ids, w):
    idx, wt = rh.weights()
    idx, wt = idx.copy(), wt.copy()
    S = rh.nnz_per_row
    for u, i in enumerate(rows):
        k = rowlen[u]
        idx[i, :k], wt[i, :k] = ids[u, :k], w[u, :k]
        idx[i, k:], wt[i, k:] = ids[u, 0], 0.0
    if S == 1:
        wt = (idx >= 0).astype(np.float64)       # a nearest handle has no weight array: weights() reports 1.0 where mapped
    return idx, wt


def _mp_terms(d2k, e):
    """1 / d^e = d2^(-e / 2) of every neighbour at 50 digits, a list of lists of mpf (None for a row whose nearest point coincides)"""
    import mpmath
    mpmath.mp.dps = 50
    return [None if row[0] == 0.0 else [mpmath.mpf(1) / mpmath.power(mpmath.mpf(float(x)), mpmath.mpf(e) / 2) for x in row] for row in d2k]


def _within_bound(w, terms, K, e, what):
    """w [n][>= K] against (1 / d^e) / sum over the K nearest of (1 / d^e), relative, within (2 B + 0.5 e + 0.5 K) eps"""
    import mpmath
    bar = (2 * B_DEVICE_POW + 0.5 * e + 0.5 * K) * EPS
    worst = 0.0
    for wr, t in zip(w, terms):
        if t is None:
            assert wr[0] == 1.0 and (wr[1:] == 0.0).all(), what
            continue
        S = mpmath.fsum(t[:K])
        for x, y in zip(wr[:K], t[:K]):
            worst = max(worst, float(abs(mpmath.mpf(float(x)) - y / S) / (y / S)))
    print("%s: worst relative error %.3g eps, bar %.3g eps" % (what, worst / EPS, bar / EPS))
    assert worst <= bar, (what, worst / EPS, bar / EPS)


def _check(R, tg, rh, out, rows, ids8, d28, name, N, e, what, mp_cache=None):
    """`out` = extrapolate(rh, ...) against the mirror: the kind, the mapped rows, the pattern and the values of the new rows"""
    method = _method(R, name)
    K = min(N if name == "idavg" else 1, ids8.shape[1])
    ids, d2k = ids8[:, :K], d28[:, :K]
    rowlen, w = tg.extrapolate_weights(d2k, method, e)
    exact_bits = name == "stod" or e == 2.0
    assert (out.n_src, out.n_dst, out.nx_dst, out.ny_dst) == (rh.n_src, rh.n_dst, rh.nx_dst, rh.ny_dst)
    stats = out.store_stats
    assert stats[1] == (rows.size if K else 0) and stats[2] == K, (what, stats[:3], rows.size, K)
    fixed = rh.nnz_per_row > 0 and (name == "stod" or N <= rh.nnz_per_row)
    if fixed:
        assert out.nnz_per_row == rh.nnz_per_row, what
        want_idx, want_w = _expected_fixed(rh, rows, rowlen, ids, w)
        got_idx, got_w = out.weights()
        assert np.array_equal(got_idx, want_idx), what
        keep = np.ones(rh.n_dst, bool)
        keep[rows] = False
        assert np.array_equal(_bits(got_w[keep]), _bits(want_w[keep])), (what, "mapped rows")
        if exact_bits:
            assert np.array_equal(_bits(got_w), _bits(want_w)), what
        else:
            assert np.array_equal(_bits(got_w[rows][:, K:]), _bits(want_w[rows][:, K:])), (what, "the +0.0 slots")
            _within_bound(got_w[rows], mp_cache(e), K, e, what)
        return
    assert out.nnz_per_row == 0, what
    want = _expected_csr(rh, rows, rowlen, ids, w)
    got = out.csr()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
    assert out.nnz == want[1].size
    new = np.zeros(want[1].size, bool)
    for i in rows:
        new[want[0][i]:want[0][i + 1]] = True
    assert np.array_equal(_bits(got[2][~new]), _bits(want[2][~new])), (what, "mapped rows")
    if exact_bits:
        assert np.array_equal(_bits(got[2]), _bits(want[2])), what
    else:
        gw = np.zeros((rows.size, max(K, 1)))
        for u, i in enumerate(rows):
            gw[u, :rowlen[u]] = got[2][got[0][i]:got[0][i + 1]]
        _within_bound(gw, mp_cache(e), K, e, what)


@pytest.fixture(scope="module")
def world(gpu_lib):
    from mpassit_amd import regrid as R, synth, target_grid as tg
    g = tg.define_target_grid_params("lambert", 61, 41, dx=30000.0, dy=30000.0, **LAMBERT)
    m_in = synth.regional_mesh_for_lambert(g.proj, 61, 41, 5003, margin=-0.08, seed=12)
    m_over = synth.mesh_edges(synth.regional_mesh_for_lambert(g.proj, 61, 41, 6001, margin=0.05, seed=11))
    gp = tg.define_target_grid_params("lat-lon", nx=25, ny=13, stand_lon=0.0, is_regional=False)
    obj = dict(grid=R.Grid.from_target(g), mesh_in=R.Mesh.from_mpas(m_in), mesh_over=R.Mesh.from_mpas(m_over), per=R.Grid.from_target(gp),
               vor=R.Mesh.from_mpas(synth.global_voronoi_mesh(1500)))
    assert (m_in.nCells, m_over.nCells) == (5084, 6030) and obj["mesh_over"].nEdges > 0 and obj["mesh_in"].nEdges == 0
    E, C_, E1, E2, EDGE = R.MESHLOC_ELEMENT, R.STAGGERLOC_CENTER, R.STAGGERLOC_EDGE1, R.STAGGERLOC_EDGE2, R.MESHLOC_EDGE
    BIL, NEAR = R.REGRIDMETHOD_BILINEAR, R.REGRIDMETHOD_NEAREST_STOD
    o = obj
    # name -> (handle, src, src_loc, dst, dst_loc, the library's own nearest Store of the pair or None)
    pairs = {
        "m2g": (R.regrid_store(o["mesh_in"], o["grid"], BIL), o["mesh_in"], E, o["grid"], C_, lambda: R.regrid_store(o["mesh_in"], o["grid"], NEAR)),
        "m2m": (R.regrid_store_mesh(o["mesh_in"], o["mesh_over"], BIL), o["mesh_in"], E, o["mesh_over"], E,
                lambda: R.regrid_store_mesh(o["mesh_in"], o["mesh_over"], NEAR)),
        "g2m cells": (R.regrid_store_to_mesh(o["grid"], o["mesh_over"], BIL), o["grid"], C_, o["mesh_over"], E,
                      lambda: R.regrid_store_to_mesh(o["grid"], o["mesh_over"], NEAR)),
        "g2m edges": (R.regrid_store_to_mesh(o["grid"], o["mesh_over"], BIL, meshloc=EDGE), o["grid"], C_, o["mesh_over"], EDGE,
                      lambda: R.regrid_store_to_mesh(o["grid"], o["mesh_over"], NEAR, meshloc=EDGE)),
        "g2g e1": (R.regrid_store_grid(o["grid"], E1), o["grid"], C_, o["grid"], E1, None),
        "g2g e2": (R.regrid_store_grid(o["grid"], E2), o["grid"], C_, o["grid"], E2, None),
        "cons": (R.regrid_store(o["mesh_in"], o["grid"], R.REGRIDMETHOD_CONSERVE), o["mesh_in"], E, o["grid"], C_,
                 lambda: R.regrid_store(o["mesh_in"], o["grid"], NEAR)),
        "pole none": (R.regrid_store_periodic_to_mesh(o["per"], o["vor"], pole_method=R.POLEMETHOD_NONE), o["per"], C_, o["vor"], E,
                      lambda: R.regrid_store_to_mesh(o["per"], o["vor"], NEAR)),
    }
    d = dict(g=g, obj=obj, pairs=pairs, nb={}, filled={})
    yield d
    for h in list(d["filled"].values()) + [p[0] for p in pairs.values()]:
        h.release()
    for x in obj.values():
        x.destroy()


def _neighbours(world, name):
    """(rows, ids [nu][9], d2 [nu][9]) of a pairing's unmapped rows from the mirror, once"""
    from mpassit_amd import target_grid as tg
    if name not in world["nb"]:
        rh, src, sloc, dst, dloc, _ = world["pairs"][name]
        rows = np.flatnonzero(_rows_of(rh)[0])
        ids, d2 = tg.extrapolate_neighbours(src.xyz(sloc), dst.xyz(dloc), rows, 9)
        world["nb"][name] = (rows, ids, d2)
    return world["nb"][name]


# ---- 1. the pairings ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PAIRINGS)
def test_pairings(world, name):
    from mpassit_amd import regrid as R, target_grid as tg
    rh, src, sloc, dst, dloc, nearest_store = world["pairs"][name]
    rows, ids9, d29 = _neighbours(world, name)
    want_kind = {"m2g": 3, "m2m": 3, "g2m cells": 4, "g2m edges": 4, "g2g e1": 4, "g2g e2": 4, "cons": 0, "pole none": 0}[name]
    assert rh.nnz_per_row == want_kind and 0 < rows.size < rh.n_dst / 2, (name, rh.nnz_per_row, rows.size, rh.n_dst)
    # no tie exemption is needed: the smallest relative gap between neighbouring ranks, the (K+1)-th included
    gap = float(((d29[:, 1:] - d29[:, :-1]) / d29[:, 1:]).min())
    print("%s: %d of %d rows unmapped, n_src %d, smallest relative gap between ranks %.3g" % (name, rows.size, rh.n_dst, rh.n_src, gap))
    assert gap > 1e-9
    mp = {}
    kinds = set()
    for oname, N, e in OPTIONS:
        what = (name, oname, N, e)
        out = R.extrapolate(rh, src, dst, _method(R, oname), N, e, src_loc=sloc, dst_loc=dloc)
        kinds.add((oname, N, out.nnz_per_row))
        _check(R, tg, rh, out, rows, ids9[:, :8], d29[:, :8], oname, N, e, what, lambda ee: mp[ee] if ee in mp else mp.setdefault(ee, _mp_terms(d29[:, :8], ee)))
        again = R.extrapolate(rh, src, dst, _method(R, oname), N, e, src_loc=sloc, dst_loc=dloc)
        if out.nnz_per_row:
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(out.weights(), again.weights())), what
        else:
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(out.csr(), again.csr())), what
        assert out.store_ms > 0.0
        again.release()
        if oname == "stod" and nearest_store is not None:
            near = nearest_store()
            got = out.weights()[0][rows, 0] if out.nnz_per_row else out.csr()[1][out.csr()[0][rows]]
            assert np.array_equal(got, near.weights()[0][rows, 0]), (what, "the library's own nearest Store")
            near.release()
        out.release()
    # the output kind on both sides of N == S
    S = rh.nnz_per_row
    for oname, N, k in kinds:
        assert k == (S if S and (oname == "stod" or N <= S) else 0), (name, oname, N, k)
    # the whole mirror in one call
    rowlen, ids, w = tg.extrapolate_rows(src.xyz(sloc), dst.xyz(dloc), _rows_of(rh)[0], R.EXTRAPMETHOD_NEAREST_IDAVG, 4, 2.0)
    assert np.array_equal(ids, ids9[:, :4]) and (rowlen == 4).all()


# ---- 2. the smallest shapes ---------------------------------------------------------------------------------------------------------------
def _cloud(rng, n, spread=0.2, centre=(38.5, -97.5)):
    """n points around `centre` (degrees) -> (lat, lon) in radians"""
    return np.deg2rad(centre[0] + spread * 50 * rng.uniform(-1, 1, n)), np.deg2rad(centre[1] + spread * 80 * rng.uniform(-1, 1, n))


def _bare_mesh(R, lat, lon):
    """a mesh of cell centres alone: three vertices nobody uses, verticesOnCell empty"""
    n = lat.size
    return R.Mesh(lat, lon, np.zeros(3), np.array([0.0, 0.1, 0.2]), np.zeros((n, 3), np.int32))


def _weights_handle(R, rng, n_src, n_dst, empty):
    """a from_weights handle of n_dst x 1 rows of 1 to 3 random entries, the rows `empty` without any"""
    lens = rng.integers(1, 4, n_dst)
    lens[list(empty)] = 0
    row = np.repeat(np.arange(1, n_dst + 1, dtype=np.int32), lens)
    col = rng.integers(1, n_src + 1, row.size).astype(np.int32)
    return R.RouteHandle.from_weights(n_src, n_dst, 1, row, col, rng.uniform(0.1, 1.0, row.size))


def _small_case(R, tg, src, sloc, dst, dloc, n_src, n_dst, empty, options, seed=0, rh=None):
    rng = np.random.default_rng(seed)
    own = rh is None
    if own:
        rh = _weights_handle(R, rng, n_src, n_dst, empty)
    rows = np.flatnonzero(_rows_of(rh)[0])
    assert np.array_equal(rows, np.array(sorted(empty), np.int64))
    ids8, d28 = tg.extrapolate_neighbours(src.xyz(sloc), dst.xyz(dloc), rows, 8)
    for oname, N, e in options:
        out = R.extrapolate(rh, src, dst, _method(R, oname), N, e, src_loc=sloc, dst_loc=dloc)
        _check(R, tg, rh, out, rows, ids8, d28, oname, N, e, (n_src, n_dst, oname, N, e))
        out.release()
    if own:
        rh.release()
    return ids8, d28


SMALL_OPTIONS = [("stod", 1, 2.0), ("idavg", 1, 2.0), ("idavg", 2, 2.0), ("idavg", 3, 2.0), ("idavg", 4, 2.0), ("idavg", 8, 2.0)]


@pytest.mark.parametrize("n_src", [5, 8, 9, 70, 600])
def test_small_meshes(gpu_lib, n_src):
    """a source set smaller than N (5), one tree leaf exactly (8), one leaf plus one item (9), three levels (70: 9 leaves, 2 nodes, 1) and
    600; n_dst in {1, 63, 64, 65, 257} with row 0 and the last row unmapped; nothing and everything unmapped"""
    from mpassit_amd import regrid as R, target_grid as tg
    rng = np.random.default_rng(n_src)
    src = _bare_mesh(R, *_cloud(rng, n_src))
    for n_dst in (1, 63, 64, 65, 257):
        dst = _bare_mesh(R, *_cloud(rng, n_dst, spread=0.3))
        empty = sorted({0, n_dst - 1, n_dst // 2, n_dst // 3})
        ids8, _ = _small_case(R, tg, src, R.MESHLOC_ELEMENT, dst, R.MESHLOC_ELEMENT, n_src, n_dst, empty, SMALL_OPTIONS, seed=n_dst)
        assert ids8.shape[1] == min(8, n_src)
        if n_dst == 65:
            _small_case(R, tg, src, R.MESHLOC_ELEMENT, dst, R.MESHLOC_ELEMENT, n_src, n_dst, [], SMALL_OPTIONS[:2] + SMALL_OPTIONS[-1:])
            _small_case(R, tg, src, R.MESHLOC_ELEMENT, dst, R.MESHLOC_ELEMENT, n_src, n_dst, range(n_dst), SMALL_OPTIONS)
        dst.destroy()
    src.destroy()


@pytest.mark.parametrize("shape", [(3, 2), (4, 4), (5, 4), (9, 7), (33, 17)])
def test_small_grids(gpu_lib, shape):
    """a stagger of fewer points than N (3 x 2), one 4 x 4 leaf exactly, one leaf plus one column, ragged leaves, five levels (33 x 17);
    sources CENTER, destinations a bare mesh"""
    from mpassit_amd import regrid as R, target_grid as tg
    nx, ny = shape
    rng = np.random.default_rng(nx * ny)
    lon, lat = np.meshgrid(-100.0 + 0.5 * np.arange(nx), 35.0 + 0.4 * np.arange(ny))
    lon, lat = lon + rng.uniform(-0.1, 0.1, lon.shape), lat + rng.uniform(-0.1, 0.1, lat.shape)
    src = R.Grid(lon, lat)
    for n_dst in (1, 65):
        dst = _bare_mesh(R, *_cloud(rng, n_dst, spread=0.2, centre=(38.0, -96.0)))
        empty = sorted({0, n_dst - 1, n_dst // 2})
        ids8, _ = _small_case(R, tg, src, R.STAGGERLOC_CENTER, dst, R.MESHLOC_ELEMENT, nx * ny, n_dst, empty, SMALL_OPTIONS, seed=n_dst)
        assert ids8.shape[1] == min(8, nx * ny)
        dst.destroy()
    src.destroy()


def test_ties_coincidence_and_the_antipode(gpu_lib):
    from mpassit_amd import regrid as R, target_grid as tg
    rng = np.random.default_rng(77)
    lat, lon = _cloud(rng, 40)
    # duplicated cell centres: ids c, c + 40 and c + 80 coincide exactly -- the lowest id wins, at rank K too
    src = _bare_mesh(R, np.tile(lat, 3), np.tile(lon, 3))
    dlat, dlon = _cloud(rng, 66, spread=0.3)
    anti = np.array([-38.5]), np.array([-97.5 + 180.0])                              # a point antipodal to the mesh
    dlat[65], dlon[65] = np.deg2rad(anti[0][0]), np.deg2rad(anti[1][0])
    dst = _bare_mesh(R, dlat, dlon)
    ids8, d28 = _small_case(R, tg, src, R.MESHLOC_ELEMENT, dst, R.MESHLOC_ELEMENT, 120, 66, [0, 7, 30, 65], SMALL_OPTIONS)
    assert (ids8[:, 1] == ids8[:, 0] + 40).all() and (ids8[:, 2] == ids8[:, 0] + 80).all() and (ids8[:, 0] < 40).all() and (ids8[:, 3] < 40).all()
    assert (d28[:, 0] == d28[:, 2]).all() and d28[3, 0] > 3.5, "exact ties, and the antipodal point is nearly a diameter away"
    # a destination mesh that is the source mesh: d2 == 0, one entry of weight 1 on the cell itself
    rh = _weights_handle(R, rng, 120, 120, [0, 50, 119])
    for oname, N, e in (("stod", 1, 2.0), ("idavg", 4, 2.0), ("idavg", 8, 1.0)):
        out = R.extrapolate(rh, src, src, _method(R, oname), N, e)
        rowptr, col, val = out.csr()
        for i, c in ((0, 0), (50, 10), (119, 39)):
            assert rowptr[i + 1] - rowptr[i] == 1 and col[rowptr[i]] == c and val[rowptr[i]] == 1.0, (oname, i, col[rowptr[i]:rowptr[i + 1]])
        out.release()
    rh.release()
    src.destroy()
    dst.destroy()


# ---- 3. consumers -------------------------------------------------------------------------------------------------------------------------
def _held(got, want, what):
    import torch
    w = torch.from_numpy(np.ascontiguousarray(want)).cuda()
    g = got.contiguous().reshape(w.shape)
    assert g.dtype == w.dtype, (what, g.dtype, w.dtype)
    it = torch.int64 if g.dtype == torch.float64 else torch.int32
    bad = g.view(it) != w.view(it)
    assert not bool(bad.any()), (what, int(bad.sum()), bad.numel())


def _filled(world, name, oname):
    from mpassit_amd import regrid as R
    key = (name, oname)
    if key not in world["filled"]:
        rh, src, sloc, dst, dloc, _ = world["pairs"][name]
        world["filled"][key] = R.extrapolate(rh, src, dst, _method(R, oname), 8, 2.0, src_loc=sloc, dst_loc=dloc)
    return world["filled"][key]


@pytest.mark.parametrize("oname", ["stod", "idavg"])
def test_consumers(world, gpu_lib, oname):
    """The STOD-filled Mesh -> Grid handle (fixed, 3 slots) and its IDAVG N = 8 twin (CSR) under every consumer: the bits of the contract's
    host restatement on the handle's exported pattern; at mapped points the bits of the unextrapolated handle; at STOD points the nearest
    cell's value."""
    import torch
    from mpassit_amd import regrid as R, target_grid as tg
    plain = world["pairs"]["m2g"][0]
    rh = _filled(world, "m2g", oname)
    assert rh.nnz_per_row == (3 if oname == "stod" else 0)
    pat = cr.Pattern.of(rh)
    rows = _neighbours(world, "m2g")[0]
    mapped = np.ones(rh.n_dst, bool)
    mapped[rows] = False
    assert not pat.unmapped.any()
    nlev, nf = 9, 2
    x64 = cr.ordinary(rh.n_src, nlev, nf, 5)
    F64, F32 = np.float64, np.float32
    try:
        for sdt in (F64, F32):
            x = cr.to_f32(x64) if sdt == F32 else x64
            cf = torch.from_numpy(x).cuda()
            lf = cf.transpose(1, 2).contiguous()
            for ddt in (F64, F32):
                tdt = torch.float32 if ddt == F32 else torch.float64
                want = cr.apply(pat, x, nlev, nf, dst_dtype=ddt)
                base = plain.regrid_typed(cf.view(-1), nlev=nlev, nfields=nf, out_dtype=tdt).reshape(nf, nlev, -1).cpu().numpy()
                assert np.array_equal(_raw(want[:, :, mapped]), _raw(base[:, :, mapped])), "mapped points: the unextrapolated bits"
                assert (base[:, :, rows] == 0).all() and np.abs(want[:, :, rows]).min() > 1.0
                if oname == "stod":
                    near = x[:, :, pat.idx[rows, 0]].astype(ddt)
                    assert np.array_equal(_raw(want[:, :, rows]), _raw(near)), "STOD points: the nearest cell's value"
                for a3 in (A3 if oname == "stod" else (-1,)):
                    gpu_lib.tune("a3_staged", a3)
                    for lfv in (LFV if oname == "stod" else (-1,)):
                        gpu_lib.tune("lf_variant", lfv)
                        for layout, s in ((R.LAYOUT_CELL_FAST, cf), (R.LAYOUT_LEV_FAST, lf)):
                            _held(rh.regrid_typed(s.view(-1), nlev=nlev, nfields=nf, layout=layout, out_dtype=tdt), want, ("typed", oname, sdt, ddt, a3, lfv, layout))
                gpu_lib.tune("a3_staged", -1)
                gpu_lib.tune("lf_variant", -1)
                wm = cr.apply_masked(pat, x, nlev, nf, dst_dtype=ddt, flags=1)
                _held(rh.regrid_masked(cf.view(-1), nlev=nlev, nfields=nf, out_dtype=tdt), wm, ("masked", oname, sdt, ddt))
            if sdt == F64:
                _held(rh.regrid(cf.view(-1), nlev=nlev, nfields=nf), cr.apply(pat, x, nlev, nf, epilogue=False), ("regrid", oname))
            g = cr.to_f32(cr.ordinary(rh.n_dst, nlev, nf, 9)) if sdt == F32 else cr.ordinary(rh.n_dst, nlev, nf, 9)
            want64, cap = cr.transpose(pat, g, nlev, nf)
            assert not cap.any()
            for ddt in (F64, F32):
                got = rh.regrid_transpose(torch.from_numpy(g).cuda(), nlev=nlev, nfields=nf, out_dtype=torch.float32 if ddt == F32 else torch.float64)
                _held(got, want64.astype(ddt), ("transpose", oname, sdt, ddt))
    finally:
        gpu_lib.tune("a3_staged", -1)
        gpu_lib.tune("lf_variant", -1)
    # compose with a second handle: CENTER -> EDGE1 after the filled Mesh -> Grid handle
    e1 = world["pairs"]["g2g e1"][0]
    c = R.compose(e1, rh)
    ca, cb = _rows_of(e1)[1:], _rows_of(rh)[1:]
    wr, wc, wv = tg.compose_csr(ca[0], ca[1], ca[2], cb[0], cb[1], cb[2])
    got = c.csr()
    assert np.array_equal(got[0], wr) and np.array_equal(got[1], wc) and np.array_equal(_bits(got[2]), _bits(wv[0]))
    c.release()
    # to_esmf_weights survives a round trip through from_weights
    row, col, S = rh.to_esmf_weights()
    twin = R.RouteHandle.from_weights(rh.n_src, rh.nx_dst, rh.ny_dst, row, col, S)
    tr, tc, tv = _rows_of(twin)[1:]              # (rows of one length come back as a fixed handle)
    fr, fc, fv = _rows_of(rh)[1:]
    assert np.array_equal(tr, fr) and np.array_equal(tc, fc) and np.array_equal(_bits(tv), _bits(fv))
    xs = torch.from_numpy(x64[0, :1].copy()).cuda()
    _held(twin.regrid_typed(xs.view(-1)), rh.regrid_typed(xs.view(-1)).cpu().numpy(), "the round trip regrids alike")
    twin.release()


# ---- 4. the wind chain --------------------------------------------------------------------------------------------------------------------
def test_wind_chain(world):
    """STOD-filled CENTER -> EDGE1 / EDGE2 handles on the 60 x 40 grid: the fused chain is the rotation plus two Regrids bit for bit and
    the contract's restatement; U's first column is the rotated mass wind of column 0; the adjoint is two transposes plus the rotation's."""
    import torch
    from mpassit_amd import regrid as R
    g = world["g"]
    nx, ny = g.nx, g.ny
    h1, h2 = _filled(world, "g2g e1", "stod"), _filled(world, "g2g e2", "stod")
    assert h1.nnz_per_row == 4 and h2.nnz_per_row == 4 and (h1.nx_dst, h1.ny_dst, h2.nx_dst, h2.ny_dst) == (nx + 1, ny, nx, ny + 1)
    p1, p2 = cr.Pattern.of(h1), cr.Pattern.of(h2)
    assert not p1.unmapped.any() and not p2.unmapped.any()
    ca, sa = (np.ascontiguousarray(a, np.float64).reshape(-1) for a in (g.cosa, g.sina))
    cat, sat = torch.from_numpy(ca).cuda(), torch.from_numpy(sa).cuda()
    for nlev in (1, 5):
        um, vm, _ = cr.mass_winds(nx, ny, nlev, "ordinary")
        umt, vmt = torch.from_numpy(um).cuda(), torch.from_numpy(vm).cuda()
        ur, vr = R.rotate_winds_cgrid(cat, sat, umt.clone(), vmt.clone())
        for dt, dst_type in ((torch.float64, 0), (torch.float32, 1)):
            U, V, ur2, vr2 = R.wind_destagger(h1, h2, cat, sat, umt, vmt, nlev, out_dtype=dt, keep_mass=True)
            wU, wV, wur, wvr = cr.wind_destagger(p1, p2, ca, sa, um, vm, nlev, dst_type, 0, True)
            _held(U, wU, ("U", nlev, dst_type))
            _held(V, wV, ("V", nlev, dst_type))
            _held(ur2, wur, "umass'")
            _held(vr2, wvr, "vmass'")
            assert torch.equal(ur2.view(torch.int64), ur.view(torch.int64))
            if dst_type == 0:      # the float64 entry stores the sum as it stands, as regrid() does
                two = (h1.regrid(ur.view(-1), nlev=nlev), h2.regrid(vr.view(-1), nlev=nlev))
            else:
                two = (h1.regrid_typed(ur.view(-1), nlev=nlev, out_dtype=dt), h2.regrid_typed(vr.view(-1), nlev=nlev, out_dtype=dt))
            it = torch.int64 if dt == torch.float64 else torch.int32
            assert torch.equal(U.reshape(-1).view(it), two[0].reshape(-1).view(it)) and torch.equal(V.reshape(-1).view(it), two[1].reshape(-1).view(it))
            col0 = ur.reshape(nlev, ny, nx)[:, :, 0].to(dt)
            assert torch.equal(U.reshape(nlev, ny, nx + 1)[:, :, 0].contiguous().view(it), col0.contiguous().view(it)), "U's first column"
            assert bool((U.reshape(nlev, ny, nx + 1)[:, :, [0, nx]] != 0).all()) and bool((V.reshape(nlev, ny + 1, nx)[:, [0, ny], :] != 0).all())
        gU = torch.from_numpy(cr.ordinary(h1.n_dst, nlev, 1, 3)[0]).cuda()
        gV = torch.from_numpy(cr.ordinary(h2.n_dst, nlev, 1, 4)[0]).cuda()
        gum, gvm = R.wind_destagger_transpose(h1, h2, cat, sat, gU.reshape(nlev, ny, nx + 1), gV.reshape(nlev, ny + 1, nx), nlev)
        a = h1.regrid_transpose(gU, nlev=nlev, out_dtype=torch.float64).reshape(nlev, ny, nx).contiguous()
        b = h2.regrid_transpose(gV, nlev=nlev, out_dtype=torch.float64).reshape(nlev, ny, nx).contiguous()
        R.rotate_winds_cgrid_transpose(cat.reshape(ny, nx), sat.reshape(ny, nx), a, b)
        assert torch.equal(gum.reshape(-1).view(torch.int64), a.reshape(-1).view(torch.int64))
        assert torch.equal(gvm.reshape(-1).view(torch.int64), b.reshape(-1).view(torch.int64))


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(world, gpu_lib):
    from mpassit_amd import _lib as L, regrid as R, synth, target_grid as tg
    lib = L.load()
    o = world["obj"]
    m2g = world["pairs"]["m2g"][0]
    who = "mpg_handle_extrapolate"
    h = C.c_void_p()

    def pts(obj, loc=0):
        return R._points(obj, loc, "x")

    def call(rh=m2g, src=None, dst=None, method=1, N=8, e=2.0, out=h, raw_src=None, raw_dst=None):
        ps = raw_src if raw_src is not None else pts(o["mesh_in"]) if src is None else src
        pd = raw_dst if raw_dst is not None else pts(o["grid"]) if dst is None else dst
        opts = L.ExtrapOpts(method=method, num_src_pnts=N, dist_exponent=e)
        return L.handle_extrapolate(rh._h if rh is not None else None, C.byref(ps), C.byref(pd), C.byref(opts), C.byref(out) if out is not None else None)

    def refused(rc, want, *words):
        msg = lib.mpg_last_error().decode()
        assert rc == want and who in msg, (rc, want, msg)
        for word in words:
            assert word in msg, msg

    INV, UNS = L.MPG_ERR_INVALID_ARG, L.MPG_ERR_UNSUPPORTED
    assert call() == 0
    L.check(lib.mpg_handle_release(h))
    h = C.c_void_p()
    refused(call(rh=None), INV, "NULL")
    refused(call(out=None), INV, "NULL")
    opts = L.ExtrapOpts(method=1, num_src_pnts=8, dist_exponent=2.0)
    ps, pd = pts(o["mesh_in"]), pts(o["grid"])
    refused(L.handle_extrapolate(m2g._h, None, C.byref(pd), C.byref(opts), C.byref(h)), INV, "NULL")
    refused(L.handle_extrapolate(m2g._h, C.byref(ps), None, C.byref(opts), C.byref(h)), INV, "NULL")
    refused(L.handle_extrapolate(m2g._h, C.byref(ps), C.byref(pd), None, C.byref(h)), INV, "NULL")
    both = L.Points(mesh=o["mesh_in"]._h, meshloc=0, grid=o["grid"]._h, staggerloc=0)
    neither = L.Points(mesh=None, meshloc=0, grid=None, staggerloc=0)
    refused(call(raw_src=both), INV, "exactly one", "both")
    refused(call(raw_dst=neither), INV, "exactly one", "neither")
    refused(call(method=0), INV, "method")
    refused(call(method=3), INV, "method")
    refused(call(method=2, N=0), INV, "num_src_pnts = 0", "1..8")
    refused(call(method=2, N=9), INV, "num_src_pnts = 9", "1..8")
    for bad in (float("nan"), float("inf"), 0.0, -1.0):
        refused(call(method=2, e=bad), INV, "dist_exponent")
    assert call(method=1, N=0, e=-1.0) == 0, "N and e are ignored for STOD"
    L.check(lib.mpg_handle_release(h))
    h = C.c_void_p()
    refused(call(src=pts(o["mesh_over"])), INV, "n_src = 5084", "6030")
    node = R.regrid_store(o["mesh_in"], o["grid"], R.REGRIDMETHOD_BILINEAR, meshloc=R.MESHLOC_NODE)
    refused(call(rh=node), INV, "n_src = %d" % node.n_src, "5084", "node-located")
    refused(call(dst=pts(o["grid"], R.STAGGERLOC_EDGE1)), INV, "n_dst = 2400", "2440", "60 x 40", "61 x 40")
    refused(call(src=pts(o["mesh_in"], R.MESHLOC_NODE)), INV, "MPG_MESHLOC_ELEMENT")
    refused(call(dst=pts(o["mesh_in"], R.MESHLOC_EDGE)), INV, "no edges", "mpg_mesh_set_edges")
    bare = R.Grid(np.array([[0.0, 1.0]]), np.array([[0.0, 0.0]]))
    refused(call(dst=pts(bare, R.STAGGERLOC_EDGE1)), INV, "no coordinates")
    bare.destroy()
    # pole terms, a localized handle, a source window
    pole = R.regrid_store_grid(o["per"], R.STAGGERLOC_EDGE2)
    assert pole.pole()[0].size > 0
    refused(call(rh=pole, src=pts(o["per"]), dst=pts(o["per"], R.STAGGERLOC_EDGE2)), UNS, "mpg_handle_pole_count > 0", "MPG_POLEMETHOD_NONE")
    idx, w = m2g.weights()
    rowptr, col, val = tg.fixed_to_csr(idx, w)
    loc = R.RouteHandle.from_weights(m2g.n_src, m2g.nx_dst, m2g.ny_dst, np.repeat(np.arange(1, m2g.n_dst + 1, dtype=np.int32), np.diff(rowptr)),
                                     (col + 1).astype(np.int32), val)
    loc.localize()
    refused(call(rh=loc), UNS, "localized or rebased")
    g2 = tg.define_target_grid_params("lambert", 41, 31, dx=30000.0, dy=30000.0, **LAMBERT)      # a mesh larger than its grid: the handle references
    m2 = R.Mesh.from_mpas(synth.regional_mesh_for_lambert(g2.proj, 41, 31, 3001, margin=0.3, seed=3))   # a proper part of the cells
    grid2 = R.Grid.from_target(g2)
    win = R.regrid_store(m2, grid2, R.REGRIDMETHOD_BILINEAR)
    first, end = win.source_range()
    assert 0 < first < end <= m2.nCells
    assert call(rh=win, src=pts(m2), dst=pts(grid2)) == 0, "the same call without a window"
    L.check(lib.mpg_handle_release(h))
    h = C.c_void_p()
    m2.set_source_window(first, end - first)
    refused(call(rh=win, src=pts(m2), dst=pts(grid2)), UNS, "source window", "mpg_mesh_set_source_window")
    m2.set_source_window(0, m2.nCells)
    assert h.value is None, "a refused call leaves *out alone"
    # the wrapper's own check, and the library still works afterwards
    with pytest.raises(ValueError):
        R.extrapolate(m2g, "mesh", o["grid"])
    again = R.extrapolate(m2g, o["mesh_in"], o["grid"])
    assert again.nnz_per_row == 3 and again.store_stats[1] == _neighbours(world, "m2g")[0].size
    for x in (again, node, pole, loc, win):
        x.release()
    m2.destroy()
    grid2.destroy()
