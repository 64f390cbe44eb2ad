"""Store-time masks on the GPU at small sizes: mpg_handle_mask against the numpy mirror target_grid.mask_rows byte for byte (the ROW rule on
fixed handles of 3, 1 and 4 slots and on the periodic CSR handle with its cap rows; the ENTRY rule under both norms on the three
conservative Stores), mpg_handle_extrapolate_masked against target_grid.extrapolate_rows_masked fed with the library's own unit vectors
(columns exactly; values bit for bit for nearest-source-to-destination and e == 2.0, within the bound tests/test_extrapolate_gpu.py derives
for e == 3.5), the ESMF-shaped composition store_masks, the consumers on masked handles, and the refusals.

Shapes: a regional mesh of 2.5 k cells under a 37 x 23 Lambert grid definition (36 x 22 mass points: ragged 4 x 4 leaf blocks, 792 rows =
three full 256-thread blocks and a part), a 600-cell global Voronoi mesh with a 24 x 12 periodic grid, a second regional mesh for Mesh -> Mesh.  Every case asserts from the
mirror that it holds a row of each class it claims to cover, so that none passes vacuously."""
import ctypes as C

import numpy as np
import pytest

import _contract_ref as cr
from conftest import LAMBERT

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
B_DEVICE_POW = 2                 # the ulp bound of the device pow that tests/test_extrapolate_gpu.py measured and uses
A3 = (-1, -2, 0, 1, 2)           # the "a3_staged" and "lf_variant" settings of tests/test_contract_gpu.py
LFV = (-1, 0, 1, 2)


def _mp_terms(d2k, e):
    """1 / d^e = d2^(-e / 2) of every neighbour at 50 digits (None for a row whose nearest point coincides), as tests/test_extrapolate_gpu.py"""
    import mpmath
    mpmath.mp.dps = 50
    return [None if row[0] == 0.0 else [mpmath.mpf(1) / mpmath.power(mpmath.mpf(float(x)), mpmath.mpf(e) / 2) for x in row] for row in d2k]


def _within_bound(w, terms, K, e, what):
    """w [n][>= K] against (1 / d^e) / sum over the K nearest of (1 / d^e), relative, within (2 B + 0.5 e + 0.5 K) eps: the bound
    tests/test_extrapolate_ref.py derives and tests/test_extrapolate_gpu.py uses"""
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


def _raw(a):
    return np.ascontiguousarray(a).tobytes()


def _export(rh):
    """what a handle exports, as bytes: kind, pattern, values, dst_frac where it has one"""
    from mpassit_amd import _lib as L
    out = {"kind": rh.nnz_per_row, "shape": (rh.n_src, rh.n_dst, rh.nx_dst, rh.ny_dst)}
    if rh.nnz_per_row:
        idx, w = rh.weights()
        out.update(idx=_raw(idx), w=_raw(w))
    else:
        rowptr, col, val = rh.csr()
        out.update(rowptr=_raw(rowptr), col=_raw(col), val=_raw(val), nnz=rh.nnz)
    try:
        out["frac"] = _raw(rh.dst_frac())
    except L.MpgError:
        out["frac"] = None
    return out


def _frac_or_none(rh):
    from mpassit_amd import _lib as L
    try:
        return rh.dst_frac()
    except L.MpgError:
        return None


def _mirror(tg, rh, sm, dm, rule, norm):
    """the expected export of mask_handle(rh, sm, dm, rule, norm) from target_grid.mask_rows, and the row classes of the case"""
    frac = _frac_or_none(rh)
    if rh.nnz_per_row:
        idx, w = rh.weights()
        rowptr, col, val = tg.fixed_to_csr(idx, w)
    else:
        rowptr, col, val = rh.csr()
    rp, c, v, f, stats = tg.mask_rows(rowptr, col, val, frac, sm, dm, rule, norm)
    had, now = np.diff(rowptr), np.diff(rp)
    dmb = np.zeros(rh.n_dst, bool) if dm is None else np.asarray(dm) != 0
    classes = {"untouched": int(((now == had) & (had > 0)).sum()), "by source": int(((had > 0) & (now == 0) & ~dmb).sum()),
               "by destination": int(((had > 0) & dmb).sum()), "partly": int(((now > 0) & (now < had)).sum())}
    want = {"kind": rh.nnz_per_row, "shape": (rh.n_src, rh.n_dst, rh.nx_dst, rh.ny_dst), "frac": None if f is None else _raw(f)}
    if rh.nnz_per_row:
        gone = (had > 0) & (now == 0)
        idx, w = idx.copy(), w.copy()
        idx[gone], w[gone] = -1, 0.0                       # as the Stores write an unmapped row: every index -1, every weight +0.0
        want.update(idx=_raw(idx), w=_raw(w))
    else:
        want.update(rowptr=_raw(rp), col=_raw(c), val=_raw(v), nnz=int(rp[-1]))
    return want, stats, classes, gone if rh.nnz_per_row else (had > 0) & (now == 0)


@pytest.fixture(scope="module")
def world(gpu_lib):
    from mpassit_amd import regrid as R, synth, target_grid as tg
    g = tg.define_target_grid_params("lambert", 37, 23, dx=30000.0, dy=30000.0, **LAMBERT)
    m_in = synth.regional_mesh_for_lambert(g.proj, 37, 23, 2500, margin=-0.08, seed=12)
    m_over = synth.regional_mesh_for_lambert(g.proj, 37, 23, 2900, margin=0.05, seed=11)
    gp = tg.define_target_grid_params("lat-lon", nx=24, ny=12, stand_lon=0.0, is_regional=False)
    vor = synth.global_voronoi_mesh(600)
    o = dict(grid=R.Grid.from_target(g), mesh_in=R.Mesh.from_mpas(m_in), mesh_over=R.Mesh.from_mpas(m_over), per=R.Grid.from_target(gp),
             vor=R.Mesh.from_mpas(vor))
    E, C_, E1 = R.MESHLOC_ELEMENT, R.STAGGERLOC_CENTER, R.STAGGERLOC_EDGE1
    BIL, NEAR, CONS = R.REGRIDMETHOD_BILINEAR, R.REGRIDMETHOD_NEAREST_STOD, R.REGRIDMETHOD_CONSERVE
    # name -> (handle, src, src_loc, dst, dst_loc)
    pairs = {
        "m2g bil": (R.regrid_store(o["mesh_in"], o["grid"], BIL), o["mesh_in"], E, o["grid"], C_),
        "m2g near": (R.regrid_store(o["mesh_in"], o["grid"], NEAR), o["mesh_in"], E, o["grid"], C_),
        "g2m bil": (R.regrid_store_to_mesh(o["grid"], o["mesh_over"], BIL), o["grid"], C_, o["mesh_over"], E),
        "g2g e1": (R.regrid_store_grid(o["grid"], E1), o["grid"], C_, o["grid"], E1),
        "p2m csr": (R.regrid_store_periodic_to_mesh(o["per"], o["vor"]), o["per"], C_, o["vor"], E),
        "cons m2g": (R.regrid_store(o["mesh_in"], o["grid"], CONS), o["mesh_in"], E, o["grid"], C_),
        "cons g2m": (R.regrid_store_conserve_to_mesh(o["grid"], o["mesh_over"], R.NORM_DSTAREA), o["grid"], C_, o["mesh_over"], E),
        "cons g2m frac": (R.regrid_store_conserve_to_mesh(o["grid"], o["mesh_over"], R.NORM_FRACAREA), o["grid"], C_, o["mesh_over"], E),
        "cons m2m": (R.regrid_store_conserve_mesh(o["mesh_in"], o["mesh_over"], R.NORM_DSTAREA), o["mesh_in"], E, o["mesh_over"], E),
        "cons m2m frac": (R.regrid_store_conserve_mesh(o["mesh_in"], o["mesh_over"], R.NORM_FRACAREA), o["mesh_in"], E, o["mesh_over"], E),
    }
    print("cells", m_in.nCells, m_over.nCells, vor.nCells)
    d = dict(g=g, obj=o, pairs=pairs, xyz={}, masks={})
    yield d
    for p in pairs.values():
        p[0].release()
    for x in o.values():
        x.destroy()


def _xyz(world, obj, loc):
    key = (id(obj), loc)
    if key not in world["xyz"]:
        world["xyz"][key] = obj.xyz(loc)
    return world["xyz"][key]


def _src_masks(world, name):
    """name -> source mask (bool [n_src]) of a pairing: a random 30 %, a coherent ocean (every source on one side of a plane), a compact
    cluster (whole BVH leaves of a mesh; one aligned 4 x 4 block of a grid), all but three, all, none"""
    key = ("src", name)
    if key in world["masks"]:
        return world["masks"][key]
    rh, src, sloc, dst, dloc = world["pairs"][name]
    xyz = _xyz(world, src, sloc)
    n = rh.n_src
    rng = np.random.default_rng(len(name) * 1000 + n)
    centre = xyz.mean(axis=1)
    axis = np.cross(centre, [0.0, 0.0, 1.0])
    axis /= np.linalg.norm(axis)
    side = xyz.T @ axis
    ocean = side > np.quantile(side, 0.6)                              # 40 % of the sources, one coherent region
    if hasattr(src, "nCells"):
        d2 = ((xyz - xyz[:, [n // 3]]) ** 2).sum(axis=0)
        cluster = np.zeros(n, bool)
        cluster[np.argsort(d2, kind="stable")[:64]] = True            # the 64 cells nearest to one cell: several whole leaves of 8 sorted sites
    else:
        ny, nx = src.stagger_shape(sloc)
        cluster = np.zeros((ny, nx), bool)
        cluster[4:8, 8:12] = True                                     # leaf block (bi, bj) = (2, 1) of the point pyramid
        cluster = cluster.reshape(-1)
    three = np.ones(n, bool)
    three[rng.choice(n, 3, replace=False)] = False
    out = {"random": rng.random(n) < 0.3, "ocean": ocean, "cluster": cluster, "all but three": three, "all": np.ones(n, bool), "none": np.zeros(n, bool)}
    world["masks"][key] = out
    return out


def _dst_mask(rh, seed=5):
    return np.random.default_rng(seed + rh.n_dst).random(rh.n_dst) < 0.15


# ---- 1. mask_handle against mask_rows ---------------------------------------------------------------------------------------------------------
ROW_PAIRS = {"m2g bil": 3, "m2g near": 1, "g2m bil": 4, "g2g e1": 4, "p2m csr": 0}


@pytest.mark.parametrize("name", sorted(ROW_PAIRS))
def test_row_rule(world, name):
    from mpassit_amd import regrid as R, target_grid as tg
    rh, src, sloc, dst, dloc = world["pairs"][name]
    assert rh.nnz_per_row == ROW_PAIRS[name]
    base = _export(rh)
    if name == "p2m csr":
        assert int(np.diff(rh.csr()[0]).max()) == src.nx > 4, "cap rows of nx entries"
    masks = _src_masks(world, name)
    dm = _dst_mask(rh)
    seen_cap = False
    for mname, sm in masks.items():
        for use_dm in (False, True):
            for rule in (R.MASKRULE_AUTO, R.MASKRULE_ROW):
                if rule == R.MASKRULE_ROW and (use_dm or mname not in ("random", "none")):
                    continue                                        # (the explicit rule once per kind of mask: AUTO resolves to it)
                want, stats, classes, gone = _mirror(tg, rh, sm, dm if use_dm else None, tg.MASKRULE_ROW, 0)
                if mname in ("random", "ocean", "cluster"):
                    assert classes["untouched"] > 0 and classes["by source"] > 0 and (classes["by destination"] > 0) == use_dm, (name, mname, classes)
                if mname == "all":
                    assert classes["untouched"] == 0
                out = R.mask_handle(rh, sm, dm if use_dm else None, rule)
                got = _export(out)
                assert got == want, (name, mname, use_dm, [k for k in want if got[k] != want[k]])
                assert out.store_stats[1:4] == stats and out.store_ms > 0.0, (name, mname, out.store_stats[:4], stats)
                if name == "p2m csr" and mname == "random":
                    rowptr = rh.csr()[0]
                    cap = np.diff(rowptr) == src.nx
                    seen_cap = bool((gone & cap).any())
                    assert seen_cap, "a cap row is a row like any other: one masked point of the end row unmaps it"
                if rh.nnz_per_row and gone.any():
                    idx, w = out.weights()
                    assert (idx[gone] == -1).all() and (w[gone] == 0.0).all() and not np.signbit(w[gone]).any()
                out.release()
    # no masks at all, and zero masks: the input's bytes; masks may be numpy bool / uint8 or torch, on the host or the device
    import torch
    n_src, n_dst = rh.n_src, rh.n_dst
    for sm, dmk in ((None, None), (np.zeros(n_src, np.uint8), np.zeros(n_dst, bool)), (torch.zeros(n_src, dtype=torch.bool, device="cuda"), torch.zeros(n_dst, dtype=torch.uint8))):
        out = R.mask_handle(rh, sm, dmk)
        assert _export(out) == base and out.store_stats[1:4] == [0, 0, 0]
        out.release()
    a = R.mask_handle(rh, masks["random"], dm)
    b = R.mask_handle(rh, torch.from_numpy(masks["random"]).cuda(), torch.from_numpy(dm.astype(np.uint8)).cuda())
    assert _export(a) == _export(b), "two runs, host and device masks: the same bytes"
    a.release()
    b.release()


ENTRY_PAIRS = ("cons m2g", "cons g2m", "cons g2m frac", "cons m2m", "cons m2m frac")


@pytest.mark.parametrize("name", ENTRY_PAIRS)
def test_entry_rule(world, name):
    from mpassit_amd import regrid as R, target_grid as tg
    rh, src, sloc, dst, dloc = world["pairs"][name]
    assert rh.nnz_per_row == 0
    has_frac = _frac_or_none(rh) is not None
    assert has_frac == (name != "cons m2g")
    base = _export(rh)
    masks = _src_masks(world, name)
    dm = _dst_mask(rh)
    norms = (R.NORM_FRACAREA,) if name.endswith("frac") else (R.NORM_DSTAREA, R.NORM_FRACAREA) if name == "cons m2g" else (R.NORM_DSTAREA,)
    for norm in norms:
        for mname, sm in masks.items():
            for use_dm in ((False, True) if mname in ("random", "none") else (False,)):
                want, stats, classes, gone = _mirror(tg, rh, sm, dm if use_dm else None, tg.MASKRULE_ENTRY, norm)
                if mname in ("random", "ocean", "cluster"):
                    # a row with some and a row with all of its entries removed, and an untouched one
                    assert classes["untouched"] > 0 and classes["partly"] > 0 and classes["by source"] > 0, (name, mname, classes)
                out = R.mask_handle(rh, sm, dm if use_dm else None, R.MASKRULE_AUTO, norm)
                got = _export(out)
                assert got == want, (name, mname, norm, use_dm, [k for k in want if got[k] != want[k]])
                assert out.store_stats[1:4] == stats, (name, mname, out.store_stats[:4], stats)
                out.release()
        out = R.mask_handle(rh, None, None, R.MASKRULE_ENTRY, norm)
        assert _export(out) == base
        out.release()
    # the ROW rule is defined for a conservative handle too (an explicit rule)
    want, stats, classes, _ = _mirror(tg, rh, masks["cluster"], None, tg.MASKRULE_ROW, 0)
    out = R.mask_handle(rh, masks["cluster"], None, R.MASKRULE_ROW)
    assert _export(out) == want and out.store_stats[1:4] == stats and classes["by source"] > 0
    out.release()


# ---- 2. extrapolate_masked against extrapolate_rows_masked -------------------------------------------------------------------------------------
def _unmapped(rh):
    if rh.nnz_per_row:
        return rh.weights()[0][:, 0] < 0
    return np.diff(rh.csr()[0]) == 0


def _expected_fill(tg, rh, rows, rowlen, ids, w, fixed):
    """the export of a handle whose rows `rows` are (ids, w) of length rowlen, every other row as rh's"""
    if fixed:
        idx, wt = rh.weights()
        idx, wt = idx.copy(), wt.copy()
        for u, i in enumerate(rows):
            k = rowlen[u]
            if k == 0:
                continue
            idx[i, :k], wt[i, :k] = ids[u, :k], w[u, :k]
            idx[i, k:], wt[i, k:] = ids[u, 0], 0.0
        if rh.nnz_per_row == 1:
            wt = (idx >= 0).astype(np.float64)
        return idx, wt
    if rh.nnz_per_row:
        rowptr, col, val = tg.fixed_to_csr(*rh.weights())
    else:
        rowptr, col, val = rh.csr()
    lens = np.diff(rowptr).astype(np.int64)
    lens[rows] = rowlen
    out_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    out_col, out_val = np.empty(out_ptr[-1], np.int32), np.empty(out_ptr[-1])
    fill = dict(zip(rows.tolist(), range(rows.size)))
    for i in range(rh.n_dst):
        a, b = out_ptr[i], out_ptr[i + 1]
        if i in fill:
            u = fill[i]
            out_col[a:b], out_val[a:b] = ids[u, :rowlen[u]], w[u, :rowlen[u]]
        else:
            out_col[a:b], out_val[a:b] = col[rowptr[i]:rowptr[i + 1]], val[rowptr[i]:rowptr[i + 1]]
    return out_ptr, out_col, out_val


OPTIONS = [("stod", 1, 2.0), ("idavg", 1, 2.0), ("idavg", 3, 2.0), ("idavg", 4, 2.0), ("idavg", 8, 2.0), ("idavg", 4, 3.5), ("idavg", 8, 3.5)]


@pytest.mark.parametrize("name", ["m2g bil", "m2g near", "g2m bil", "cons m2g"])
def test_extrapolate_masked(world, name):
    """mesh sources (site BVH) and grid sources (point pyramid); fixed handles of 3, 1 and 4 slots and a CSR handle"""
    from mpassit_amd import regrid as R, target_grid as tg
    rh, src, sloc, dst, dloc = world["pairs"][name]
    sx, dx = _xyz(world, src, sloc), _xyz(world, dst, dloc)
    masks = _src_masks(world, name)
    own = None
    if name == "m2g near":       # a nearest Store maps every point: the rows under the ocean are unmapped first, as store_masks does
        rh = own = R.mask_handle(rh, masks["ocean"], None)
        assert rh.nnz_per_row == 1
    un = _unmapped(rh)
    assert 0 < un.sum() < rh.n_dst
    skip = np.random.default_rng(3).random(rh.n_dst) < 0.3
    assert (un & skip).any() and (un & ~skip).any(), "unmapped rows on both sides of dst_skip"
    for mname, sm in masks.items():
        live = int((~sm).sum())
        for use_skip in ((False, True) if mname in ("ocean", "none") else (False,)):
            rows = np.flatnonzero(un & ~skip) if use_skip else np.flatnonzero(un)
            ids8, d28 = None, None
            mp = {}
            for oname, N, e in (OPTIONS if mname in ("random", "ocean", "cluster") else OPTIONS[:1] + OPTIONS[4:5]):
                method = R.EXTRAPMETHOD_NEAREST_STOD if oname == "stod" else R.EXTRAPMETHOD_NEAREST_IDAVG
                what = (name, mname, use_skip, oname, N, e)
                rowlen, ids, w = tg.extrapolate_rows_masked(sx, dx, rows, sm, method, N, e)
                K = min(N if oname == "idavg" else 1, live)
                assert ids.shape[1] == K
                if mname == "all but three" and N == 8:
                    assert K == 3 and (rowlen == 3).all(), "rows of three"
                if K:
                    assert not sm[ids[ids >= 0]].any()
                out = R.extrapolate_masked(rh, src, dst, sm, skip if use_skip else None, method, N, e, src_loc=sloc, dst_loc=dloc)
                stats = out.store_stats
                assert stats[1:4] == [rows.size if K else 0, K, live], (what, stats[:4])
                fixed = rh.nnz_per_row > 0 and (oname == "stod" or N <= rh.nnz_per_row)
                assert out.nnz_per_row == (rh.nnz_per_row if fixed else 0), what
                exact = oname == "stod" or e == 2.0
                want = _expected_fill(tg, rh, rows, rowlen, ids, w, fixed)
                got = out.weights() if fixed else out.csr()
                assert np.array_equal(got[0], want[0]), (what, "pattern")
                if not fixed:
                    assert np.array_equal(got[1], want[1]), (what, "columns")
                if exact:
                    assert _raw(got[-1]) == _raw(want[-1]), (what, "values, bit for bit")
                else:
                    # the bound of tests/test_extrapolate_gpu.py: (2 B + 0.5 e + 0.5 K) eps against a 50-digit evaluation of the mirror's distances
                    d2k = np.zeros((rows.size, K))
                    for u, p in enumerate(rows):
                        d = dx[:, [p]] - sx[:, ids[u]]
                        d2k[u] = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                    gw = np.zeros((rows.size, K))
                    for u, i in enumerate(rows):
                        gw[u, :rowlen[u]] = got[1][i, :rowlen[u]] if fixed else got[2][got[0][i]:got[0][i + 1]]
                    _within_bound(gw, _mp_terms(d2k, e), K, e, what)
                    keep = np.ones(rh.n_dst, bool)
                    keep[rows] = False
                    if fixed:
                        assert _raw(got[1][keep]) == _raw(want[1][keep]), (what, "untouched rows")
                if use_skip:
                    still = _unmapped(out)
                    assert still[un & skip].all() and not still[rows].any(), (what, "dst_skip rows stay unmapped, the others are filled")
                if mname == "all":
                    assert K == 0 and _export(out) == _export_as(rh, out), "every source masked: nothing is filled, and that is success"
                if oname == "idavg" and N == 8 and e == 2.0:
                    again = R.extrapolate_masked(rh, src, dst, sm, skip if use_skip else None, method, N, e, src_loc=sloc, dst_loc=dloc)
                    assert _export(again) == _export(out), (what, "two runs, the same bytes")
                    again.release()
                out.release()
    # NULL masks: the bytes of extrapolate(); a zero mask: the same bytes through the alive walk
    for oname, N, e in OPTIONS[:1] + OPTIONS[3:5]:
        method = R.EXTRAPMETHOD_NEAREST_STOD if oname == "stod" else R.EXTRAPMETHOD_NEAREST_IDAVG
        plain = R.extrapolate(rh, src, dst, method, N, e, src_loc=sloc, dst_loc=dloc)
        null = R.extrapolate_masked(rh, src, dst, None, None, method, N, e, src_loc=sloc, dst_loc=dloc)
        zero = R.extrapolate_masked(rh, src, dst, masks["none"], np.zeros(rh.n_dst, bool), method, N, e, src_loc=sloc, dst_loc=dloc)
        assert _export(null) == _export(plain) and _export(zero) == _export(plain), (name, oname, N)
        assert null.store_stats[1:4] == zero.store_stats[1:4] == plain.store_stats[1:3] + [rh.n_src]
        for x in (plain, null, zero):
            x.release()
    if own is not None:
        own.release()


def _export_as(rh, out):
    """rh's export in out's kind (a fixed handle that came back as CSR: its slots in slot order)"""
    from mpassit_amd import target_grid as tg
    e = _export(rh)
    if rh.nnz_per_row and not out.nnz_per_row:
        rowptr, col, val = tg.fixed_to_csr(*rh.weights())
        e = {"kind": 0, "shape": e["shape"], "rowptr": _raw(rowptr), "col": _raw(col), "val": _raw(val), "nnz": int(rowptr[-1]), "frac": None}
    e["frac"] = None                                  # an extrapolated handle carries no dst_frac
    return e


# ---- 3. store_masks: ESMF's masked nearest Store ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname", ["random", "ocean", "cluster", "all but three"])
def test_store_masks_nearest(world, mname):
    from mpassit_amd import regrid as R
    rh, src, sloc, dst, dloc = world["pairs"]["m2g near"]
    sm = _src_masks(world, "m2g near")[mname]
    dm = _dst_mask(rh)
    sx, dx = _xyz(world, src, sloc), _xyz(world, dst, dloc)
    idx0 = rh.weights()[0][:, 0]
    hit = (idx0 >= 0) & sm[np.maximum(idx0, 0)]
    assert hit[~dm].any() and dm.any(), "re-filled and skipped rows"
    if mname != "all but three":
        assert (~hit & (idx0 >= 0))[~dm].any(), "untouched rows"
    out = R.store_masks(rh, src, dst, sm, dm)
    assert out.nnz_per_row == 1
    idx = out.weights()[0][:, 0]
    live = np.flatnonzero(~sm)
    # brute force: the nearest unmasked cell of every destination point, ties to the lower id
    want = np.empty(rh.n_dst, np.int64)
    for p in range(rh.n_dst):
        d = dx[:, [p]] - sx[:, live]
        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        want[p] = live[np.flatnonzero(d2 == d2.min())[0]]
    assert (idx[dm] == -1).all(), "every skipped row is unmapped"
    assert np.array_equal(idx[~dm], want[~dm]), "every unskipped row holds the nearest unmasked cell"
    out.release()
    # a bilinear handle is refilled only on request
    bil = world["pairs"]["m2g bil"][0]
    a = R.store_masks(bil, src, dst, sm, dm)
    b = R.mask_handle(bil, sm, dm)
    assert _export(a) == _export(b)
    c = R.store_masks(bil, src, dst, sm, dm, extrap_method=R.EXTRAPMETHOD_NEAREST_IDAVG, num_src_pnts=3)
    d = R.extrapolate_masked(b, src, dst, sm, dm, R.EXTRAPMETHOD_NEAREST_IDAVG, 3, 2.0)
    assert _export(c) == _export(d) and c.nnz_per_row == 3
    for x in (a, b, c, d):
        x.release()


# ---- 4. consumers ---------------------------------------------------------------------------------------------------------------------------
def _held(got, want, what):
    import torch
    w = torch.from_numpy(np.ascontiguousarray(want)).cuda()
    g = got.contiguous().reshape(w.shape)
    assert g.dtype == w.dtype, (what, g.dtype, w.dtype)
    it = torch.int64 if g.dtype == torch.float64 else torch.int32
    bad = g.view(it) != w.view(it)
    assert not bool(bad.any()), (what, int(bad.sum()), bad.numel())


def test_consumers_fixed(world, gpu_lib):
    """regrid_typed (cell-fast and file order) of the masked-and-filled 3-slot Mesh -> Grid handle under every staged-kernel setting: the bits
    of the contract's host restatement on the exported pattern; NaN in every masked source never reaches a result; masked destinations +0.0"""
    import torch
    from mpassit_amd import regrid as R
    rh, src, sloc, dst, dloc = world["pairs"]["m2g bil"]
    sm = _src_masks(world, "m2g bil")["ocean"]
    dm = _dst_mask(rh)
    out = R.store_masks(rh, src, dst, sm, dm, extrap_method=R.EXTRAPMETHOD_NEAREST_IDAVG, num_src_pnts=3)
    assert out.nnz_per_row == 3
    pat = cr.Pattern.of(out)
    assert np.array_equal(pat.unmapped, dm), "every unmasked destination is mapped, every masked one is not"
    assert not sm[pat.idx[~dm]].any()
    nlev, nf = 5, 2
    x = cr.ordinary(rh.n_src, nlev, nf, 5)
    x[:, :, sm] = np.nan
    cf = torch.from_numpy(x).cuda()
    lf = cf.transpose(1, 2).contiguous()
    try:
        for ddt, tdt in ((np.float64, torch.float64), (np.float32, torch.float32)):
            want = cr.apply(pat, x, nlev, nf, dst_dtype=ddt)
            assert not np.isnan(want).any() and (want[:, :, dm] == 0).all() and not np.signbit(want[:, :, dm]).any()
            assert np.abs(want[:, :, ~dm]).min() > 0.0
            for a3 in A3:
                gpu_lib.tune("a3_staged", a3)
                for lfv in LFV:
                    gpu_lib.tune("lf_variant", lfv)
                    for layout, s in ((R.LAYOUT_CELL_FAST, cf), (R.LAYOUT_LEV_FAST, lf)):
                        _held(out.regrid_typed(s.view(-1), nlev=nlev, nfields=nf, layout=layout, out_dtype=tdt), want, ("typed", ddt, a3, lfv, layout))
    finally:
        gpu_lib.tune("a3_staged", -1)
        gpu_lib.tune("lf_variant", -1)
        out.release()


@pytest.mark.parametrize("norm_name", ["dstarea", "fracarea"])
def test_consumers_conservative(world, norm_name):
    """regrid_csr_to_mesh of a masked conservative Grid -> Mesh handle: the contract's bits; no NaN from masked sources; masked destinations
    +0.0; under FRACAREA a constant comes back constant on the mapped rows within row_len 2^-52 relative"""
    import torch
    from mpassit_amd import regrid as R
    frac = norm_name == "fracarea"
    rh, src, sloc, dst, dloc = world["pairs"]["cons g2m frac" if frac else "cons g2m"]
    sm = _src_masks(world, "cons g2m")["ocean"]
    dm = _dst_mask(rh)
    out = R.mask_handle(rh, sm, dm, R.MASKRULE_AUTO, R.NORM_FRACAREA if frac else R.NORM_DSTAREA)
    pat = cr.Pattern.of(out)
    assert not sm[pat.col].any() and pat.unmapped[dm].all() and (~pat.unmapped).any()
    nlev, nf = 3, 2
    x = cr.ordinary(rh.n_src, nlev, nf, 7)
    x[:, :, sm] = np.nan
    cf = torch.from_numpy(x).cuda()
    for ddt, tdt in ((np.float64, torch.float64), (np.float32, torch.float32)):
        for layout, lev_fast in ((R.LAYOUT_CELL_FAST, False), (R.LAYOUT_LEV_FAST, True)):
            want = cr.apply(pat, x, nlev, nf, dst_dtype=ddt, dst_lev_fast=lev_fast)
            assert not np.isnan(want).any()
            wd = want[:, dm, :] if lev_fast else want[:, :, dm]
            assert (wd == 0).all() and not np.signbit(wd).any()
            _held(out.regrid_csr_to_mesh(cf, nlev=nlev, nfields=nf, layout=layout, out_dtype=tdt), want, ("csr_to_mesh", norm_name, ddt, layout))
    if frac:
        const = torch.full((1, 1, rh.n_src), 273.15, dtype=torch.float64, device="cuda")
        const[0, 0, torch.from_numpy(sm).cuda()] = float("nan")
        got = out.regrid_csr_to_mesh(const, nlev=1, nfields=1, out_dtype=torch.float64).reshape(-1).cpu().numpy()
        lens = np.diff(pat.rowptr)
        mapped = lens > 0
        assert mapped.sum() > 100
        rel = np.abs(got[mapped] - 273.15) / 273.15
        # each w' = w / Wk carries half an ulp, the products another, the row's sum at most row_len - 1 more: row_len 2^-52 covers them
        print("constant field: worst %.3g eps, longest row %d" % (rel.max() / EPS, lens.max()))
        assert (rel <= lens[mapped] * EPS).all()
        assert (got[~mapped] == 0).all()
    out.release()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(world, gpu_lib):
    from mpassit_amd import _lib as L, regrid as R, target_grid as tg
    lib = L.load()
    o = world["obj"]
    bil, near, cons = (world["pairs"][k][0] for k in ("m2g bil", "m2g near", "cons m2g"))
    INV, UNS = L.MPG_ERR_INVALID_ARG, L.MPG_ERR_UNSUPPORTED
    h = C.c_void_p()

    def refused(rc, want, who, *words):
        msg = lib.mpg_last_error().decode()
        assert rc == want and msg.startswith(who + ":"), (rc, want, msg)
        for word in words:
            assert word in msg, msg
        assert h.value is None, "a refused call leaves *out alone"

    def mask(rh, rule=0, norm=0, out=h, opts=True):
        op = L.StoreMaskOpts(src_mask_dev=None, dst_mask_dev=None, rule=rule, norm_type=norm)
        return L.handle_mask(rh._h if rh is not None else None, C.byref(op) if opts else None, C.byref(out) if out is not None else None)

    who = "mpg_handle_mask"
    refused(mask(None), INV, who, "NULL")
    refused(mask(bil, out=None), INV, who, "NULL")
    refused(mask(bil, opts=False), INV, who, "NULL")
    refused(mask(bil, rule=3), INV, who, "rule")
    refused(mask(bil, rule=-1), INV, who, "rule")
    refused(mask(cons, rule=2, norm=2), INV, who, "norm_type")
    refused(mask(cons, rule=0, norm=-1), INV, who, "norm_type")
    refused(mask(bil, rule=2), UNS, who, "mpg_handle_get_weights", "mpg_handle_from_weights")
    refused(mask(near, rule=2), UNS, who, "mpg_handle_from_weights")
    assert mask(bil, rule=1, norm=77) == 0, "norm_type is read under the ENTRY rule only"
    L.check(lib.mpg_handle_release(h))
    h.value = None
    # AUTO needs a method: from-weights and composed handles record none
    idx, w = bil.weights()
    rowptr, col, val = tg.fixed_to_csr(idx, w)
    fw = R.RouteHandle.from_weights(bil.n_src, bil.nx_dst, bil.ny_dst, np.repeat(np.arange(1, bil.n_dst + 1, dtype=np.int32), np.diff(rowptr)),
                                    (col + 1).astype(np.int32), val)
    e1 = world["pairs"]["g2g e1"][0]
    comp = R.compose(e1, bil)
    for x in (fw, comp):
        refused(mask(x, rule=0), INV, who, "MPG_MASKRULE_ROW or MPG_MASKRULE_ENTRY")
    for rule in (1, 2):
        assert mask(comp, rule=rule) == 0, "an explicit rule serves a handle without a method"
        L.check(lib.mpg_handle_release(h))
        h.value = None
    # pole terms, a localized handle
    pole = R.regrid_store_grid(o["per"], R.STAGGERLOC_EDGE2)
    assert pole.pole()[0].size > 0
    refused(mask(pole, rule=1), UNS, who, "mpg_handle_pole_count > 0")
    fw.localize()
    refused(mask(fw, rule=1), UNS, who, "localized or rebased")
    # the masked extrapolation refuses as the plain one does, under its own name
    who = "mpg_handle_extrapolate_masked"

    def ex(rh=bil, src=None, dst=None, method=1, N=8, e=2.0, out=h, null_opts=False):
        ps = R._points(o["mesh_in"], 0, "x") if src is None else src
        pd = R._points(o["grid"], 0, "x") if dst is None else dst
        opts = L.ExtrapOpts(method=method, num_src_pnts=N, dist_exponent=e)
        return L.handle_extrapolate_masked(rh._h if rh is not None else None, C.byref(ps), C.byref(pd), None if null_opts else C.byref(opts), None, None,
                                           C.byref(out) if out is not None else None)

    refused(ex(rh=None), INV, who, "NULL")
    refused(ex(out=None), INV, who, "NULL")
    refused(ex(null_opts=True), INV, who, "NULL")
    refused(ex(method=0), INV, who, "method")
    refused(ex(method=2, N=9), INV, who, "num_src_pnts = 9")
    refused(ex(method=2, e=float("nan")), INV, who, "dist_exponent")
    refused(ex(src=R._points(o["mesh_over"], 0, "x")), INV, who, "n_src = %d" % bil.n_src)
    refused(ex(src=R._points(o["mesh_in"], R.MESHLOC_NODE, "x")), INV, who, "MPG_MESHLOC_ELEMENT")
    refused(ex(dst=R._points(o["grid"], R.STAGGERLOC_EDGE1, "x")), INV, who, "n_dst = %d" % bil.n_dst)
    refused(ex(rh=pole, src=R._points(o["per"], 0, "x"), dst=R._points(o["per"], R.STAGGERLOC_EDGE2, "x")), UNS, who, "mpg_handle_pole_count > 0")
    refused(ex(rh=fw), UNS, who, "localized or rebased")
    # the wrappers' own checks, and the library still works afterwards
    with pytest.raises(ValueError):
        R.mask_handle(bil, np.zeros(bil.n_src + 1, bool))
    with pytest.raises(ValueError):
        R.mask_handle(bil, np.zeros(bil.n_src, np.float64))
    with pytest.raises(ValueError):
        R.extrapolate_masked(bil, o["mesh_in"], o["grid"], dst_skip=np.zeros(3, bool))
    again = R.mask_handle(bil)
    assert _export(again) == _export(bil)
    for x in (again, fw, comp, pole):
        x.release()
