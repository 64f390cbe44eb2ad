"""Nearest destination to source on the GPU at small sizes (mpg_regrid_store_nearest_dtos): rowptr, col and nearest[] EXACTLY and val BIT FOR
BIT against the numpy mirror target_grid.nearest_dtos_rows fed with the library's own unit vectors (Mesh.xyz / Grid.xyz) -- every result
is discrete or one rounded division, so no comparison carries a tolerance -- on every pairing of source set and destination kind, at the
shapes that can go wrong, under masks, on an exact tie, twice on fresh objects, under every CSR consumer, and the refusals.

Not reached by any test: the MPG_ERR_OVERFLOW refusal (a point set beyond int32 ids cannot be made at these sizes)."""
import ctypes as C

import numpy as np
import pytest

import _contract_ref as cr
from conftest import LAMBERT

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _raw(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _grid(R, nx, ny, lon0=-110.0, lat0=28.0, width=26.0, height=18.0, jitter=0.0, seed=0):
    """a CENTER-only grid of nx x ny points spread over a lon / lat rectangle (degrees), optionally jittered"""
    rng = np.random.default_rng(seed)
    lon, lat = np.meshgrid(lon0 + width * (np.arange(nx) + 0.5) / nx, lat0 + height * (np.arange(ny) + 0.5) / ny)
    if jitter:
        lon, lat = lon + rng.uniform(-jitter, jitter, lon.shape), lat + rng.uniform(-jitter, jitter, lat.shape)
    return R.Grid(lon, lat)


def _cloud(rng, n, centre=(37.0, -97.0), half=(9.0, 13.0)):
    """n points around `centre` (degrees) -> (lat, lon) in radians"""
    return np.deg2rad(centre[0] + half[0] * rng.uniform(-1, 1, n)), np.deg2rad(centre[1] + half[1] * rng.uniform(-1, 1, n))


def _bare_mesh(R, lat, lon):
    """a mesh of cell centres alone: three vertices nobody uses, verticesOnCell empty"""
    n = lat.size
    return R.Mesh(lat, lon, np.zeros(3), np.array([0.0, 0.1, 0.2]), np.zeros((n, 3), np.int32))


def _host(m):
    """a mask as the mirror reads it: numpy, wherever the Store's copy lives"""
    return m.cpu().numpy() if hasattr(m, "cpu") else m


def _n(obj, loc):
    return obj.xyz(loc).shape[1]


def _store_and_check(R, tg, src, sloc, dst, dloc, norm, src_mask=None, dst_mask=None, what=""):
    """one Store against the mirror -> (handle, (rowptr, col, val, nearest) of the mirror)"""
    rh = R.regrid_store_nearest_dtos(src, dst, norm, src_mask, dst_mask, sloc, dloc)
    sx, dx = src.xyz(sloc), dst.xyz(dloc)
    want = tg.nearest_dtos_rows(sx, dx, norm, _host(src_mask), _host(dst_mask))
    rowptr, col, val = rh.csr()
    near = rh.src_nearest()
    what = (what, norm)
    assert (rh.n_src, rh.n_dst, rh.nnz_per_row) == (sx.shape[1], dx.shape[1], 0), what
    assert rh.nx_dst * rh.ny_dst == rh.n_dst, what
    assert near.dtype == np.int32 and np.array_equal(near, want[3]), (what, "nearest", int((near != want[3]).sum()))
    assert np.array_equal(rowptr, want[0]), (what, "rowptr")
    assert np.array_equal(col, want[1]), (what, "col")
    assert val.size == want[2].size and np.array_equal(_bits(val), _bits(want[2])), (what, "val")
    lens = np.diff(want[0])
    stats = rh.store_stats
    assert (rh.nnz, stats[1], stats[2], stats[3]) == (col.size, col.size, int((lens > 0).sum()), int(lens.max(initial=0))), (what, stats[:4])
    return rh, want


@pytest.fixture(scope="module")
def world(gpu_lib):
    from mpassit_amd import regrid as R, synth, target_grid as tg
    g = tg.define_target_grid_params("lambert", 31, 21, dx=60000.0, dy=60000.0, **LAMBERT)
    gc = tg.define_target_grid_params("lambert", 13, 9, dx=150000.0, dy=150000.0, **LAMBERT)
    gp = tg.define_target_grid_params("lat-lon", nx=25, ny=13, stand_lon=0.0, is_regional=False)
    m = synth.mesh_edges(synth.regional_mesh_for_lambert(g.proj, 31, 21, 601, margin=0.05, seed=11))
    obj = dict(grid=R.Grid.from_target(g), coarse=R.Grid.from_target(gc), per=R.Grid.from_target(gp), mesh=R.Mesh.from_mpas(m))
    assert (obj["per"].nx, obj["per"].ny) == (24, 12) and obj["mesh"].nEdges > 0
    d = dict(obj=obj, m=m, handles={})
    yield d
    for h in d["handles"].values():
        h.release()
    for x in obj.values():
        x.destroy()


def _sources(R, o):
    return {"cells": (o["mesh"], R.MESHLOC_ELEMENT), "vertices": (o["mesh"], R.MESHLOC_NODE), "edges": (o["mesh"], R.MESHLOC_EDGE),
            "center": (o["grid"], R.STAGGERLOC_CENTER), "edge1": (o["grid"], R.STAGGERLOC_EDGE1), "corner": (o["grid"], R.STAGGERLOC_CORNER),
            "periodic": (o["per"], R.STAGGERLOC_CENTER)}


SOURCES = ("cells", "vertices", "edges", "center", "edge1", "corner", "periodic")


# ---- 1. the pairings ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst_kind", ("grid", "mesh"))
@pytest.mark.parametrize("src_name", SOURCES)
def test_pairings(world, src_name, dst_kind):
    from mpassit_amd import regrid as R, target_grid as tg
    o = world["obj"]
    src, sloc = _sources(R, o)[src_name]
    dst, dloc = (o["coarse"], R.STAGGERLOC_EDGE2) if dst_kind == "grid" else (o["mesh"], R.MESHLOC_ELEMENT)
    for norm in (R.DTOS_SUM, R.DTOS_MEAN):
        rh, want = _store_and_check(R, tg, src, sloc, dst, dloc, norm, what=(src_name, dst_kind))
        lens = np.diff(want[0])
        print("%s -> %s, norm %d: %d sources, %d of %d rows non-empty, longest %d, store %.3f ms" % (
            src_name, dst_kind, norm, rh.n_src, int((lens > 0).sum()), rh.n_dst, int(lens.max()), rh.store_ms))
        assert want[1].size == rh.n_src and rh.store_ms > 0.0
        if norm == R.DTOS_SUM:
            assert (want[2] == 1.0).all()
        if dst_kind == "grid":
            assert (rh.ny_dst, rh.nx_dst) == dst.stagger_shape(dloc)
        else:
            assert (rh.nx_dst, rh.ny_dst) == (dst.nCells, 1)
        rh.release()


# ---- 2. the shapes that can go wrong --------------------------------------------------------------------------------------------------------
def test_fine_to_coarse(gpu_lib):
    """96 x 48 points onto 4 x 3: rows several hundred entries long, across the 64- and 256-lane boundaries; and everything onto a
    destination of one point: one row, one counter"""
    from mpassit_amd import regrid as R, target_grid as tg
    fine, coarse = _grid(R, 96, 48, jitter=0.05, seed=1), _grid(R, 4, 3, jitter=1.0, seed=2)
    one = _bare_mesh(R, np.deg2rad(np.array([37.0])), np.deg2rad(np.array([-97.0])))
    for norm in (R.DTOS_SUM, R.DTOS_MEAN):
        rh, want = _store_and_check(R, tg, fine, R.STAGGERLOC_CENTER, coarse, R.STAGGERLOC_CENTER, norm, what="96x48 -> 4x3")
        lens = np.diff(want[0])
        assert lens.sum() == 96 * 48 and lens.min() > 256 and len(set(lens % 64)) > 1, lens
        rh.release()
        rh, want = _store_and_check(R, tg, fine, R.STAGGERLOC_CENTER, one, R.MESHLOC_ELEMENT, norm, what="96x48 -> 1")
        assert np.array_equal(want[0], [0, 96 * 48]) and np.array_equal(want[1], np.arange(96 * 48)) and (want[3] == 0).all()
        assert rh.store_stats[3] == 96 * 48
        rh.release()
    for x in (fine, coarse, one):
        x.destroy()


def test_coarse_to_fine_and_identity(gpu_lib):
    """5 x 3 onto 64 x 40: most rows empty; a source grid equal to the destination grid: the identity pattern in row order"""
    from mpassit_amd import regrid as R, target_grid as tg
    coarse, fine = _grid(R, 5, 3, jitter=0.7, seed=3), _grid(R, 64, 40, jitter=0.02, seed=4)
    for norm in (R.DTOS_SUM, R.DTOS_MEAN):
        rh, want = _store_and_check(R, tg, coarse, R.STAGGERLOC_CENTER, fine, R.STAGGERLOC_CENTER, norm, what="5x3 -> 64x40")
        assert (np.diff(want[0]) == 0).sum() >= 64 * 40 - 15 and want[1].size == 15
        rh.release()
        rh, want = _store_and_check(R, tg, fine, R.STAGGERLOC_CENTER, fine, R.STAGGERLOC_CENTER, norm, what="identity")
        n = 64 * 40
        assert np.array_equal(want[0], np.arange(n + 1)) and np.array_equal(want[1], np.arange(n)) and (want[2] == 1.0).all()
        rh.release()
    coarse.destroy()
    fine.destroy()


@pytest.mark.parametrize("n_src", (1, 255, 256, 257))
def test_block_boundaries(gpu_lib, n_src):
    """n_src at and around one workgroup of 256 lanes, as mesh cells (the Morton-ordered visit) onto a grid and onto mesh cells"""
    from mpassit_amd import regrid as R, target_grid as tg
    rng = np.random.default_rng(n_src)
    src = _bare_mesh(R, *_cloud(rng, n_src))
    gd, md = _grid(R, 5, 3, jitter=0.5, seed=5), _bare_mesh(R, *_cloud(rng, 9))
    for norm in (R.DTOS_SUM, R.DTOS_MEAN):
        _store_and_check(R, tg, src, R.MESHLOC_ELEMENT, gd, R.STAGGERLOC_CENTER, norm, what=(n_src, "grid"))[0].release()
        _store_and_check(R, tg, src, R.MESHLOC_ELEMENT, md, R.MESHLOC_ELEMENT, norm, what=(n_src, "mesh"))[0].release()
    for x in (src, gd, md):
        x.destroy()


# ---- 3. masks -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst_kind", ("grid", "mesh"))
def test_masks(world, dst_kind):
    from mpassit_amd import regrid as R, target_grid as tg
    import torch
    o = world["obj"]
    src, sloc = o["mesh"], R.MESHLOC_NODE
    dst, dloc = (o["coarse"], R.STAGGERLOC_CENTER) if dst_kind == "grid" else (o["mesh"], R.MESHLOC_ELEMENT)
    ns, nd = _n(src, sloc), _n(dst, dloc)
    rng = np.random.default_rng(21)
    sm, dm = rng.uniform(size=ns) < 0.3, rng.uniform(size=nd) < 0.4
    free, base = _store_and_check(R, tg, src, sloc, dst, dloc, R.DTOS_SUM, what="no mask")
    free.release()
    for norm in (R.DTOS_SUM, R.DTOS_MEAN):
        rh, want = _store_and_check(R, tg, src, sloc, dst, dloc, norm, src_mask=sm, what="src mask")
        assert (want[3][sm] == -1).all() and np.array_equal(want[3][~sm], base[3][~sm])
        rh.release()
        # a masked nearest destination passes its sources to the next unmasked one
        rh, want = _store_and_check(R, tg, src, sloc, dst, dloc, norm, dst_mask=dm.astype(np.uint8), what="dst mask")
        moved = dm[base[3]]
        assert moved.any() and (want[3] >= 0).all() and not dm[want[3]].any() and np.array_equal(want[3][~moved], base[3][~moved])
        assert (np.diff(want[0])[dm] == 0).all()
        rh.release()
        rh, want = _store_and_check(R, tg, src, sloc, dst, dloc, norm, src_mask=torch.from_numpy(sm).cuda(), dst_mask=torch.from_numpy(dm), what="both")
        assert (want[3][sm] == -1).all() and not dm[want[3][~sm]].any()
        rh.release()
        rh, want = _store_and_check(R, tg, src, sloc, dst, dloc, norm, dst_mask=np.ones(nd, bool), what="every dst masked")
        assert (want[3] == -1).all() and (want[0] == 0).all() and rh.nnz == 0
        rh.release()
        rh, want = _store_and_check(R, tg, src, sloc, dst, dloc, norm, src_mask=np.ones(ns, np.uint8), what="every src masked")
        assert (want[3] == -1).all() and rh.nnz == 0 and rh.store_stats[2] == 0
        rh.release()


# ---- 4. ties --------------------------------------------------------------------------------------------------------------------------------
def test_equator_tie_goes_to_the_lower_id(gpu_lib):
    """destination points at lat +-a on one meridian, the source on the equator of that meridian: the two d2 are equal bit for bit (only
    the sign of dz differs), and the lower id wins -- in either listing order, in a BVH and in a pyramid"""
    from mpassit_amd import regrid as R, target_grid as tg
    rng = np.random.default_rng(31)
    a, L0 = 0.3, 0.5
    src = _bare_mesh(R, np.array([0.0, 0.0]), np.array([L0, L0]))
    for flip in (1.0, -1.0):
        lat, lon = rng.uniform(-0.4, 0.4, 40), L0 + 1.5 + rng.uniform(-0.3, 0.3, 40)      # 38 points far away ...
        lat[5], lon[5], lat[31], lon[31] = flip * a, L0, -flip * a, L0                     # ... and the pair, in two different leaves
        dst = _bare_mesh(R, lat, lon)
        s, d = src.xyz(), dst.xyz()
        d2 = ((s[:, :1] - d) ** 2)
        d2 = (d2[0] + d2[1]) + d2[2]
        assert d2[5] == d2[31] and (np.delete(d2, [5, 31]) > d2[5]).all(), "the test's own premise: an exact tie"
        for norm in (R.DTOS_SUM, R.DTOS_MEAN):
            rh, want = _store_and_check(R, tg, src, R.MESHLOC_ELEMENT, dst, R.MESHLOC_ELEMENT, norm, what=("tie", flip))
            assert np.array_equal(rh.src_nearest(), [5, 5])
            rh.release()
        dm = np.zeros(40, bool)
        dm[5] = True
        rh, _ = _store_and_check(R, tg, src, R.MESHLOC_ELEMENT, dst, R.MESHLOC_ELEMENT, R.DTOS_SUM, dst_mask=dm, what=("tie, lower masked", flip))
        assert np.array_equal(rh.src_nearest(), [31, 31])
        rh.release()
        dst.destroy()
        # a grid's pyramid: rows of latitude -a and +a (flipped: +a and -a), the first column on the source's meridian
        lon2, lat2 = np.meshgrid(np.rad2deg(L0) + np.array([0.0, 9.0, 18.0, 27.0, 36.0]), np.rad2deg(a) * np.array([-flip, flip]))
        gd = R.Grid(lon2, lat2)
        d = gd.xyz()
        sq = (s[:, :1] - d) ** 2
        sq = (sq[0] + sq[1]) + sq[2]
        assert sq[0] == sq[5] and (sq[[1, 2, 3, 4, 6, 7, 8, 9]] > sq[0]).all(), "the test's own premise: an exact tie"
        rh, _ = _store_and_check(R, tg, src, R.MESHLOC_ELEMENT, gd, R.STAGGERLOC_CENTER, R.DTOS_SUM, what=("grid tie", flip))
        assert np.array_equal(rh.src_nearest(), [0, 0])
        rh.release()
        gd.destroy()
    src.destroy()


# ---- 5. determinism -------------------------------------------------------------------------------------------------------------------------
def test_two_stores_on_fresh_objects_give_the_same_bytes(world):
    from mpassit_amd import regrid as R
    m = world["m"]
    got = []
    for _ in range(2):
        mesh, fine, coarse = R.Mesh.from_mpas(m), _grid(R, 96, 48, jitter=0.05, seed=1), _grid(R, 4, 3, jitter=1.0, seed=2)
        out = []
        for src, sloc, dst, dloc in ((mesh, R.MESHLOC_EDGE, coarse, R.STAGGERLOC_CENTER), (fine, R.STAGGERLOC_CENTER, mesh, R.MESHLOC_ELEMENT),
                                     (fine, R.STAGGERLOC_CENTER, coarse, R.STAGGERLOC_CENTER)):
            rh = R.regrid_store_nearest_dtos(src, dst, R.DTOS_MEAN, None, None, sloc, dloc)
            out += [_raw(a).copy() for a in rh.csr()] + [_raw(rh.src_nearest()).copy()]
            rh.release()
        got.append(out)
        for x in (mesh, fine, coarse):
            x.destroy()
    assert len(got[0]) == 12 and all(np.array_equal(a, b) for a, b in zip(*got))


# ---- 6. consumers ---------------------------------------------------------------------------------------------------------------------------
def _handle(world, name):
    from mpassit_amd import regrid as R
    o = world["obj"]
    if name not in world["handles"]:
        src, sloc, dst, dloc, norm = {
            "long sum": (o["mesh"], R.MESHLOC_NODE, o["coarse"], R.STAGGERLOC_CENTER, R.DTOS_SUM),
            "long mean": (o["mesh"], R.MESHLOC_NODE, o["coarse"], R.STAGGERLOC_CENTER, R.DTOS_MEAN),
            "sparse sum": (o["mesh"], R.MESHLOC_ELEMENT, o["grid"], R.STAGGERLOC_CORNER, R.DTOS_SUM),
            "grid sum": (o["grid"], R.STAGGERLOC_CENTER, o["coarse"], R.STAGGERLOC_CENTER, R.DTOS_SUM),
        }[name]
        world["handles"][name] = R.regrid_store_nearest_dtos(src, dst, norm, None, None, sloc, dloc)
    return world["handles"][name]


@pytest.mark.parametrize("name", ("long sum", "long mean", "sparse sum"))
def test_regrid_typed_and_rows(world, name):
    """regrid_typed in float32 and float64 and regrid_csr_rows against the CSR restatement of tests/_contract_ref.py, bit for bit; the
    source field has random mantissas, so the summation order shows"""
    import torch
    rh = _handle(world, name)
    pat = cr.Pattern.of(rh)
    lens = np.diff(pat.rowptr)
    assert lens.max() >= 2 and (name != "sparse sum" or (lens == 0).any())
    nlev, nf = 3, 2
    x = cr.ordinary(rh.n_src, nlev, nf, 3)
    tdt = {np.float32: torch.float32, np.float64: torch.float64}
    for sdt in (np.float32, np.float64):
        xs = x.astype(sdt)
        dev = torch.from_numpy(xs).cuda()
        lf = dev.transpose(1, 2).contiguous()
        for ddt in (np.float32, np.float64):
            want = cr.apply(pat, xs, nlev, nf, dst_dtype=ddt)
            got = rh.regrid_typed(dev.view(-1), nlev=nlev, nfields=nf, out_dtype=tdt[ddt])
            assert np.array_equal(_raw(got), _raw(want)), (name, "typed", sdt, ddt)
            want = cr.apply(pat, xs, nlev, nf, dst_dtype=ddt, dst_lev_fast=True)
            got = rh.regrid_csr_rows(lf, nlev=nlev, nfields=nf, out_dtype=tdt[ddt])
            assert np.array_equal(_raw(got), _raw(want)), (name, "rows", sdt, ddt)
            got = rh.regrid_csr_to_mesh(dev.view(-1), nlev=nlev, nfields=nf, out_dtype=tdt[ddt])
            assert np.array_equal(_raw(got), _raw(cr.apply(pat, xs, nlev, nf, dst_dtype=ddt))), (name, "csr_to_mesh", sdt, ddt)
    # what the sum rule means: a count per destination
    if name.endswith("sum"):
        ones = rh.regrid_typed(torch.ones(rh.n_src, dtype=torch.float64, device="cuda")).reshape(-1).cpu().numpy()
        assert np.array_equal(ones, lens.astype(np.float64)) and not np.signbit(ones).any()


def test_transpose_is_the_nearest_gather(world):
    import torch
    rh = _handle(world, "sparse sum")
    near = rh.src_nearest()
    nlev, nf = 2, 2
    g = cr.ordinary(rh.n_dst, nlev, nf, 4)
    got = rh.regrid_transpose(torch.from_numpy(g).cuda().reshape(nf, nlev, rh.ny_dst, rh.nx_dst), nlev=nlev, nfields=nf).cpu().numpy()
    assert (near >= 0).all()
    assert np.array_equal(_raw(got), _raw(g[:, :, near]))
    # ... with +0.0 where nearest is -1
    from mpassit_amd import regrid as R
    o = world["obj"]
    sm = np.arange(rh.n_src) % 3 == 0
    masked = R.regrid_store_nearest_dtos(o["mesh"], o["grid"], R.DTOS_SUM, sm, None, R.MESHLOC_ELEMENT, R.STAGGERLOC_CORNER)
    near = masked.src_nearest()
    assert np.array_equal(near < 0, sm)
    got = masked.regrid_transpose(torch.from_numpy(g).cuda().reshape(nf, nlev, rh.ny_dst, rh.nx_dst), nlev=nlev, nfields=nf).cpu().numpy()
    want = np.where(near >= 0, g[:, :, np.maximum(near, 0)], 0.0)
    assert np.array_equal(_raw(got), _raw(want))
    masked.release()


def test_regrid_masked_fills_the_empty_rows(world):
    import torch
    rh = _handle(world, "sparse sum")
    empty = np.diff(rh.csr()[0]) == 0
    assert empty.any() and not empty.all()
    x = torch.from_numpy(cr.ordinary(rh.n_src, 2, 1, 8)).cuda()
    got = rh.regrid_masked(x.view(-1), nlev=2, nfields=1, missing=None, fill_value=-777.0).cpu().numpy().reshape(2, -1)
    plain = rh.regrid_typed(x.view(-1), nlev=2, nfields=1).cpu().numpy().reshape(2, -1)
    assert (got[:, empty] == -777.0).all() and np.array_equal(_bits(got[:, ~empty]), _bits(plain[:, ~empty]))
    assert (plain[:, empty] == 0.0).all() and not np.signbit(plain[:, empty]).any()


def test_compose_with_a_bilinear_handle(world):
    """compose(dtos, bilinear): the mesh's cells bilinearly onto the grid's points, those points binned onto the coarse grid"""
    from mpassit_amd import regrid as R, target_grid as tg
    o = world["obj"]
    outer = _handle(world, "grid sum")
    inner = R.regrid_store(o["mesh"], o["grid"], R.REGRIDMETHOD_BILINEAR)
    c = R.compose(outer, inner)
    a = outer.csr()
    b = tg.fixed_to_csr(*inner.weights())
    want = tg.compose_csr(a[0], a[1], a[2], b[0], b[1], b[2])
    got = c.csr()
    assert (c.n_src, c.n_dst) == (inner.n_src, outer.n_dst) and got[1].size > 0
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(_bits(got[2]), _bits(np.asarray(want[2]).reshape(-1)))
    c.release()
    inner.release()


def test_mask_handle_auto_is_refused(world):
    from mpassit_amd import _lib as L, regrid as R
    rh = _handle(world, "sparse sum")
    dm = np.zeros(rh.n_dst, bool)
    dm[::2] = True
    with pytest.raises(L.MpgError) as e:
        R.mask_handle(rh, dst_mask=dm, rule=R.MASKRULE_AUTO)
    assert e.value.rc == L.MPG_ERR_UNSUPPORTED and "mpg_handle_mask" in str(e.value) and "mpg_regrid_store_nearest_dtos" in str(e.value)
    assert "dst_mask_dev" in str(e.value)
    # the explicit rules keep working as for any CSR handle
    out = R.mask_handle(rh, dst_mask=dm, rule=R.MASKRULE_ROW)
    lens, before = np.diff(out.csr()[0]), np.diff(rh.csr()[0])
    assert (lens[dm] == 0).all() and np.array_equal(lens[~dm], before[~dm])
    out.release()
    # the to_esmf_weights() export and a handle of another origin
    row, col, S = rh.to_esmf_weights()[:3]
    assert len(S) == rh.nnz
    other = R.regrid_store(world["obj"]["mesh"], world["obj"]["grid"], R.REGRIDMETHOD_NEAREST_STOD)
    with pytest.raises(L.MpgError) as e:
        other.src_nearest()
    assert e.value.rc == L.MPG_ERR_INVALID_ARG and "mpg_handle_get_src_nearest" in str(e.value)
    other.release()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(world):
    from mpassit_amd import _lib as L, regrid as R
    lib = L.load()
    o = world["obj"]
    who = "mpg_regrid_store_nearest_dtos"
    INV, UNS = L.MPG_ERR_INVALID_ARG, L.MPG_ERR_UNSUPPORTED
    h = C.c_void_p()

    def pts(obj, loc=0):
        return R._points(obj, loc, "x")

    def call(src=None, dst=None, norm=0, out=h):
        ps = pts(o["mesh"]) if src is None else src
        pd = pts(o["coarse"]) if dst is None else dst
        return L.regrid_store_nearest_dtos(C.byref(ps) if ps != "null" else None, C.byref(pd) if pd != "null" else None, norm, None, None,
                                           C.byref(out) if out is not None else None)

    def refused(rc, want, *words):
        msg = lib.mpg_last_error().decode()
        assert rc == want and who in msg, (rc, want, msg)
        for word in words:
            assert word in msg, msg

    assert call() == 0
    L.check(lib.mpg_handle_release(h))
    h = C.c_void_p()
    refused(call(src="null"), INV, "NULL")
    refused(call(dst="null"), INV, "NULL")
    refused(call(out=None), INV, "NULL")
    both = L.Points(mesh=o["mesh"]._h, meshloc=0, grid=o["grid"]._h, staggerloc=0)
    neither = L.Points(mesh=None, meshloc=0, grid=None, staggerloc=0)
    refused(call(src=both), INV, "both")
    refused(call(dst=neither), INV, "neither")
    refused(call(norm=2), INV, "MPG_DTOS_SUM")
    refused(call(src=pts(o["mesh"], 7)), INV, "mesh location")
    refused(call(dst=pts(o["coarse"], 4)), INV, "stagger")
    bare = _grid(R, 6, 5)
    refused(call(src=pts(bare, R.STAGGERLOC_EDGE1)), INV, "no coordinates")
    refused(call(dst=pts(bare, R.STAGGERLOC_CORNER)), INV, "no coordinates")
    noedges = _bare_mesh(R, *_cloud(np.random.default_rng(1), 12))
    refused(call(src=pts(noedges, R.MESHLOC_EDGE)), INV, "mpg_mesh_set_edges")
    refused(call(dst=pts(o["mesh"], R.MESHLOC_NODE)), UNS, "MPG_MESHLOC_ELEMENT")
    refused(call(dst=pts(o["mesh"], R.MESHLOC_EDGE)), UNS, "MPG_MESHLOC_ELEMENT")
    win = R.Mesh.from_mpas(world["m"], window_grid=o["grid"])
    refused(call(src=pts(win)), UNS, "mpg_mesh_create_window")
    refused(call(dst=pts(win)), UNS, "mpg_mesh_create_window")
    noedges.set_source_window(2, 5)
    refused(call(dst=pts(noedges)), UNS, "mpg_mesh_set_source_window")
    assert h.value is None
    # empty input is success: every source masked is an all-empty pattern (test_masks); nothing was left behind by the refusals
    for x in (bare, noedges, win):
        x.destroy()
