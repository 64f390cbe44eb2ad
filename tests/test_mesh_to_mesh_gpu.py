"""Mesh -> Mesh on the GPU at small sizes: the Store (mpg_regrid_store_mesh, through the C-ABI) against the oracle's all-triangles search
(orc_bilinear_weights: the lowest passing triangle id) for both line types and against its brute-force nearest search, the all-ties
identity case src == dst, the independence of the answer from the source mesh's numbering, and the contract around the Store: handle
shape, cache, source windows, refusals, and the other consumers of a fixed handle.

The mesh pairs and the oracle's answers come from tests/_mesh_to_mesh_cases.py; test_mesh_to_mesh_abi.py qualifies them on the CPU."""
import ctypes as C

import numpy as np
import pytest

import _mesh_to_mesh_cases as MC
from _parity_helpers import assert_fixed_weights_equal, assert_nearest_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(gpu_lib):
    """Device meshes by name, created on first use, destroyed at the end of the module."""
    from mpassit_amd import regrid as R
    made = {}

    def get(name):
        if name not in made:
            made[name] = R.Mesh.from_mpas(MC.mesh(name))
        return made[name]

    yield get
    for m in made.values():
        m.destroy()


def _store(src, dst, method=0, src_loc=0, dst_loc=0):
    """mpg_regrid_store_mesh through the C-ABI -> RouteHandle."""
    from mpassit_amd import _lib as L, regrid as R
    h = C.c_void_p()
    L.check(L.regrid_store_mesh(src._h, src_loc, dst._h, dst_loc, method, C.byref(h)))
    return R.RouteHandle(h)


_NAMES = {"geo10_to_vor1500": ("geo10", "vor1500"), "vor2500_to_hex": ("vor2500", "hex_small"), "hex_to_geo10": ("hex_large", "geo10"),
          "varres3000_to_geo8": ("varres3000", "geo8"), "geo10_to_vor1500_nodes": ("geo10", "vor1500")}


def _bytes_equal(a, b):
    import torch
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    bits = torch.int64 if a.dtype == torch.float64 else torch.int32
    return torch.equal(a.reshape(-1).view(bits), b.reshape(-1).view(bits))


@pytest.mark.parametrize("linetype", [0, 1])
@pytest.mark.parametrize("name", MC.PAIR_NAMES)
def test_store_parity_bilinear(dev, gpu_lib, oracle, name, linetype):
    sname, dname = _NAMES[name]
    src_m, dst_m, loc = MC.pair(name)
    oi, ow, pts, _ = MC.oracle_bilinear(oracle, name, linetype)
    assert MC.edge_share(oi, ow) <= MC.TIE_CAP
    gpu_lib.tune("bilinear_linetype", linetype)
    try:
        rh = _store(dev(sname), dev(dname), 0, 0, loc)
    finally:
        gpu_lib.tune("bilinear_linetype", 0)
    n = pts.shape[0]
    assert (rh.n_src, rh.n_dst, rh.nx_dst, rh.ny_dst, rh.nnz_per_row, rh.nnz) == (src_m.nCells, n, n, 1, 3, 3 * n)
    assert rh.store_stats[2] == n and rh.store_ms > 0.0 and rh.store_path == 0
    gi, gw = rh.weights()
    ties = assert_fixed_weights_equal(oi, ow, gi, gw)          # mapped mask identical, weights within 1e-11, every differing point examined
    mapped = gi[:, 0] >= 0
    print("%s linetype %d: %d mapped of %d, %d tie points" % (name, linetype, int(mapped.sum()), n, ties))
    assert ties <= MC.TIE_CAP * mapped.sum()
    assert (gw[~mapped] == 0.0).all() and (gi[~mapped] == -1).all()
    rh.release()


@pytest.mark.parametrize("name", ["geo10_to_vor1500", "hex_to_geo10", "geo10_to_vor1500_nodes"])
def test_store_parity_nearest(dev, oracle, name):
    from mpassit_amd import regrid as R
    sname, dname = _NAMES[name]
    src_m, dst_m, loc = MC.pair(name)
    rh = _store(dev(sname), dev(dname), R.REGRIDMETHOD_NEAREST_STOD, 0, loc)
    cx, pts = MC.cell_xyz(oracle, src_m), MC.points(oracle, dst_m, loc)
    n = pts.shape[0]
    assert (rh.n_src, rh.n_dst, rh.nx_dst, rh.ny_dst, rh.nnz_per_row, rh.nnz) == (src_m.nCells, n, n, 1, 1, n)
    assert rh.store_stats[2] == n
    gi, gw = rh.weights()
    assert (gi >= 0).all() and (gw == 1.0).all(), "every destination point is mapped"
    assert_nearest_equal(oracle.nearest(cx, pts, brute=True), gi[:, 0], pts, cx, max_ties=2)
    rh.release()


def _identity_fields(torch, n):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(8)
    for dt in (torch.float64, torch.float32):
        for nlev in (1, 55):
            field = (torch.rand((n, nlev), dtype=torch.float64, device="cuda", generator=gen) + 0.5).to(dt)         # no zeros: their sign is
            yield torch.where(torch.rand(field.shape, device="cuda", generator=gen) < 0.5, -field, field), nlev  # the epilogue's, not ours


def test_identity_src_is_dst(dev):
    """The deliberate all-ties case: every point coincides with a corner of its triangles, so with the ray from the centre (the
    default line type) two determinants vanish exactly: one weight exactly 1.0 on the own cell, two exactly 0.0, and regrid_rows
    returns any field bit for bit."""
    import torch
    m = MC.mesh("geo8")
    rh = _store(dev("geo8"), dev("geo8"))
    gi, gw = rh.weights()
    assert (gi[:, 0] >= 0).all(), "every point is mapped"
    own = gi == np.arange(m.nCells)[:, None]
    assert (own.sum(axis=1) == 1).all(), "every point's own cell is one of its three slots"
    assert (gw[own] == 1.0).all() and (gw[~own] == 0.0).all(), "one weight exactly 1.0, two exactly 0.0"
    for field, nlev in _identity_fields(torch, m.nCells):
        assert _bytes_equal(rh.regrid_rows(field, nlev=nlev)[0], field), "regrid_rows returns the field bit for bit"
    rh.release()


def test_identity_src_is_dst_normal_linetype(dev, gpu_lib):
    """The same pair along the triangles' normals.  tri_weights_normal drops P by d = (P - A) . n / n . n; with P ON the corner A that
    is 0 exactly and the weights are exactly (1, 0, 0) again, but with P on corner B or C the dot product of the side B - A (or C - A)
    with the normal n = (B - A) x (C - A) is zero only mathematically: it is off by up to 3 eps |P - A| |n|, the foot by 3 eps |P - A|,
    and a weight by that over the triangle's height -- 3 eps x side / height, 1.2-1.4 on a geodesic mesh -- plus the few eps of the
    determinants themselves.  Bar: 16 eps per weight, and 3 x 16 eps x max|field| for a field taken through regrid_rows."""
    import torch
    eps = np.finfo(np.float64).eps
    m = MC.mesh("geo8")
    gpu_lib.tune("bilinear_linetype", 1)
    try:
        rh = _store(dev("geo8"), dev("geo8"))
    finally:
        gpu_lib.tune("bilinear_linetype", 0)
    gi, gw = rh.weights()
    assert (gi[:, 0] >= 0).all(), "every point is mapped"
    own = gi == np.arange(m.nCells)[:, None]
    assert (own.sum(axis=1) == 1).all(), "every point's own cell is one of its three slots"
    first = own[:, 0]
    assert first.any() and (~first).any()
    assert (gw[first, 0] == 1.0).all() and (gw[first, 1:] == 0.0).all(), "on the triangle's first corner the foot is the point itself"
    print("normal line type: largest |w - (1, 0, 0)| %.3g eps" % (max(np.abs(gw[own] - 1.0).max(), np.abs(gw[~own]).max()) / eps))
    assert np.abs(gw[own] - 1.0).max() <= 16 * eps and np.abs(gw[~own]).max() <= 16 * eps
    for field, nlev in _identity_fields(torch, m.nCells):
        if field.dtype == torch.float64:
            got = rh.regrid_rows(field, nlev=nlev)[0]
            assert float((got - field).abs().max()) <= 48 * eps * float(field.abs().max())
    rh.release()


@pytest.mark.parametrize("name", ["geo10_to_vor1500", "varres3000_to_geo8"])
def test_independent_of_the_source_numbering(gpu_lib, oracle, name):
    """The same pair with the source cells renumbered (shuffled, Morton): same mapped mask, and a smooth field -- the same function of
    position on either numbering -- gives the same value at every destination point within 1e-12."""
    import torch
    from mpassit_amd import regrid as R, synth
    src_m, dst_m, loc = MC.pair(name)
    dst = R.Mesh.from_mpas(dst_m)
    nlev = 3
    vals, masks = [], []
    for variant in (src_m, synth.shuffle_cells(src_m), synth.morton_cells(src_m)):
        src = R.Mesh.from_mpas(variant)
        rh = _store(src, dst, 0, 0, loc)
        field = torch.as_tensor(MC.smooth_field(variant, nlev), device="cuda")
        vals.append(rh.regrid_rows(field, nlev=nlev)[0].cpu().numpy())
        gi, gw = rh.weights()
        masks.append(gi[:, 0] >= 0)
        # this numbering's own oracle answer
        cx = MC.cell_xyz(oracle, variant)
        tri, _ = oracle.dual_triangles(variant.verticesOnCell, variant.nVertices, cx)
        oi, ow = oracle.bilinear_weights(cx, tri, MC.points(oracle, dst_m, loc), 0)
        assert assert_fixed_weights_equal(oi, ow, gi, gw) == 0
        rh.release()
        src.destroy()
    for v, mk in zip(vals[1:], masks[1:]):
        assert np.array_equal(mk, masks[0])
        assert np.abs(v - vals[0]).max() <= 1e-12, np.abs(v - vals[0]).max()
    dst.destroy()


def test_cache(gpu_lib):
    from mpassit_amd import regrid as R
    src, dst = R.Mesh.from_mpas(MC.mesh("geo8")), R.Mesh.from_mpas(MC.mesh("geo10"))
    a = _store(src, dst)
    assert a.store_stats[3] > 0, "the first bilinear Store of a source mesh builds its triangle tree"
    b = _store(src, dst)
    assert a._h.value == b._h.value, "a second Store with the same arguments returns the cached handle"
    gpu_lib.tune("bilinear_linetype", 1)
    try:
        c = _store(src, dst)
    finally:
        gpu_lib.tune("bilinear_linetype", 0)
    assert c._h.value != a._h.value, "the line type is part of a bilinear key"
    assert c.store_stats[3] == 0, "the tree is kept on the mesh"
    n1 = _store(src, dst, R.REGRIDMETHOD_NEAREST_STOD)
    v = _store(src, dst, 0, 0, 1)
    rev = _store(dst, src)
    assert len({a._h.value, c._h.value, n1._h.value, v._h.value, rev._h.value}) == 5
    assert (rev.n_src, rev.n_dst) == (a.n_dst, a.n_src) and v.n_dst == MC.mesh("geo10").nVertices
    for rh in (b, c, n1, v, rev):
        rh.release()
    # a released handle stays parked: the Store again returns it
    addr = a._h.value
    wa = a.weights()
    a.release()
    a = _store(src, dst)
    assert a._h.value == addr
    a.release()
    # destroying EITHER mesh drops the parked entry: a new mesh at whatever address stores anew (same weights, its own tree)
    dst.destroy()
    dst2 = R.Mesh.from_mpas(MC.mesh("geo10"))
    a2 = _store(src, dst2)
    assert a2.store_ms > 0.0 and all(np.array_equal(x, y) for x, y in zip(wa, a2.weights()))
    a2.release()
    src.destroy()
    src2 = R.Mesh.from_mpas(MC.mesh("geo8"))
    a3 = _store(src2, dst2)
    assert a3.store_stats[3] > 0, "a new source mesh builds a tree of its own: nothing of the destroyed one was found"
    assert all(np.array_equal(x, y) for x, y in zip(wa, a3.weights()))
    a3.release()
    src2.destroy()
    dst2.destroy()


def test_source_window(gpu_lib):
    """A window on the SOURCE mesh rebases the handle, and the Regrid from the windowed slab has the bits of the Regrid from the whole
    slab; a window on the destination mesh does not touch it."""
    import torch
    from mpassit_amd import regrid as R
    src_m, dst_m, _ = MC.pair("vor2500_to_hex")
    src, dst = R.Mesh.from_mpas(src_m), R.Mesh.from_mpas(dst_m)
    rh = _store(src, dst)
    first, end = rh.source_range()
    assert 0 < first < end < src_m.nCells, "the region references a band of the global mesh's cells"
    i0, w0 = rh.weights()
    nlev = 5
    field = torch.as_tensor(MC.smooth_field(src_m, nlev), device="cuda")
    whole = rh.regrid_rows(field, nlev=nlev)
    dst.set_source_window(3, dst_m.nCells - 7)
    i1, w1 = rh.weights()
    assert np.array_equal(i0, i1) and np.array_equal(w0, w1), "a window on the destination mesh passes the handle by"
    dst.set_source_window(0, dst_m.nCells)
    src.set_source_window(first, end - first)
    rh._refresh()
    assert rh.n_src == end - first
    i2, w2 = rh.weights()
    assert np.array_equal(np.where(i0 >= 0, i0 - first, -1), i2) and np.array_equal(w0, w2)
    assert rh.source_range() == (first, end), "back in global ids"
    windowed = rh.regrid_rows(field[first:end].contiguous(), nlev=nlev)
    assert _bytes_equal(windowed, whole)
    late = _store(src, dst, R.REGRIDMETHOD_NEAREST_STOD)       # a Store under the window is window-relative from the start
    assert late.n_src == end - first
    late.release()
    src.set_source_window(0, src_m.nCells)
    rh._refresh()
    assert rh.n_src == src_m.nCells and np.array_equal(rh.weights()[0], i0)
    rh.release()
    src.destroy()
    dst.destroy()


def test_refusals(dev, gpu_lib):
    from mpassit_amd import _lib as L, regrid as R, target_grid as tg
    lib = L.load()

    def refused(rc, want, word=None):
        msg = lib.mpg_last_error().decode()
        assert rc == want and msg, (rc, want, msg)
        if word:
            assert word in msg, msg

    h = C.c_void_p()
    a, b = dev("geo8"), dev("geo10")
    refused(L.regrid_store_mesh(a._h, 0, b._h, 0, R.REGRIDMETHOD_CONSERVE, C.byref(h)), L.MPG_ERR_UNSUPPORTED, "conservative")
    assert "mpg_regrid_store_conserve_to_mesh" in lib.mpg_last_error().decode(), "the message names the way out"
    refused(L.regrid_store_mesh(a._h, 1, b._h, 0, 0, C.byref(h)), L.MPG_ERR_UNSUPPORTED, "node-located")
    refused(L.regrid_store_mesh(a._h, 1, b._h, 0, R.REGRIDMETHOD_NEAREST_STOD, C.byref(h)), L.MPG_ERR_UNSUPPORTED, "MPG_MESHLOC_ELEMENT")
    refused(L.regrid_store_mesh(None, 0, b._h, 0, 0, C.byref(h)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(L.regrid_store_mesh(a._h, 0, None, 0, 0, C.byref(h)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(L.regrid_store_mesh(a._h, 0, b._h, 0, 0, None), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(L.regrid_store_mesh(a._h, 2, b._h, 0, 0, C.byref(h)), L.MPG_ERR_INVALID_ARG, "source mesh location")
    refused(L.regrid_store_mesh(a._h, 0, b._h, -1, 0, C.byref(h)), L.MPG_ERR_INVALID_ARG, "destination mesh location")
    refused(L.regrid_store_mesh(a._h, 0, b._h, 0, 3, C.byref(h)), L.MPG_ERR_INVALID_ARG, "method")
    # either mesh cut to a grid's window
    g = tg.define_target_grid_params("lambert", 61, 41, dx=30000.0, dy=30000.0, **MC.LAMBERT)
    grid = R.Grid.from_proj(g, fill_target=False)
    wmesh = R.Mesh.from_mpas(MC.mesh("hex_small"), window_grid=grid)
    refused(L.regrid_store_mesh(wmesh._h, 0, b._h, 0, 0, C.byref(h)), L.MPG_ERR_UNSUPPORTED, "source mesh was cut")
    refused(L.regrid_store_mesh(a._h, 0, wmesh._h, 0, 0, C.byref(h)), L.MPG_ERR_UNSUPPORTED, "destination mesh was cut")
    assert "mpg_mesh_create" in lib.mpg_last_error().decode()
    wmesh.destroy()
    grid.destroy()
    # the Python face raises the library's refusal
    with pytest.raises(L.MpgError) as e:
        R.regrid_store_mesh(a, b, R.REGRIDMETHOD_CONSERVE)
    assert e.value.rc == L.MPG_ERR_UNSUPPORTED


def test_every_consumer_of_a_fixed_handle_takes_it(dev, oracle):
    """typed / masked / transpose / to_mesh Regrids, the getters, unique_sources, localize and rebase on a Mesh -> Mesh handle."""
    import torch
    from mpassit_amd import regrid as R
    src_m, dst_m, _ = MC.pair("hex_to_geo10")
    rh = R.regrid_store_mesh(dev("hex_large"), dev("geo10"))
    gi, gw = rh.weights()
    un = torch.as_tensor(gi[:, 0] < 0, device="cuda")
    assert 0 < int(un.sum()) < rh.n_dst
    nlev = 4
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4)
    cf = torch.rand((nlev, rh.n_src), dtype=torch.float64, device="cuda", generator=gen) + 1.0
    lf = cf.t().contiguous()
    ref = torch.as_tensor(oracle.apply_fixed(gi, gw, cf.cpu().numpy().reshape(-1), nlev), device="cuda")
    typed = rh.regrid_typed(cf.reshape(-1), nlev=nlev).reshape(nlev, -1)
    assert float((typed - ref).abs().max()) <= 1e-13 * 2.0 and (typed[:, un] == 0.0).all()
    assert _bytes_equal(rh.regrid_typed(lf.reshape(-1), nlev=nlev, layout=R.LAYOUT_LEV_FAST).reshape(nlev, -1), typed)
    assert _bytes_equal(rh.regrid_rows(lf, nlev=nlev)[0], typed.t().contiguous())
    assert _bytes_equal(rh.regrid_to_mesh(cf, nlev=nlev, layout=R.LAYOUT_LEV_FAST)[0], typed.t().contiguous())
    masked = rh.regrid_masked(cf.reshape(-1), nlev=nlev, fill_value=float("nan")).reshape(nlev, -1)
    assert torch.isnan(masked[:, un]).all() and torch.equal(masked[:, ~un], typed[:, ~un])
    y = torch.rand((nlev, rh.n_dst), dtype=torch.float64, device="cuda", generator=gen)
    aty = rh.regrid_transpose(y, nlev=nlev).reshape(nlev, -1)
    lhs, rhs = float((typed * y).sum()), float((cf * aty).sum())
    assert abs(lhs - rhs) <= 1e-13 * float(typed.norm() * y.norm())
    ids = rh.unique_sources()
    assert np.array_equal(ids, np.unique(gi[gi >= 0]))
    rh.release()
    solo = R.regrid_store_mesh(dev("hex_large"), dev("geo10"), dst_meshloc=R.MESHLOC_NODE)
    si, _ = solo.weights()
    ids = solo.localize()
    li, _ = solo.weights()
    assert solo.n_src == ids.size and np.array_equal(np.where(si >= 0, ids[np.maximum(li, 0)], -1), si)
    solo.release()
