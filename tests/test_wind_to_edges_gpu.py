"""Winds onto mesh edges on the GPU at small sizes (mpg_mesh_set_edges, the MESHLOC_EDGE Store, mpg_mesh_edge_rotang_dev,
mpg_wind_to_edges_dev): the Store onto edges held byte for byte to the Stores onto cells and vertices at the same points; the angles
against their numpy mirror; the fused call held BIT FOR BIT to the chain it replaces -- two regrid_to_mesh calls into float64, the torch
products and sums, one cast, +0.0 where either handle leaves a point unmapped -- for every type pair, both layouts, with and without the
tangential component and level counts on both sides of the kernel's chunk limits; agreement with wind_to_mesh followed by the
projection; the sign; pitched sources, canaries, graph capture from the first call, refusals, and the differentiable op.

The case is that of tests/test_wind_to_mesh_gpu.py: a 60 x 40 Lambert grid at 30 km, a jittered hex mesh that overhangs it (an
unmapped rim, and EDGE1 / EDGE2 rims that differ) and one that lies inside it, with the edges synth.mesh_edges derives (about 18 k and
15 k); neither count is a multiple of the kernel's 64 points."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from _wind_pair_helpers import _bytes_equal, _pitched, _unmapped, _winds
from conftest import LAMBERT

pytestmark = pytest.mark.gpu

# [edge][lev] results leave through ONE LDS tile of at most 64 KB with an odd row stride when only un is asked (apply_mesh.h am_tile_plan:
# all levels in the tile up to 127 float64 / 255 float32 levels, level chunks beyond), through TWO tiles of half the cap each with ut
# (am_tile_plan with two tiles: 63 / 127)
SINGLE_EDGE = {"f64": (127, 128, 129), "f32": (255, 256, 257)}
PAIR_EDGE = {"f64": (63, 64), "f32": (127, 128)}


def _with_edges(synth, m):
    m = synth.mesh_edges(m)
    if m.nEdges % 64 == 0:      # keep a partial last block of 64 points
        m = dataclasses.replace(m, latEdge=m.latEdge[:-1], lonEdge=m.lonEdge[:-1], angleEdge=m.angleEdge[:-1], cellsOnEdge=m.cellsOnEdge[:-1])
    assert m.nEdges % 64 != 0
    return m


@pytest.fixture(scope="module")
def case(gpu_lib):
    import torch
    from mpassit_amd import regrid as R, synth, target_grid as tg
    g = tg.define_target_grid_params("lambert", 61, 41, dx=30000.0, dy=30000.0, **LAMBERT)
    m_over = _with_edges(synth, synth.regional_mesh_for_lambert(g.proj, 61, 41, 6001, margin=0.05, seed=11))
    m_in = _with_edges(synth, synth.regional_mesh_for_lambert(g.proj, 61, 41, 5003, margin=-0.08, seed=12))
    ga = R.Grid.from_proj(g, fill_target=False)
    d = dict(g=g, ga=ga, m_over=m_over, m_in=m_in, mesh_over=R.Mesh.from_mpas(m_over), mesh_in=R.Mesh.from_mpas(m_in))
    for tag in ("over", "in"):
        mesh = d["mesh_" + tag]
        assert mesh.nEdges == d["m_" + tag].nEdges > 2.9 * mesh.nCells
        d["u_" + tag] = R.regrid_store_to_mesh(ga, mesh, staggerloc=R.STAGGERLOC_EDGE1, meshloc=R.MESHLOC_EDGE)
        d["v_" + tag] = R.regrid_store_to_mesh(ga, mesh, staggerloc=R.STAGGERLOC_EDGE2, meshloc=R.MESHLOC_EDGE)
        d["rot_" + tag] = R.mesh_edge_rotang(ga, mesh)
        d["un_" + tag] = _unmapped(torch, d["u_" + tag], d["v_" + tag])
    yield d
    for k in ("u_over", "v_over", "u_in", "v_in"):
        d[k].release()
    for k in ("mesh_over", "mesh_in", "ga"):
        d[k].destroy()


def _chain(torch, rh_u, rh_v, rot, un, u, v, nlev, ddt):
    """The route the fused call replaces, [lev][edge]: every product and every sum a torch operation of its own (nothing to contract)."""
    a = rh_u.regrid_to_mesh(u, nlev=nlev, out_dtype=torch.float64).reshape(nlev, -1)
    b = rh_v.regrid_to_mesh(v, nlev=nlev, out_dtype=torch.float64).reshape(nlev, -1)
    cn, sn = rot
    t1 = a * cn
    t2 = b * sn
    wn = t1 + t2
    t3 = b * cn
    t4 = a * sn
    wt = t3 - t4
    wn, wt = wn.to(ddt), wt.to(ddt)
    wn[:, un] = 0.0
    wt[:, un] = 0.0
    return wn, wt


def _check_identity(R, rh_u, rh_v, rot, un, nlev, sdt, ddt, seed, tangential=(False, True)):
    import torch
    u, v = _winds(torch, rh_u, rh_v, nlev, sdt, seed)
    want_n, want_t = _chain(torch, rh_u, rh_v, rot, un, u, v, nlev, ddt)
    cn, sn = rot
    n = rh_u.n_dst
    for tan in tangential:
        got = R.wind_to_edges(rh_u, rh_v, cn, sn, u, v, nlev, layout=R.LAYOUT_CELL_FAST, out_dtype=ddt, tangential=tan)
        got = got if tan else (got,)
        want = (want_n, want_t) if tan else (want_n,)
        assert len(got) == len(want)
        for x, w, name in zip(got, want, ("un", "ut")):
            assert tuple(x.shape) == (nlev, n) and x.dtype == ddt
            assert _bytes_equal(x, w), "[lev][edge] %s differs from the chain (tangential=%s)" % (name, tan)
        lf = R.wind_to_edges(rh_u, rh_v, cn, sn, u, v, nlev, layout=R.LAYOUT_LEV_FAST, out_dtype=ddt, tangential=tan)
        lf = lf if tan else (lf,)
        for x, w, name in zip(lf, want, ("un", "ut")):
            assert tuple(x.shape) == (n, nlev)
            assert _bytes_equal(x, w.t().contiguous()), "[edge][lev] %s is not the transposition of the chain (tangential=%s)" % (name, tan)
        again = R.wind_to_edges(rh_u, rh_v, cn, sn, u, v, nlev, layout=R.LAYOUT_LEV_FAST, out_dtype=ddt, tangential=tan)
        again = again if tan else (again,)
        assert all(_bytes_equal(x, y) for x, y in zip(again, lf)), "two calls differ"
    return u, v


# ---- the Store onto edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("boxes", [1, 0])
def test_store_onto_edges_is_the_store_onto_the_same_points(case, gpu_lib, boxes):
    """Edges given the CELL coordinates get the MESHLOC_ELEMENT handle's indices and weights byte for byte, edges given the vertex
    coordinates the MESHLOC_NODE handle's: bilinear and nearest, EDGE1 and CENTER, both candidate routes (fresh objects: nothing from
    the handle cache)."""
    from mpassit_amd import regrid as R
    m = case["m_over"]
    ga = R.Grid.from_proj(case["g"], fill_target=False)
    gpu_lib.tune("store_boxes", boxes)
    try:
        for lat, lon, loc in ((m.latCell, m.lonCell, R.MESHLOC_ELEMENT), (m.latVertex, m.lonVertex, R.MESHLOC_NODE)):
            mesh = R.Mesh(m.latCell, m.lonCell, m.latVertex, m.lonVertex, m.verticesOnCell)
            assert mesh.nEdges == 0
            mesh.set_edges(lat, lon)
            assert mesh.nEdges == lat.size
            for method in (R.REGRIDMETHOD_BILINEAR, R.REGRIDMETHOD_NEAREST_STOD):
                for st in (R.STAGGERLOC_EDGE1, R.STAGGERLOC_CENTER):
                    re_ = R.regrid_store_to_mesh(ga, mesh, method, staggerloc=st, meshloc=R.MESHLOC_EDGE)
                    rp = R.regrid_store_to_mesh(ga, mesh, method, staggerloc=st, meshloc=loc)
                    assert re_._h.value != rp._h.value, "two handles: the cache key carries the location"
                    assert re_.store_path == rp.store_path == boxes
                    assert (re_.n_dst, re_.nx_dst, re_.ny_dst, re_.nnz_per_row) == (lat.size, lat.size, 1, rp.nnz_per_row)
                    (ie, we), (ip, wp) = re_.weights(), rp.weights()
                    assert ie.tobytes() == ip.tobytes() and we.tobytes() == wp.tobytes(), (loc, method, st)
                    if method == R.REGRIDMETHOD_BILINEAR:
                        assert 0 < (ie[:, 0] < 0).sum() < lat.size / 2
                    re_.release()
                    rp.release()
            mesh.destroy()
    finally:
        gpu_lib.tune("store_boxes", 1)
    ga.destroy()


def test_masks_exercise_the_either_rule(case):
    """With the real edges the overhanging mesh has an unmapped rim in both handles and the two rims differ; the inside mesh is mapped
    everywhere."""
    iu, iv = case["u_over"].weights()[0][:, 0], case["v_over"].weights()[0][:, 0]
    n = case["u_over"].n_dst
    assert n == case["v_over"].n_dst == case["m_over"].nEdges and n % 64 != 0 and case["u_in"].n_dst % 64 != 0
    assert (case["u_over"].nnz_per_row, case["v_over"].nnz_per_row) == (4, 4)
    assert 0 < (iu < 0).sum() < n / 2 and 0 < (iv < 0).sum() < n / 2
    assert ((iu < 0) != (iv < 0)).sum() >= 1, "the two unmapped masks are one: the 'either' rule is not exercised"
    assert int(case["un_in"].sum()) == 0


def test_edges_refusals(case, gpu_lib):
    from mpassit_amd import _lib as L, regrid as R
    lib = L.load()

    def refused(rc, want, *words):
        msg = lib.mpg_last_error().decode()
        assert rc == want and msg, (rc, want, msg)
        for w in words:
            assert w in msg, msg

    m, ga = case["m_in"], case["ga"]
    mesh = R.Mesh(m.latCell, m.lonCell, m.latVertex, m.lonVertex, m.verticesOnCell)
    n = C.c_int64(-1)
    assert L.mesh_edge_count(mesh._h, C.byref(n)) == 0 and n.value == 0
    h = C.c_void_p()
    refused(L.regrid_store_to_mesh(ga._h, 0, mesh._h, 2, 0, C.byref(h)), L.MPG_ERR_INVALID_ARG, "mesh location", "mpg_mesh_set_edges")
    refused(L.regrid_store_to_mesh(ga._h, 0, mesh._h, 3, 0, C.byref(h)), L.MPG_ERR_INVALID_ARG, "mesh location")
    refused(L.regrid_store_to_mesh(ga._h, 0, mesh._h, -1, 0, C.byref(h)), L.MPG_ERR_INVALID_ARG, "mesh location")
    lat, lon, ang = (np.ascontiguousarray(x[:1000], dtype=np.float64) for x in (m.latEdge, m.lonEdge, m.angleEdge))
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    refused(L.mesh_set_edges(None, 1000, p(lat), p(lon), p(ang)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(L.mesh_set_edges(mesh._h, 0, p(lat), p(lon), p(ang)), L.MPG_ERR_INVALID_ARG, "nEdges")
    refused(L.mesh_set_edges(mesh._h, 1000, None, p(lon), p(ang)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(L.mesh_set_edges(mesh._h, 1000, p(lat), None, p(ang)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(L.mesh_set_edges(mesh._h, 2 ** 31, p(lat), p(lon), p(ang)), L.MPG_ERR_OVERFLOW, "int32")
    for arr, i, bad in ((lat, 17, np.nan), (lon, 555, np.inf), (ang, 999, np.nan), (lat, 3, 1.6)):
        keep = arr[i]
        arr[i] = bad
        refused(L.mesh_set_edges(mesh._h, 1000, p(lat), p(lon), p(ang)), L.MPG_ERR_INVALID_ARG, " %d " % i)
        arr[i] = keep
    assert L.mesh_edge_count(mesh._h, C.byref(n)) == 0 and n.value == 0, "a refused call leaves the mesh without edges"
    # edges without angles: the Store works, the angles are refused
    assert L.mesh_set_edges(mesh._h, 1000, p(lat), p(lon), None) == 0
    assert L.mesh_edge_count(mesh._h, C.byref(n)) == 0 and n.value == 1000
    refused(L.mesh_set_edges(mesh._h, 1000, p(lat), p(lon), p(ang)), L.MPG_ERR_INVALID_ARG, "edges are already set")
    assert L.regrid_store_to_mesh(ga._h, 0, mesh._h, 2, 0, C.byref(h)) == 0
    assert lib.mpg_handle_release(h) == 0
    # edges are a destination only: every call that takes a source location goes on refusing location 2
    refused(lib.mpg_regrid_store(mesh._h, C.c_int(2), ga._h, C.c_int(0), C.c_int(0), C.byref(h)), L.MPG_ERR_INVALID_ARG, "mesh location")
    refused(lib.mpg_mesh_set_source_window(mesh._h, C.c_int(2), C.c_int64(0), C.c_int64(10)), L.MPG_ERR_INVALID_ARG)
    refused(L.regrid_store_mesh(mesh._h, 0, mesh._h, 2, 0, C.byref(h)), L.MPG_ERR_INVALID_ARG, "mesh location")
    mesh.destroy()
    wmesh = R.Mesh(m.latCell, m.lonCell, m.latVertex, m.lonVertex, m.verticesOnCell, window_grid=ga)
    refused(L.mesh_set_edges(wmesh._h, 1000, p(lat), p(lon), p(ang)), L.MPG_ERR_UNSUPPORTED, "window")
    wmesh.destroy()
    with pytest.raises(ValueError):
        case["mesh_in"].set_edges(lat, lon[:-1])
    with pytest.raises(L.MpgError):
        case["mesh_in"].set_edges(lat, lon, ang)        # a second call through the wrapper
    assert case["mesh_in"].nEdges == m.nEdges


# ---- the angles ---------------------------------------------------------------------------------------------------------------------
def test_mesh_edge_rotang(case, gpu_lib):
    """mpg_mesh_edge_rotang_dev against its numpy mirror at the longitudes of the mesh file, 1e-14 absolute (test_mesh_rotang's bound: a
    few ulp of the longitude through atan2, the rounding of phi, |phi| <= 2 pi, and sin / cos); a NULL grid; the refusals."""
    import torch
    from mpassit_amd import _lib as L, regrid as R, target_grid as tg
    g, ga = case["g"], case["ga"]
    for tag in ("over", "in"):
        m, mesh = case["m_" + tag], case["mesh_" + tag]
        lon = np.degrees(m.lonEdge)
        for grid, proj in ((ga, g.proj), (None, None)):
            cn, sn = R.mesh_edge_rotang(grid, mesh)
            wc, ws = tg.edge_rotang_at(proj, lon, m.angleEdge)
            assert cn.dtype == torch.float64 and tuple(cn.shape) == (m.nEdges,) and tuple(sn.shape) == (m.nEdges,)
            dc, ds = np.abs(cn.cpu().numpy() - wc).max(), np.abs(sn.cpu().numpy() - ws).max()
            print("mesh_%s grid %s: |cn - mirror| %.3g, |sn - mirror| %.3g" % (tag, "None" if grid is None else "Lambert", dc, ds))
            assert dc <= 1e-14 and ds <= 1e-14
            if grid is None:
                assert np.abs(cn.cpu().numpy() - np.cos(m.angleEdge)).max() <= 1e-14 and np.abs(sn.cpu().numpy() - np.sin(m.angleEdge)).max() <= 1e-14
        assert np.abs(tg.rotang_at(g.proj, lon)[1]).max() > 0.05, "the mesh spans longitudes off the standard one: alpha matters"
    lib = L.load()
    ne = case["m_in"].nEdges
    out = torch.zeros(2 * ne, dtype=torch.float64, device="cuda")
    args = lambda grid, mesh: (grid._h if grid is not None else None, mesh._h, out.data_ptr(), out.data_ptr() + 8 * ne, None)   # noqa: E731

    def refused(rc, want, word=None):
        msg = lib.mpg_last_error().decode()
        assert rc == want and msg, (rc, want, msg)
        assert "mpg_mesh_edge_rotang" in msg, msg
        if word:
            assert word in msg, msg

    gl = R.Grid.from_proj(tg.define_target_grid_params("lat-lon", 81, 61, dx=0.25, dy=0.25, ref_lat=30.0, ref_lon=-110.0, ref_x=1.0, ref_y=1.0,
                                                       stand_lon=-110.0), fill_target=False)
    refused(L.mesh_edge_rotang_dev(*args(gl, case["mesh_in"])), L.MPG_ERR_UNSUPPORTED, "the forward chain does not rotate there: pass a NULL grid")
    gl.destroy()
    c = {st: ga.coords(st) for st in range(4)}
    gb = R.Grid(c[0][0], c[0][1], c[3][0], c[3][1], c[1][0], c[1][1], c[2][0], c[2][1])        # the same points, no projection
    refused(L.mesh_edge_rotang_dev(*args(gb, case["mesh_in"])), L.MPG_ERR_UNSUPPORTED, "the forward chain does not rotate there: pass a NULL grid")
    gb.destroy()
    m = case["m_in"]
    bare = R.Mesh(m.latCell, m.lonCell, m.latVertex, m.lonVertex, m.verticesOnCell)
    refused(L.mesh_edge_rotang_dev(*args(ga, bare)), L.MPG_ERR_INVALID_ARG, "mpg_mesh_set_edges")
    with pytest.raises(L.MpgError):
        R.mesh_edge_rotang(ga, bare)
    bare.set_edges(m.latEdge, m.lonEdge)
    refused(L.mesh_edge_rotang_dev(*args(ga, bare)), L.MPG_ERR_INVALID_ARG, "mpg_mesh_set_edges")
    refused(L.mesh_edge_rotang_dev(*args(None, bare)), L.MPG_ERR_INVALID_ARG, "angleEdge")
    bare.destroy()
    refused(L.mesh_edge_rotang_dev(ga._h, None, out.data_ptr(), out.data_ptr(), None), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(L.mesh_edge_rotang_dev(ga._h, case["mesh_in"]._h, None, out.data_ptr(), None), L.MPG_ERR_INVALID_ARG, "NULL")
    assert L.mesh_edge_rotang_dev(*args(ga, case["mesh_in"])) == 0 and L.mesh_edge_rotang_dev(*args(None, case["mesh_in"])) == 0
    torch.cuda.synchronize()
    # mpg_mesh_rotang_dev goes on refusing location 2
    assert L.mesh_rotang_dev(ga._h, case["mesh_in"]._h, 2, out.data_ptr(), out.data_ptr() + 8 * ne, None) == L.MPG_ERR_INVALID_ARG
    assert "mesh location" in lib.mpg_last_error().decode()


# ---- identity with the chain --------------------------------------------------------------------------------------------------------
DT = {"f64": "float64", "f32": "float32"}


@pytest.mark.parametrize("nlev", [1, 3, 55])
@pytest.mark.parametrize("types", ["f64f64", "f32f32", "f32f64", "f64f32"])
def test_identity_with_the_chain(case, types, nlev):
    import torch
    from mpassit_amd import regrid as R
    sdt, ddt = getattr(torch, DT[types[:3]]), getattr(torch, DT[types[3:]])
    _check_identity(R, case["u_over"], case["v_over"], case["rot_over"], case["un_over"], nlev, sdt, ddt, 300 + nlev)


@pytest.mark.parametrize("types", ["f64f64", "f32f32", "f32f64", "f64f32"])
def test_identity_at_the_chunk_edges(case, types):
    """On both sides of the single tile's limit with un alone, of the pair's limit with ut (SINGLE_EDGE / PAIR_EDGE of the result type)."""
    import torch
    from mpassit_amd import regrid as R
    sdt, ddt = getattr(torch, DT[types[:3]]), getattr(torch, DT[types[3:]])
    assert set(SINGLE_EDGE["f64"]) >= {128, 129} and set(SINGLE_EDGE["f32"]) >= {256, 257}
    for nlev in SINGLE_EDGE[types[3:]]:
        _check_identity(R, case["u_over"], case["v_over"], case["rot_over"], case["un_over"], nlev, sdt, ddt, 400 + nlev, tangential=(False,))
    for nlev in PAIR_EDGE[types[3:]]:
        _check_identity(R, case["u_over"], case["v_over"], case["rot_over"], case["un_over"], nlev, sdt, ddt, 500 + nlev, tangential=(True,))


def test_nearest_pair_and_one_handle_twice(case):
    import torch
    from mpassit_amd import regrid as R
    ga, mesh = case["ga"], case["mesh_over"]
    nu = R.regrid_store_to_mesh(ga, mesh, R.REGRIDMETHOD_NEAREST_STOD, staggerloc=R.STAGGERLOC_EDGE1, meshloc=R.MESHLOC_EDGE)
    nv = R.regrid_store_to_mesh(ga, mesh, R.REGRIDMETHOD_NEAREST_STOD, staggerloc=R.STAGGERLOC_EDGE2, meshloc=R.MESHLOC_EDGE)
    assert (nu.nnz_per_row, nv.nnz_per_row) == (1, 1)
    un = _unmapped(torch, nu, nv)
    for nlev, sdt, ddt in ((1, torch.float64, torch.float64), (9, torch.float32, torch.float32), (64, torch.float64, torch.float32),
                           (129, torch.float32, torch.float64)):
        _check_identity(R, nu, nv, case["rot_over"], un, nlev, sdt, ddt, 50 + nlev)
    nu.release()
    nv.release()
    rc = R.regrid_store_to_mesh(ga, mesh, meshloc=R.MESHLOC_EDGE)      # winds on mass points: one CENTER handle for both components
    un = _unmapped(torch, rc, rc)
    assert 0 < int(un.sum()) < rc.n_dst / 2
    for nlev, sdt, ddt in ((1, torch.float32, torch.float64), (55, torch.float64, torch.float64), (128, torch.float32, torch.float32)):
        _check_identity(R, rc, rc, case["rot_over"], un, nlev, sdt, ddt, 70 + nlev)
    rc.release()


def test_agreement_with_the_long_way_round(case):
    """wind_to_mesh on the same edge handles with cos / sin of alpha at the edges (rotang_at, uploaded), then ue cos(theta) + ve
    sin(theta) in torch, against the fused un in float64: within 64 eps (|a| + |b|) per point -- both routes are about ten rounded
    operations on terms of at most |a| + |b|, plus the rounding of phi, at most 2 pi eps relative."""
    import torch
    from mpassit_amd import regrid as R, target_grid as tg
    nlev = 5
    eps = float(np.finfo(np.float64).eps)
    for tag in ("over", "in"):
        rh_u, rh_v, (cn, sn), m = case["u_" + tag], case["v_" + tag], case["rot_" + tag], case["m_" + tag]
        ca, sa = (torch.as_tensor(x, device="cuda") for x in tg.rotang_at(case["g"].proj, np.degrees(m.lonEdge)))
        ct, st = (torch.as_tensor(f(m.angleEdge), device="cuda") for f in (np.cos, np.sin))
        u, v = _winds(torch, rh_u, rh_v, nlev, torch.float64, 611)
        ue, ve = R.wind_to_mesh(rh_u, rh_v, ca, sa, u, v, nlev)
        long_n, long_t = ue * ct + ve * st, ve * ct - ue * st
        un_, ut_ = R.wind_to_edges(rh_u, rh_v, cn, sn, u, v, nlev, tangential=True)
        a = rh_u.regrid_to_mesh(u, nlev=nlev, out_dtype=torch.float64).reshape(nlev, -1)
        b = rh_v.regrid_to_mesh(v, nlev=nlev, out_dtype=torch.float64).reshape(nlev, -1)
        mapped = ~case["un_" + tag]
        scale = (a.abs() + b.abs())[:, mapped]
        assert float(scale.min()) > 0
        rn = float(((un_ - long_n).abs()[:, mapped] / scale).max()) / eps
        rt = float(((ut_ - long_t).abs()[:, mapped] / scale).max()) / eps
        print("mesh_%s: max |fused - long way| / (eps (|a| + |b|)): un %.3g, ut %.3g (bound 64)" % (tag, rn, rt))
        assert rn <= 64 and rt <= 64
        assert float(un_.abs().max()) > 1 and bool((un_[:, ~mapped] == 0).all()) and bool((long_n[:, ~mapped] == 0).all())


def test_sign(case):
    """A uniform earth wind of 10 m/s eastward, turned grid-relative at the CENTER points with the grid's own angles (u_g = u_e ca + v_e sa,
    v_g = v_e ca - u_e sa), goes through one CENTER handle twice onto the edges of the inside mesh: un = 10 cos(angleEdge), ut =
    -10 sin(angleEdge) within 1e-3 m/s (bilinear interpolation of cos / sin(alpha) over one 30-km cell errs by at most
    10 (cone dlambda)^2 / 4, about 2e-4).  With -sn the miss exceeds 1."""
    import torch
    from mpassit_amd import regrid as R
    ga, g, m = case["ga"], case["g"], case["m_in"]
    rc = R.regrid_store_to_mesh(ga, case["mesh_in"], meshloc=R.MESHLOC_EDGE)
    assert int((rc.weights()[0][:, 0] < 0).sum()) == 0
    cosa, sina = (torch.as_tensor(np.ascontiguousarray(x), device="cuda").reshape(1, -1) for x in ga.rotang())
    ug, vg = (10.0 * cosa).contiguous(), (-10.0 * sina).contiguous()
    cn, sn = case["rot_in"]
    un, ut = R.wind_to_edges(rc, rc, cn, sn, ug, vg, 1, tangential=True)
    theta = torch.as_tensor(m.angleEdge, device="cuda")
    en = float((un.reshape(-1) - 10.0 * torch.cos(theta)).abs().max())
    et = float((ut.reshape(-1) + 10.0 * torch.sin(theta)).abs().max())
    flipped = R.wind_to_edges(rc, rc, cn, -sn, ug, vg, 1)
    ef = float((flipped.reshape(-1) - 10.0 * torch.cos(theta)).abs().max())
    print("uniform eastward wind: max |un - 10 cos(angleEdge)| %.3g, |ut + 10 sin(angleEdge)| %.3g m/s (bound 1e-3); with -sn %.3g" % (en, et, ef))
    assert en <= 1e-3 and et <= 1e-3
    assert ef > 1.0, "the check cannot tell the two signs apart"
    rc.release()


# ---- sources, bands, capture --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_pitched_sources(case, dt):
    """U and V in plane-pitched views whose pad is NaN go into the call as they are: the bytes of the dense call, and no NaN."""
    import torch
    from mpassit_amd import regrid as R
    dt = torch.float64 if dt == "f64" else torch.float32
    g, nlev = case["g"], 6
    rh_u, rh_v, (cn, sn) = case["u_over"], case["v_over"], case["rot_over"]
    du, dv = _winds(torch, rh_u, rh_v, nlev, dt, 8)
    ld = max(rh_u.n_src, rh_v.n_src) + 37
    _, pu = _pitched(torch, nlev, g.ny, g.nx + 1, dt, ld)
    _, pv = _pitched(torch, nlev, g.ny + 1, g.nx, dt, ld)
    pu.copy_(du.reshape(pu.shape))
    pv.copy_(dv.reshape(pv.shape))
    assert not pu.is_contiguous() and not pv.is_contiguous()
    for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
        for tan in (False, True):
            want = R.wind_to_edges(rh_u, rh_v, cn, sn, du, dv, nlev, layout=layout, tangential=tan)
            got = R.wind_to_edges(rh_u, rh_v, cn, sn, pu, pv, nlev, layout=layout, tangential=tan)
            want, got = (want, got) if tan else ((want,), (got,))
            for x, w in zip(got, want):
                assert _bytes_equal(x, w), "pitched sources differ from dense (their NaN pad was read?)"
                assert not torch.isnan(x).any()
    with pytest.raises(ValueError):     # a strided view that is not plane-pitched is refused by the wrapper
        R.wind_to_edges(rh_u, rh_v, cn, sn, pu.transpose(1, 2), pv, nlev)


def test_canaries(case):
    """Every result sits between NaN-filled bands: the bands stay untouched, in both layouts, with and without level chunks, for un
    alone and the pair."""
    import torch
    from mpassit_amd import regrid as R
    rh_u, rh_v, (cn, sn) = case["u_over"], case["v_over"], case["rot_over"]
    n, band = rh_u.n_dst, 4096
    for nlev, ddt in ((55, torch.float32), (64, torch.float64), (129, torch.float64), (1, torch.float32)):
        u, v = _winds(torch, rh_u, rh_v, nlev, torch.float32, 90 + nlev)
        for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
            for tan in (False, True):
                want = R.wind_to_edges(rh_u, rh_v, cn, sn, u, v, nlev, layout=layout, out_dtype=ddt, tangential=tan)
                want = want if tan else (want,)
                bufs = [torch.full((2 * band + nlev * n,), float("nan"), dtype=ddt, device="cuda") for _ in want]
                outs = tuple(b[band:band + nlev * n] for b in bufs)
                got = R.wind_to_edges(rh_u, rh_v, cn, sn, u, v, nlev, layout=layout, tangential=tan, outs=outs if tan else outs[0])
                got = got if tan else (got,)
                for x, o, b, w in zip(got, outs, bufs, want):
                    assert x.data_ptr() == o.data_ptr()
                    assert torch.isnan(b[:band]).all() and torch.isnan(b[band + nlev * n:]).all(), "a canary band was written"
                    assert _bytes_equal(b[band:band + nlev * n], w.reshape(-1))


def test_graph_capture_on_the_first_call(gpu_lib):
    """The very first wind_to_edges on fresh handles is captured (after mpg_warmup_wait) and replayed twice: the bytes of the eager call."""
    import torch
    from mpassit_amd import regrid as R, synth, target_grid as tg
    g = tg.define_target_grid_params("lambert", 51, 35, dx=30000.0, dy=30000.0, **LAMBERT)
    m = _with_edges(synth, synth.regional_mesh_for_lambert(g.proj, 51, 35, 3001, margin=0.03, seed=21))
    grid, mesh = R.Grid.from_proj(g, fill_target=False), R.Mesh.from_mpas(m)
    rh_u = R.regrid_store_to_mesh(grid, mesh, staggerloc=R.STAGGERLOC_EDGE1, meshloc=R.MESHLOC_EDGE)
    rh_v = R.regrid_store_to_mesh(grid, mesh, staggerloc=R.STAGGERLOC_EDGE2, meshloc=R.MESHLOC_EDGE)
    cn, sn = R.mesh_edge_rotang(grid, mesh)
    assert gpu_lib.load().mpg_warmup_wait() == 0
    nlev, n = 55, rh_u.n_dst
    u, v = _winds(torch, rh_u, rh_v, nlev, torch.float32, 5)
    lf = torch.full((n, nlev), float("nan"), dtype=torch.float32, device="cuda")
    cf = tuple(torch.full((nlev, n), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):        # one stream: a chain, no parallel branches
            R.wind_to_edges(rh_u, rh_v, cn, sn, u, v, nlev, layout=R.LAYOUT_LEV_FAST, outs=lf)
            R.wind_to_edges(rh_u, rh_v, cn, sn, u, v, nlev, layout=R.LAYOUT_CELL_FAST, tangential=True, outs=cf)
    for trial in range(2):
        u.mul_(-0.5).add_(0.25)
        v.mul_(0.75).sub_(1.0)
        graph.replay()
        torch.cuda.synchronize()
        got = [lf.clone()] + [t.clone() for t in cf]
        want_lf = R.wind_to_edges(rh_u, rh_v, cn, sn, u, v, nlev, layout=R.LAYOUT_LEV_FAST)
        want_cf = R.wind_to_edges(rh_u, rh_v, cn, sn, u, v, nlev, layout=R.LAYOUT_CELL_FAST, out_dtype=torch.float64, tangential=True)
        for x, w in zip(got, [want_lf] + list(want_cf)):
            assert not torch.isnan(x).any() and _bytes_equal(x, w)
    rh_u.release()
    rh_v.release()
    mesh.destroy()
    grid.destroy()


# ---- refusals of the apply ----------------------------------------------------------------------------------------------------------
def test_refusals(case, gpu_lib):
    import torch
    from mpassit_amd import _lib as L, regrid as R, target_grid as tg
    lib = L.load()

    def refused(rc, want, word=None):
        msg = lib.mpg_last_error().decode()
        assert rc == want and msg, (rc, want, msg)
        assert "mpg_wind_to_edges" in msg, msg
        if word:
            assert word in msg, msg

    ga, mesh = case["ga"], case["mesh_in"]
    rh_u, rh_v, (cn, sn) = case["u_in"], case["v_in"], case["rot_in"]
    n = rh_u.n_dst
    src = torch.zeros(4 * max(rh_u.n_src, rh_v.n_src, n), dtype=torch.float64, device="cuda")
    en = torch.zeros(4 * max(n, rh_u.n_src, rh_v.n_src), dtype=torch.float64, device="cuda")
    et = torch.zeros_like(en)

    def args(**kw):
        return [kw.get("hu", rh_u._h), kw.get("hv", rh_v._h), kw.get("cn", cn.data_ptr()), kw.get("sn", sn.data_ptr()), kw.get("u", src.data_ptr()),
                kw.get("v", src.data_ptr()), kw.get("st", 0), kw.get("ldu", 0), kw.get("ldv", 0), kw.get("nlev", 2), kw.get("un", en.data_ptr()),
                kw.get("ut", et.data_ptr()), kw.get("dt", 0), kw.get("layout", 1), None]

    call = L.wind_to_edges_dev
    # MPG_ERR_UNSUPPORTED: the handle kinds and the big-endian types
    rcsr = R.regrid_store_conserve_to_mesh(ga, mesh)
    ang = torch.zeros(max(n, rcsr.n_dst), dtype=torch.float64, device="cuda")
    assert rcsr.nnz_per_row == 0
    refused(call(*args(hu=rcsr._h)), L.MPG_ERR_UNSUPPORTED, "CSR")
    refused(call(*args(hv=rcsr._h)), L.MPG_ERR_UNSUPPORTED, "CSR")
    rcsr.release()
    gp = R.Grid.from_target(tg.define_target_grid_params("lat-lon", nx=73, ny=37, stand_lon=0.0, is_regional=False))
    rp = R.regrid_store_grid(gp, R.STAGGERLOC_EDGE2)
    assert rp.pole()[0].size > 0 and rp.n_src <= src.numel() // 2 and rp.n_dst <= min(en.numel() // 2, ang.numel())
    refused(call(*args(hu=rp._h, hv=rp._h, cn=ang.data_ptr(), sn=ang.data_ptr())), L.MPG_ERR_UNSUPPORTED, "pole")
    rp.release()
    gp.destroy()
    near = R.regrid_store_to_mesh(ga, mesh, R.REGRIDMETHOD_NEAREST_STOD, staggerloc=R.STAGGERLOC_EDGE2, meshloc=R.MESHLOC_EDGE)
    refused(call(*args(hv=near._h)), L.MPG_ERR_UNSUPPORTED, "slots")
    near.release()
    r3 = R.regrid_store(mesh, ga)                       # Mesh -> Grid: 3 slots
    assert r3.nnz_per_row == 3 and r3.n_src <= src.numel() // 2 and r3.n_dst <= min(en.numel() // 2, ang.numel())
    refused(call(*args(hu=r3._h, hv=r3._h, cn=ang.data_ptr(), sn=ang.data_ptr())), L.MPG_ERR_UNSUPPORTED, "slots")
    r3.release()
    refused(call(*args(st=2)), L.MPG_ERR_UNSUPPORTED, "big-endian")
    refused(call(*args(dt=3)), L.MPG_ERR_UNSUPPORTED, "big-endian")
    # MPG_ERR_INVALID_ARG
    rcell = R.regrid_store_to_mesh(ga, mesh, staggerloc=R.STAGGERLOC_EDGE2)
    assert rcell.n_dst != n
    refused(call(*args(hv=rcell._h)), L.MPG_ERR_INVALID_ARG, "same points")
    rcell.release()
    refused(call(*args(cn=None)), L.MPG_ERR_INVALID_ARG, "NULL")        # the angles are required
    refused(call(*args(sn=None)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(call(*args(cn=None, sn=None)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(call(*args(ldu=rh_u.n_src - 1)), L.MPG_ERR_INVALID_ARG, "u_level_stride")
    refused(call(*args(ldv=rh_v.n_src - 1)), L.MPG_ERR_INVALID_ARG, "v_level_stride")
    refused(call(*args(nlev=0)), L.MPG_ERR_INVALID_ARG, "nlev")
    refused(call(*args(layout=2)), L.MPG_ERR_INVALID_ARG, "dst_layout")
    refused(call(*args(st=4)), L.MPG_ERR_INVALID_ARG)
    refused(call(*args(hu=None)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(call(*args(hv=None)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(call(*args(u=None)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(call(*args(un=None)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(call(*args(ut=en.data_ptr())), L.MPG_ERR_INVALID_ARG, "alias")
    refused(call(*args(ut=en.data_ptr() + 8)), L.MPG_ERR_INVALID_ARG, "un_dev and ut_dev")
    refused(call(*args(un=src.data_ptr())), L.MPG_ERR_INVALID_ARG, "alias")
    refused(call(*args(ut=src.data_ptr())), L.MPG_ERR_INVALID_ARG, "alias")
    big = torch.zeros_like(en)          # angles in a block of their own, large enough that a result laid over it touches nothing else
    a0, a1 = big.data_ptr(), big.data_ptr() + 8 * n
    refused(call(*args(cn=a0, sn=a1, un=a0)), L.MPG_ERR_INVALID_ARG, "angles")
    refused(call(*args(cn=a0, sn=a1, ut=a1)), L.MPG_ERR_INVALID_ARG, "angles")
    # ... and the same arguments without a fault are accepted: dense and strided, with and without ut, one handle twice
    assert call(*args()) == 0 and call(*args(ldu=rh_u.n_src, ldv=rh_v.n_src + 5)) == 0 and call(*args(ut=None)) == 0
    assert call(*args(hv=rh_u._h)) == 0
    torch.cuda.synchronize()
    # the wrapper's own checks
    u, v = _winds(torch, rh_u, rh_v, 2, torch.float64, 1)
    with pytest.raises(ValueError):
        R.wind_to_edges(rh_u, rh_v, cn, None, u, v, 2)
    with pytest.raises(ValueError):
        R.wind_to_edges(rh_u, rh_v, cn, sn, u, v.float(), 2)
    with pytest.raises(ValueError):
        R.wind_to_edges(rh_u, rh_v, cn, sn, u[:1], v, 2)
    with pytest.raises(ValueError):
        R.wind_to_edges(rh_u, rh_v, cn[:-1], sn[:-1], u, v, 2)
    with pytest.raises(ValueError):
        R.wind_to_edges(rh_u, rh_v, cn, sn, u, v, 2, outs=(torch.empty(2 * n, dtype=torch.float64, device="cuda"),) * 2)


# ---- the differentiable op ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tangential", [False, True])
@pytest.mark.parametrize("layout", ["cell_fast", "lev_fast"])
@pytest.mark.parametrize("tag", ["in", "over"])
def test_autograd_dot_product(case, tag, layout, tangential):
    """Float64 dot-product test: |<F(u, v), y> - <(u, v), F^T y>| <= 1e-11 * sum |terms| (n * eps accumulation for n ~ 3e5 terms); the
    gradients have the inputs' dtypes and shapes.  On the inside mesh every point is mapped; on the overhanging mesh some points are
    mapped in one handle only, where the forward stores +0.0 and the backward must pass nothing."""
    import torch
    from mpassit_amd import regrid as R
    layout = R.LAYOUT_CELL_FAST if layout == "cell_fast" else R.LAYOUT_LEV_FAST
    rh_u, rh_v, (cn, sn) = case["u_" + tag], case["v_" + tag], case["rot_" + tag]
    nlev, g = 3, case["g"]
    u0, v0 = _winds(torch, rh_u, rh_v, nlev, torch.float64, 23)
    u = u0.reshape(nlev, g.ny, g.nx + 1).clone().requires_grad_(True)
    v = v0.reshape(nlev, g.ny + 1, g.nx).clone().requires_grad_(True)
    out = R.wind_to_edges_autograd(rh_u, rh_v, cn, sn, u, v, nlev, layout=layout, tangential=tangential)
    want = R.wind_to_edges(rh_u, rh_v, cn, sn, u0, v0, nlev, layout=layout, tangential=tangential)
    out, want = (out, want) if tangential else ((out,), (want,))
    assert all(_bytes_equal(x.detach(), w) for x, w in zip(out, want))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(29)
    ys = [torch.randn(tuple(x.shape), dtype=torch.float64, device="cuda", generator=gen) for x in out]
    lhs_terms = torch.cat([(x.detach() * y).reshape(-1) for x, y in zip(out, ys)])
    sum((x * y).sum() for x, y in zip(out, ys)).backward()
    assert u.grad.dtype == u.dtype and v.grad.dtype == v.dtype and u.grad.shape == u.shape and v.grad.shape == v.shape
    rhs_terms = torch.cat([(u.detach() * u.grad).reshape(-1), (v.detach() * v.grad).reshape(-1)])
    lhs, rhs = float(lhs_terms.sum()), float(rhs_terms.sum())
    bound = 1e-11 * float(lhs_terms.abs().sum())
    print("dot-product test: lhs %.17g rhs %.17g |diff| %.3g bound %.3g" % (lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound
    assert float(u.grad.abs().max()) > 0 and float(v.grad.abs().max()) > 0


def test_autograd_float32_and_points_mapped_in_one_handle(case):
    """float32 inputs get float32 gradients; an incoming gradient that is non-zero only on points mapped in ONE handle passes nothing."""
    import torch
    from mpassit_amd import regrid as R
    rh_u, rh_v, (cn, sn) = case["u_over"], case["v_over"], case["rot_over"]
    nlev = 2
    u0, v0 = _winds(torch, rh_u, rh_v, nlev, torch.float32, 31)
    u, v = u0.clone().requires_grad_(True), v0.clone().requires_grad_(True)
    un, ut = R.wind_to_edges_autograd(rh_u, rh_v, cn, sn, u, v, nlev, layout=R.LAYOUT_LEV_FAST, tangential=True)
    assert un.dtype == torch.float32 and tuple(un.shape) == (rh_u.n_dst, nlev) and tuple(ut.shape) == (rh_u.n_dst, nlev)
    mu = torch.as_tensor(rh_u.weights()[0][:, 0] >= 0, device="cuda")
    mv = torch.as_tensor(rh_v.weights()[0][:, 0] >= 0, device="cuda")
    one_only = mu ^ mv
    assert int(one_only.sum()) >= 1
    y = torch.zeros_like(un)
    y[one_only] = 1.0
    ((un * y).sum() + (ut * y).sum()).backward()
    assert u.grad.dtype == torch.float32 and v.grad.dtype == torch.float32 and u.grad.shape == u.shape and v.grad.shape == v.shape
    assert float(u.grad.abs().max()) == 0.0 and float(v.grad.abs().max()) == 0.0, "a point mapped in one handle only passed a gradient"
    # ... and a gradient on the points mapped in both arrives: d(sum un)/du = A_u^T cn, d(sum un)/dv = A_v^T sn
    u.grad = None
    v.grad = None
    un = R.wind_to_edges_autograd(rh_u, rh_v, cn, sn, u, v, nlev)
    un.sum().backward()
    both = (mu & mv).to(torch.float64)
    want_u = rh_u.regrid_transpose((both * cn).float().expand(nlev, -1).contiguous(), nlev=nlev, out_dtype=torch.float32).reshape(u.shape)
    want_v = rh_v.regrid_transpose((both * sn).float().expand(nlev, -1).contiguous(), nlev=nlev, out_dtype=torch.float32).reshape(v.shape)
    assert torch.allclose(u.grad, want_u, rtol=1e-6, atol=1e-6) and torch.allclose(v.grad, want_v, rtol=1e-6, atol=1e-6)
    assert float(u.grad.abs().max()) > 0
