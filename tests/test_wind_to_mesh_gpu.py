"""The wind chain turned round on the GPU at small sizes (mpg_wind_to_mesh_dev, mpg_mesh_rotang_dev): the fused call held BIT FOR BIT
to the chain it replaces -- two regrid_to_mesh calls into float64, four torch products and two sums, one cast, +0.0 where either handle
leaves a point unmapped -- for every type pair, both layouts and level counts on both sides of the kernel's chunk limit; the sign against
the forward rotation; the angles against their numpy mirror; pitched sources, canaries, graph capture from the first call, refusals, and
the differentiable op by a dot-product test.

The case is that of tests/test_to_mesh_gpu.py: a 60 x 40 Lambert grid built from its projection, a jittered hex mesh that overhangs it
(an unmapped rim, and EDGE1 / EDGE2 rims that differ) and one that lies inside it; neither count is a multiple of the kernel's 64 points."""
import numpy as np
import pytest

from _wind_pair_helpers import _bytes_equal, _pitched, _unmapped, _winds
from conftest import LAMBERT

pytestmark = pytest.mark.gpu

# [cell][lev] results leave through two LDS tiles that share the 64 KB tile cap: all levels in one pair of tiles up to 63 (float64) /
# 127 (float32) levels, level chunks from 64 / 128 on (apply_mesh.h am_tile_plan with two tiles)
CHUNK_EDGE = {"f64": (63, 64), "f32": (127, 128)}


@pytest.fixture(scope="module")
def case(gpu_lib):
    import torch
    from mpassit_amd import regrid as R, synth, target_grid as tg
    g = tg.define_target_grid_params("lambert", 61, 41, dx=30000.0, dy=30000.0, **LAMBERT)
    m_over = synth.regional_mesh_for_lambert(g.proj, 61, 41, 6001, margin=0.05, seed=11)
    m_in = synth.regional_mesh_for_lambert(g.proj, 61, 41, 5003, margin=-0.08, seed=12)
    ga = R.Grid.from_proj(g, fill_target=False)
    d = dict(g=g, ga=ga, m_over=m_over, m_in=m_in, mesh_over=R.Mesh.from_mpas(m_over), mesh_in=R.Mesh.from_mpas(m_in))
    for tag in ("over", "in"):
        mesh = d["mesh_" + tag]
        d["u_" + tag] = R.regrid_store_to_mesh(ga, mesh, staggerloc=R.STAGGERLOC_EDGE1)
        d["v_" + tag] = R.regrid_store_to_mesh(ga, mesh, staggerloc=R.STAGGERLOC_EDGE2)
        d["rot_" + tag] = R.mesh_rotang(ga, mesh)
        d["un_" + tag] = _unmapped(torch, d["u_" + tag], d["v_" + tag])
    yield d
    for k in ("u_over", "v_over", "u_in", "v_in"):
        d[k].release()
    for k in ("mesh_over", "mesh_in", "ga"):
        d[k].destroy()


def _chain(torch, rh_u, rh_v, rot, un, u, v, nlev, ddt):
    """The route the fused call replaces, [lev][cell]: every product and every sum a torch operation of its own (nothing to contract)."""
    a = rh_u.regrid_to_mesh(u, nlev=nlev, out_dtype=torch.float64).reshape(nlev, -1)
    b = rh_v.regrid_to_mesh(v, nlev=nlev, out_dtype=torch.float64).reshape(nlev, -1)
    if rot is not None:
        ca, sa = rot
        t1 = a * ca
        t2 = b * sa
        t3 = a * sa
        t4 = b * ca
        ue = t1 - t2
        ve = t3 + t4
    else:
        ue, ve = a, b
    ue, ve = ue.to(ddt), ve.to(ddt)
    ue[:, un] = 0.0
    ve[:, un] = 0.0
    return ue, ve


def _check_identity(R, rh_u, rh_v, rot, un, nlev, sdt, ddt, seed):
    import torch
    u, v = _winds(torch, rh_u, rh_v, nlev, sdt, seed)
    want_ue, want_ve = _chain(torch, rh_u, rh_v, rot, un, u, v, nlev, ddt)
    ca, sa = rot if rot is not None else (None, None)
    ue, ve = R.wind_to_mesh(rh_u, rh_v, ca, sa, u, v, nlev, layout=R.LAYOUT_CELL_FAST, out_dtype=ddt)
    assert tuple(ue.shape) == (nlev, rh_u.n_dst) and tuple(ve.shape) == (nlev, rh_u.n_dst) and ue.dtype == ddt and ve.dtype == ddt
    assert _bytes_equal(ue, want_ue), "[lev][cell] ue differs from the chain"
    assert _bytes_equal(ve, want_ve), "[lev][cell] ve differs from the chain"
    le, lv = R.wind_to_mesh(rh_u, rh_v, ca, sa, u, v, nlev, layout=R.LAYOUT_LEV_FAST, out_dtype=ddt)
    assert tuple(le.shape) == (rh_u.n_dst, nlev) and tuple(lv.shape) == (rh_u.n_dst, nlev)
    assert _bytes_equal(le, want_ue.t().contiguous()), "[cell][lev] ue is not the transposition of the chain"
    assert _bytes_equal(lv, want_ve.t().contiguous()), "[cell][lev] ve is not the transposition of the chain"
    again = R.wind_to_mesh(rh_u, rh_v, ca, sa, u, v, nlev, layout=R.LAYOUT_LEV_FAST, out_dtype=ddt)
    assert _bytes_equal(again[0], le) and _bytes_equal(again[1], lv), "two calls differ"
    return u, v, ue, ve


def test_masks_exercise_the_either_rule(case):
    """The overhanging mesh has an unmapped rim in both handles and the two rims differ; the inside mesh is mapped everywhere."""
    iu, iv = case["u_over"].weights()[0][:, 0], case["v_over"].weights()[0][:, 0]
    n = case["u_over"].n_dst
    assert n == case["v_over"].n_dst == case["m_over"].nCells and n % 64 != 0 and case["u_in"].n_dst % 64 != 0
    assert (case["u_over"].nnz_per_row, case["v_over"].nnz_per_row) == (4, 4)
    assert 0 < (iu < 0).sum() < n / 2 and 0 < (iv < 0).sum() < n / 2
    assert ((iu < 0) != (iv < 0)).sum() >= 1, "the two unmapped masks are one: the 'either' rule is not exercised"
    assert int(case["un_in"].sum()) == 0


@pytest.mark.parametrize("nlev", [1, 3, 55, 63, 64, 127, 128])
@pytest.mark.parametrize("types", ["f64f64", "f32f32", "f32f64", "f64f32"])
def test_identity_with_the_chain(case, types, nlev):
    import torch
    from mpassit_amd import regrid as R
    dt = {"f64": torch.float64, "f32": torch.float32}
    assert nlev in (1, 3, 55) or nlev in CHUNK_EDGE["f64"] + CHUNK_EDGE["f32"]
    _check_identity(R, case["u_over"], case["v_over"], case["rot_over"], case["un_over"], nlev, dt[types[:3]], dt[types[3:]], 300 + nlev)


@pytest.mark.parametrize("types", ["f64f64", "f32f32", "f64f32"])
def test_no_rotation(case, types):
    """NULL angles: the bytes of the two regrid_to_mesh calls on the points mapped in both handles, +0.0 elsewhere."""
    import torch
    from mpassit_amd import regrid as R
    dt = {"f64": torch.float64, "f32": torch.float32}
    sdt, ddt = dt[types[:3]], dt[types[3:]]
    rh_u, rh_v, un, nlev = case["u_over"], case["v_over"], case["un_over"], 7
    u, v, ue, ve = _check_identity(R, rh_u, rh_v, None, un, nlev, sdt, ddt, 17)
    a = rh_u.regrid_to_mesh(u, nlev=nlev, out_dtype=ddt).reshape(nlev, -1)
    b = rh_v.regrid_to_mesh(v, nlev=nlev, out_dtype=ddt).reshape(nlev, -1)
    assert _bytes_equal(ue[:, ~un], a[:, ~un]) and _bytes_equal(ve[:, ~un], b[:, ~un])
    bits = torch.int64 if ddt == torch.float64 else torch.int32
    assert (ue[:, un].contiguous().view(bits) == 0).all() and (ve[:, un].contiguous().view(bits) == 0).all(), "+0.0 where either is unmapped"
    assert (a[:, un] != 0).any() or (b[:, un] != 0).any(), "some point is mapped in one handle only"


def test_edges_call_with_minus_sina_is_the_cells_call(case):
    """The policies of the one kernel tied together on the cell handles: wind_to_edges with (ca, -sa) and the tangential component is
    wind_to_mesh with (ca, sa) BIT FOR BIT -- un = a ca + b (-sa) is ue = a ca - b sa and ut = b ca - a (-sa) is ve = a sa + b ca, exact in
    IEEE arithmetic (b * (-s) == -(b * s), x + (-y) == x - y, b * c + a * s == a * s + b * c) -- and the normal-only call gives the un of
    the tangential one.  Both layouts, below and in the level chunks of the pair, float32 and float64 sources."""
    import torch
    from mpassit_amd import regrid as R
    rh_u, rh_v, (ca, sa) = case["u_over"], case["v_over"], case["rot_over"]
    msa = -sa
    for sdt in (torch.float32, torch.float64):
        for nlev in (3, 64):
            u, v = _winds(torch, rh_u, rh_v, nlev, sdt, 800 + nlev)
            for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
                ue, ve = R.wind_to_mesh(rh_u, rh_v, ca, sa, u, v, nlev, layout=layout, out_dtype=torch.float32)
                un, ut = R.wind_to_edges(rh_u, rh_v, ca, msa, u, v, nlev, layout=layout, out_dtype=torch.float32, tangential=True)
                assert _bytes_equal(un, ue), "un of (ca, -sa) is not ue (layout %d, %d levels, %s)" % (layout, nlev, sdt)
                assert _bytes_equal(ut, ve), "ut of (ca, -sa) is not ve (layout %d, %d levels, %s)" % (layout, nlev, sdt)
                alone = R.wind_to_edges(rh_u, rh_v, ca, msa, u, v, nlev, layout=layout, out_dtype=torch.float32)
                assert _bytes_equal(alone, un), "un alone is not the un of the pair (layout %d, %d levels, %s)" % (layout, nlev, sdt)
            assert float(ue.abs().max()) > 1 and float(ve.abs().max()) > 1 and not _bytes_equal(ue, ve)


def test_nearest_pair_and_one_handle_twice(case):
    import torch
    from mpassit_amd import regrid as R
    ga, mesh = case["ga"], case["mesh_over"]
    nu = R.regrid_store_to_mesh(ga, mesh, R.REGRIDMETHOD_NEAREST_STOD, staggerloc=R.STAGGERLOC_EDGE1)
    nv = R.regrid_store_to_mesh(ga, mesh, R.REGRIDMETHOD_NEAREST_STOD, staggerloc=R.STAGGERLOC_EDGE2)
    assert (nu.nnz_per_row, nv.nnz_per_row) == (1, 1)
    un = _unmapped(torch, nu, nv)
    for nlev, sdt, ddt in ((1, torch.float64, torch.float64), (9, torch.float32, torch.float32), (64, torch.float64, torch.float32)):
        _check_identity(R, nu, nv, case["rot_over"], un, nlev, sdt, ddt, 50 + nlev)
        _check_identity(R, nu, nv, None, un, nlev, sdt, ddt, 60 + nlev)
    nu.release()
    nv.release()
    rc = R.regrid_store_to_mesh(ga, mesh)                    # winds on mass points: one CENTER handle for both components
    un = _unmapped(torch, rc, rc)
    assert 0 < int(un.sum()) < rc.n_dst / 2
    for nlev, sdt, ddt in ((1, torch.float32, torch.float64), (55, torch.float64, torch.float64), (128, torch.float32, torch.float32)):
        _check_identity(R, rc, rc, case["rot_over"], un, nlev, sdt, ddt, 70 + nlev)
    rc.release()


def test_sign_against_the_forward_rotation(case):
    """Earth winds on the CENTER points, rotate_winds_cgrid with the grid's own angles, then wind_to_mesh through a nearest CENTER handle
    with the grid's angles gathered at the handle's indices: the original winds at those indices, within 8 ulp of max|wind| (a handful of
    rounded operations each way).  The opposite sign would miss by O(0.1) of the wind."""
    import torch
    from mpassit_amd import regrid as R
    ga, g = case["ga"], case["g"]
    rn = R.regrid_store_to_mesh(ga, case["mesh_in"], R.REGRIDMETHOD_NEAREST_STOD)
    idx = torch.as_tensor(rn.weights()[0][:, 0].astype(np.int64), device="cuda")
    assert int(idx.min()) >= 0
    cosa, sina = (torch.as_tensor(np.ascontiguousarray(x), device="cuda") for x in ga.rotang())
    nlev = 5
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4)
    ue0 = torch.randn((nlev, g.ny, g.nx), dtype=torch.float64, device="cuda", generator=gen) * 15.0
    ve0 = torch.randn((nlev, g.ny, g.nx), dtype=torch.float64, device="cuda", generator=gen) * 15.0
    ug, vg = ue0.clone(), ve0.clone()
    R.rotate_winds_cgrid(cosa, sina, ug, vg)
    ca, sa = cosa.reshape(-1)[idx].contiguous(), sina.reshape(-1)[idx].contiguous()
    ue, ve = R.wind_to_mesh(rn, rn, ca, sa, ug, vg, nlev)
    wmax = float(torch.maximum(ue0.abs().max(), ve0.abs().max()))
    tol = 8.0 * float(np.spacing(wmax))
    err = max(float((ue - ue0.reshape(nlev, -1)[:, idx]).abs().max()), float((ve - ve0.reshape(nlev, -1)[:, idx]).abs().max()))
    fu, fv = R.wind_to_mesh(rn, rn, ca, -sa, ug, vg, nlev)
    flipped = max(float((fu - ue0.reshape(nlev, -1)[:, idx]).abs().max()), float((fv - ve0.reshape(nlev, -1)[:, idx]).abs().max()))
    print("round trip: max error %.3g (bound %.3g = 8 ulp of %.3g); with -sina %.3g; max|sina| %.3g" % (err, tol, wmax, flipped, float(sa.abs().max())))
    assert err <= tol
    assert flipped > 0.1, "the check cannot tell the two signs apart"
    rn.release()


def test_mesh_rotang(case, gpu_lib):
    """mpg_mesh_rotang_dev against its numpy mirror at the longitudes of the mesh file, 1e-14 absolute (a few ulp of the longitude through
    atan2 and sin / cos); the refusals."""
    import torch
    from mpassit_amd import _lib as L, regrid as R, target_grid as tg
    g, ga = case["g"], case["ga"]
    for tag in ("over", "in"):
        m, mesh = case["m_" + tag], case["mesh_" + tag]
        for loc, lon in ((R.MESHLOC_ELEMENT, m.lonCell), (R.MESHLOC_NODE, m.lonVertex)):
            cosa, sina = R.mesh_rotang(ga, mesh, loc)
            wc, ws = tg.rotang_at(g.proj, np.degrees(lon))
            assert cosa.dtype == torch.float64 and tuple(cosa.shape) == (lon.size,) and tuple(sina.shape) == (lon.size,)
            dc, ds = np.abs(cosa.cpu().numpy() - wc).max(), np.abs(sina.cpu().numpy() - ws).max()
            print("mesh_%s loc %d: |cosa - mirror| %.3g, |sina - mirror| %.3g, max|sina| %.3g" % (tag, loc, dc, ds, np.abs(ws).max()))
            assert dc <= 1e-14 and ds <= 1e-14
            assert np.abs(ws).max() > 0.05, "the mesh spans longitudes off the standard one: the angles are not all zero"
    lib = L.load()
    out = torch.zeros(2 * case["m_in"].nCells, dtype=torch.float64, device="cuda")
    args = lambda grid, mesh, loc=0: (grid._h, mesh._h, loc, out.data_ptr(), out.data_ptr() + 8 * case["m_in"].nCells, None)   # noqa: E731

    def refused(rc, want, word=None):
        msg = lib.mpg_last_error().decode()
        assert rc == want and msg, (rc, want, msg)
        if word:
            assert word in msg, msg

    gl = R.Grid.from_proj(tg.define_target_grid_params("lat-lon", 81, 61, dx=0.25, dy=0.25, ref_lat=30.0, ref_lon=-110.0, ref_x=1.0, ref_y=1.0,
                                                       stand_lon=-110.0), fill_target=False)
    refused(L.mesh_rotang_dev(*args(gl, case["mesh_in"])), L.MPG_ERR_UNSUPPORTED, "the forward chain does not rotate there: pass NULL angles")
    gl.destroy()
    c = {st: ga.coords(st) for st in range(4)}
    gb = R.Grid(c[0][0], c[0][1], c[3][0], c[3][1], c[1][0], c[1][1], c[2][0], c[2][1])        # the same points, no projection
    refused(L.mesh_rotang_dev(*args(gb, case["mesh_in"])), L.MPG_ERR_UNSUPPORTED, "pass NULL angles")
    wmesh = R.Mesh.from_mpas(case["m_in"], window_grid=gb)
    refused(L.mesh_rotang_dev(*args(ga, wmesh)), L.MPG_ERR_UNSUPPORTED, "window")
    wmesh.destroy()
    gb.destroy()
    refused(L.mesh_rotang_dev(*args(ga, case["mesh_in"], 2)), L.MPG_ERR_INVALID_ARG, "mesh location")
    refused(L.mesh_rotang_dev(None, case["mesh_in"]._h, 0, out.data_ptr(), out.data_ptr(), None), L.MPG_ERR_INVALID_ARG)
    assert L.mesh_rotang_dev(*args(ga, case["mesh_in"])) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_pitched_sources(case, dt):
    """U and V as wind_destagger writes them into plane-pitched results (one level stride for both, so the larger of the two handles'
    strides, in views laid out as empty_pitched lays them out) go into the call as they are: the bytes of the dense call."""
    import torch
    from mpassit_amd import regrid as R
    dt = torch.float64 if dt == "f64" else torch.float32
    ga, g, nlev = case["ga"], case["g"], 6
    gu, gv = R.regrid_store_grid(ga, R.STAGGERLOC_EDGE1), R.regrid_store_grid(ga, R.STAGGERLOC_EDGE2)
    cosa, sina = (torch.as_tensor(np.ascontiguousarray(x), device="cuda") for x in ga.rotang())
    gen = torch.Generator(device="cuda")
    gen.manual_seed(8)
    um = torch.randn((nlev, g.ny, g.nx), dtype=torch.float64, device="cuda", generator=gen) * 10.0
    vm = torch.randn((nlev, g.ny, g.nx), dtype=torch.float64, device="cuda", generator=gen) * 10.0
    ld = max(gu.level_stride(dt), gv.level_stride(dt))
    assert ld > max(gu.n_dst, gv.n_dst)
    _, pu = _pitched(torch, nlev, gu.ny_dst, gu.nx_dst, dt, ld)
    _, pv = _pitched(torch, nlev, gv.ny_dst, gv.nx_dst, dt, ld)
    R.wind_destagger(gu, gv, cosa, sina, um, vm, nlev, out_dtype=dt, outs=(pu, pv))
    assert not pu.is_contiguous() and not pv.is_contiguous() and not torch.isnan(pu).any() and not torch.isnan(pv).any()
    du, dv = pu.contiguous(), pv.contiguous()
    rh_u, rh_v, (ca, sa) = case["u_over"], case["v_over"], case["rot_over"]
    assert (rh_u.n_src, rh_v.n_src) == (gu.n_dst, gv.n_dst)
    for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
        want = R.wind_to_mesh(rh_u, rh_v, ca, sa, du, dv, nlev, layout=layout)
        got = R.wind_to_mesh(rh_u, rh_v, ca, sa, pu, pv, nlev, layout=layout)
        assert _bytes_equal(got[0], want[0]) and _bytes_equal(got[1], want[1]), "pitched sources differ from dense (their NaN pad was read?)"
        assert not torch.isnan(got[0]).any() and not torch.isnan(got[1]).any()
    # a strided view that is not plane-pitched is refused by the wrapper
    with pytest.raises(ValueError):
        R.wind_to_mesh(rh_u, rh_v, ca, sa, du.transpose(1, 2), dv, nlev)
    gu.release()
    gv.release()


def test_canaries(case):
    """Both results sit between NaN-filled bands: the bands stay untouched, in both layouts, with and without level chunks."""
    import torch
    from mpassit_amd import regrid as R
    rh_u, rh_v, (ca, sa) = case["u_over"], case["v_over"], case["rot_over"]
    n, band = rh_u.n_dst, 4096
    for nlev, ddt in ((55, torch.float32), (64, torch.float64), (1, torch.float32)):
        u, v = _winds(torch, rh_u, rh_v, nlev, torch.float32, 90 + nlev)
        for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
            want = R.wind_to_mesh(rh_u, rh_v, ca, sa, u, v, nlev, layout=layout, out_dtype=ddt)
            bufs = [torch.full((2 * band + nlev * n,), float("nan"), dtype=ddt, device="cuda") for _ in range(2)]
            outs = tuple(b[band:band + nlev * n] for b in bufs)
            got = R.wind_to_mesh(rh_u, rh_v, ca, sa, u, v, nlev, layout=layout, outs=outs)
            assert got[0].data_ptr() == outs[0].data_ptr() and got[1].data_ptr() == outs[1].data_ptr()
            for b, w in zip(bufs, want):
                assert torch.isnan(b[:band]).all() and torch.isnan(b[band + nlev * n:]).all(), "a canary band was written"
                assert _bytes_equal(b[band:band + nlev * n], w.reshape(-1))


def test_graph_capture_on_the_first_call(gpu_lib):
    """The very first wind_to_mesh on fresh handles is captured (after mpg_warmup_wait) and replayed twice: the bytes of the eager call."""
    import torch
    from mpassit_amd import regrid as R, synth, target_grid as tg
    g = tg.define_target_grid_params("lambert", 51, 35, dx=30000.0, dy=30000.0, **LAMBERT)
    m = synth.regional_mesh_for_lambert(g.proj, 51, 35, 3001, margin=0.03, seed=21)
    grid, mesh = R.Grid.from_proj(g, fill_target=False), R.Mesh.from_mpas(m)
    rh_u = R.regrid_store_to_mesh(grid, mesh, staggerloc=R.STAGGERLOC_EDGE1)
    rh_v = R.regrid_store_to_mesh(grid, mesh, staggerloc=R.STAGGERLOC_EDGE2)
    ca, sa = R.mesh_rotang(grid, mesh)
    assert gpu_lib.load().mpg_warmup_wait() == 0
    nlev, n = 55, rh_u.n_dst
    u, v = _winds(torch, rh_u, rh_v, nlev, torch.float32, 5)
    lf = tuple(torch.full((n, nlev), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2))
    cf = tuple(torch.full((nlev, n), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):        # one stream: a chain, no parallel branches
            R.wind_to_mesh(rh_u, rh_v, ca, sa, u, v, nlev, layout=R.LAYOUT_LEV_FAST, outs=lf)
            R.wind_to_mesh(rh_u, rh_v, ca, sa, u, v, nlev, layout=R.LAYOUT_CELL_FAST, outs=cf)
    for trial in range(2):
        u.mul_(-0.5).add_(0.25)
        v.mul_(0.75).sub_(1.0)
        graph.replay()
        torch.cuda.synchronize()
        got_lf, got_cf = [t.clone() for t in lf], [t.clone() for t in cf]
        want_lf = R.wind_to_mesh(rh_u, rh_v, ca, sa, u, v, nlev, layout=R.LAYOUT_LEV_FAST)
        want_cf = R.wind_to_mesh(rh_u, rh_v, ca, sa, u, v, nlev, layout=R.LAYOUT_CELL_FAST, out_dtype=torch.float64)
        for got, want in zip(got_lf + got_cf, list(want_lf) + list(want_cf)):
            assert not torch.isnan(got).any() and _bytes_equal(got, want)
    rh_u.release()
    rh_v.release()
    mesh.destroy()
    grid.destroy()


def test_refusals(case, gpu_lib):
    import torch
    from mpassit_amd import _lib as L, regrid as R, target_grid as tg
    lib = L.load()

    def refused(rc, want, word=None):
        msg = lib.mpg_last_error().decode()
        assert rc == want and msg, (rc, want, msg)
        assert "mpg_wind_to_mesh" in msg, msg
        if word:
            assert word in msg, msg

    ga, mesh = case["ga"], case["mesh_in"]
    rh_u, rh_v, (ca, sa) = case["u_in"], case["v_in"], case["rot_in"]
    n = rh_u.n_dst
    src = torch.zeros(4 * max(rh_u.n_src, rh_v.n_src, n), dtype=torch.float64, device="cuda")
    eu = torch.zeros(4 * max(n, rh_u.n_src, rh_v.n_src), dtype=torch.float64, device="cuda")
    ev = torch.zeros_like(eu)

    def args(**kw):
        return [kw.get("hu", rh_u._h), kw.get("hv", rh_v._h), kw.get("ca", ca.data_ptr()), kw.get("sa", sa.data_ptr()), kw.get("u", src.data_ptr()),
                kw.get("v", src.data_ptr()), kw.get("st", 0), kw.get("ldu", 0), kw.get("ldv", 0), kw.get("nlev", 2), kw.get("ue", eu.data_ptr()),
                kw.get("ve", ev.data_ptr()), kw.get("dt", 0), kw.get("layout", 1), None]

    call = L.wind_to_mesh_dev
    # MPG_ERR_UNSUPPORTED: the handle kinds and the big-endian types
    rcsr = R.regrid_store_conserve_to_mesh(ga, mesh)
    assert rcsr.nnz_per_row == 0 and rcsr.n_dst == n
    refused(call(*args(hu=rcsr._h)), L.MPG_ERR_UNSUPPORTED, "CSR")
    refused(call(*args(hv=rcsr._h)), L.MPG_ERR_UNSUPPORTED, "CSR")
    rcsr.release()
    gp = R.Grid.from_target(tg.define_target_grid_params("lat-lon", nx=73, ny=37, stand_lon=0.0, is_regional=False))
    rp = R.regrid_store_grid(gp, R.STAGGERLOC_EDGE2)
    assert rp.pole()[0].size > 0 and rp.n_src <= src.numel() // 2 and rp.n_dst <= eu.numel() // 2
    refused(call(*args(hu=rp._h, hv=rp._h, ca=None, sa=None)), L.MPG_ERR_UNSUPPORTED, "pole")
    rp.release()
    gp.destroy()
    near = R.regrid_store_to_mesh(ga, mesh, R.REGRIDMETHOD_NEAREST_STOD, staggerloc=R.STAGGERLOC_EDGE2)
    refused(call(*args(hv=near._h)), L.MPG_ERR_UNSUPPORTED, "slots")
    near.release()
    r3 = R.regrid_store(mesh, ga)                       # Mesh -> Grid: 3 slots
    assert r3.nnz_per_row == 3 and r3.n_src <= src.numel() // 2 and r3.n_dst <= eu.numel() // 2
    refused(call(*args(hu=r3._h, hv=r3._h, ca=None, sa=None)), L.MPG_ERR_UNSUPPORTED, "slots")
    r3.release()
    refused(call(*args(st=2)), L.MPG_ERR_UNSUPPORTED, "big-endian")
    refused(call(*args(dt=3)), L.MPG_ERR_UNSUPPORTED, "big-endian")
    # MPG_ERR_INVALID_ARG
    rvert = R.regrid_store_to_mesh(ga, mesh, staggerloc=R.STAGGERLOC_EDGE2, meshloc=R.MESHLOC_NODE)
    assert rvert.n_dst != n
    refused(call(*args(hv=rvert._h)), L.MPG_ERR_INVALID_ARG, "same points")
    rvert.release()
    refused(call(*args(ca=None)), L.MPG_ERR_INVALID_ARG, "cosa and sina")
    refused(call(*args(sa=None)), L.MPG_ERR_INVALID_ARG, "cosa and sina")
    refused(call(*args(ldu=rh_u.n_src - 1)), L.MPG_ERR_INVALID_ARG, "u_level_stride")
    refused(call(*args(ldv=rh_v.n_src - 1)), L.MPG_ERR_INVALID_ARG, "v_level_stride")
    refused(call(*args(nlev=0)), L.MPG_ERR_INVALID_ARG, "nlev")
    refused(call(*args(layout=2)), L.MPG_ERR_INVALID_ARG, "dst_layout")
    refused(call(*args(st=4)), L.MPG_ERR_INVALID_ARG)
    refused(call(*args(hu=None)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(call(*args(hv=None)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(call(*args(u=None)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(call(*args(ve=None)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(call(*args(ve=eu.data_ptr())), L.MPG_ERR_INVALID_ARG, "alias")
    refused(call(*args(ue=src.data_ptr())), L.MPG_ERR_INVALID_ARG, "alias")
    ang = torch.zeros_like(eu)          # angles in a block of their own, large enough that a result laid over it touches nothing else
    a0, a1 = ang.data_ptr(), ang.data_ptr() + 8 * n
    refused(call(*args(ca=a0, sa=a1, ue=a0)), L.MPG_ERR_INVALID_ARG, "angles")
    refused(call(*args(ca=a0, sa=a1, ve=a1)), L.MPG_ERR_INVALID_ARG, "angles")
    # ... and the same arguments without a fault are accepted, dense and at the smallest and a larger stride
    assert call(*args()) == 0 and call(*args(ldu=rh_u.n_src, ldv=rh_v.n_src + 5)) == 0 and call(*args(ca=None, sa=None)) == 0
    torch.cuda.synchronize()
    # the wrapper's own checks
    u, v = _winds(torch, rh_u, rh_v, 2, torch.float64, 1)
    with pytest.raises(ValueError):
        R.wind_to_mesh(rh_u, rh_v, ca, None, u, v, 2)
    with pytest.raises(ValueError):
        R.wind_to_mesh(rh_u, rh_v, ca, sa, u, v.float(), 2)
    with pytest.raises(ValueError):
        R.wind_to_mesh(rh_u, rh_v, ca, sa, u[:1], v, 2)
    with pytest.raises(ValueError):
        R.wind_to_mesh(rh_u, rh_v, ca[:-1], sa[:-1], u, v, 2)


@pytest.mark.parametrize("rotated", [True, False])
@pytest.mark.parametrize("layout", ["cell_fast", "lev_fast"])
@pytest.mark.parametrize("tag", ["in", "over"])
def test_autograd_dot_product(case, tag, layout, rotated):
    """Float64 dot-product test: |<F(u, v), y> - <(u, v), F^T y>| <= 1e-11 * sum |terms| (n * eps accumulation for n ~ 3e5 terms); the
    gradients have the inputs' dtypes and shapes.  On the inside mesh every point is mapped; on the overhanging mesh some points are
    mapped in one handle only (test_masks_exercise_the_either_rule), where the forward stores +0.0 and the backward must pass nothing."""
    import torch
    from mpassit_amd import regrid as R
    layout = R.LAYOUT_CELL_FAST if layout == "cell_fast" else R.LAYOUT_LEV_FAST
    rh_u, rh_v = case["u_" + tag], case["v_" + tag]
    ca, sa = case["rot_" + tag] if rotated else (None, None)
    nlev, g = 3, case["g"]
    u0, v0 = _winds(torch, rh_u, rh_v, nlev, torch.float64, 23)
    u = u0.reshape(nlev, g.ny, g.nx + 1).clone().requires_grad_(True)
    v = v0.reshape(nlev, g.ny + 1, g.nx).clone().requires_grad_(True)
    ue, ve = R.wind_to_mesh_autograd(rh_u, rh_v, ca, sa, u, v, nlev, layout=layout)
    want = R.wind_to_mesh(rh_u, rh_v, ca, sa, u0, v0, nlev, layout=layout)
    assert _bytes_equal(ue.detach(), want[0]) and _bytes_equal(ve.detach(), want[1])
    gen = torch.Generator(device="cuda")
    gen.manual_seed(29)
    ye = torch.randn(tuple(ue.shape), dtype=torch.float64, device="cuda", generator=gen)
    yv = torch.randn(tuple(ve.shape), dtype=torch.float64, device="cuda", generator=gen)
    lhs_terms = torch.cat([(ue.detach() * ye).reshape(-1), (ve.detach() * yv).reshape(-1)])
    ((ue * ye).sum() + (ve * yv).sum()).backward()
    assert u.grad.dtype == u.dtype and v.grad.dtype == v.dtype and u.grad.shape == u.shape and v.grad.shape == v.shape
    rhs_terms = torch.cat([(u.detach() * u.grad).reshape(-1), (v.detach() * v.grad).reshape(-1)])
    lhs, rhs = float(lhs_terms.sum()), float(rhs_terms.sum())
    bound = 1e-11 * float(lhs_terms.abs().sum())
    print("dot-product test: lhs %.17g rhs %.17g |diff| %.3g bound %.3g" % (lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound
    assert float(u.grad.abs().max()) > 0 and float(v.grad.abs().max()) > 0


def test_autograd_float32_and_one_handle_twice(case):
    """float32 inputs get float32 gradients; with one handle for both components the two transposes stay separate gradients."""
    import torch
    from mpassit_amd import regrid as R
    rc = R.regrid_store_to_mesh(case["ga"], case["mesh_in"])
    ca, sa = case["rot_in"]
    nlev = 2
    u0, v0 = _winds(torch, rc, rc, nlev, torch.float32, 31)
    u, v = u0.clone().requires_grad_(True), v0.clone().requires_grad_(True)
    ue, ve = R.wind_to_mesh_autograd(rc, rc, ca, sa, u, v, nlev, layout=R.LAYOUT_LEV_FAST)
    assert ue.dtype == torch.float32 and tuple(ue.shape) == (rc.n_dst, nlev)
    ye, yv = torch.ones_like(ue), torch.zeros_like(ve)
    ((ue * ye).sum() + (ve * yv).sum()).backward()
    assert u.grad.dtype == torch.float32 and v.grad.dtype == torch.float32 and u.grad.shape == u.shape and v.grad.shape == v.shape
    # d(sum ue)/du = A^T ca, d(sum ue)/dv = -A^T sa: two different fields from one handle
    one = torch.ones((nlev, rc.n_dst), dtype=torch.float64, device="cuda")
    want_u = rc.regrid_transpose((one * ca).float(), nlev=nlev, out_dtype=torch.float32).reshape(u.shape)
    want_v = rc.regrid_transpose((-(one * sa)).float(), nlev=nlev, out_dtype=torch.float32).reshape(v.shape)
    assert torch.allclose(u.grad, want_u, rtol=1e-6, atol=1e-6) and torch.allclose(v.grad, want_v, rtol=1e-6, atol=1e-6)
    assert not torch.equal(u.grad, v.grad)
    rc.release()
