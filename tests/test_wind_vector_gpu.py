"""The Cartesian-vector wind Regrid on the GPU at small sizes (mpg_sphere_frames_dev, mpg_wind_vector_weights_dev, mpg_wind_vector_dev):
the frames against the numpy mirror, the blocks BIT FOR BIT against numpy, the apply BIT FOR BIT against the chain it replaces -- four
regrid_csr_to_mesh calls of from-weights handles with the values m[k] into float64, one torch add per result, one cast -- for every type
pair, both layouts, one result and two, level counts on both sides of the kernel's tile thresholds and runs longer than its LDS chunk;
empty rows, pitched sources, canaries, graph capture from the first call, refusals, a handle without entries, the differentiable op,
and the solid-body rotation, which is a wind on the cap rows.

Handles (those of tests/test_wind_csr_gpu.py):
  P        periodic 24 x 12 ALLAVG onto the 20 000 cells of the global mesh (no multiple of 64; cap rows of 24 entries)
  E        periodic 72 x 36 ALLAVG onto its 59 994 edges
  E_none   24 x 12 NONE onto the edges: 505 empty rows
  coarse   conservative, the 61 x 41 Lambert grid onto its coarse mesh: 64-row runs longer than the kernel's LDS chunk
  over_d   conservative onto the overhanging mesh: empty rows"""
import numpy as np
import pytest

from _wind_pair_helpers import _bytes_equal, _pitched, _winds
from _wind_vector_helpers import CAP_ROWS, solid_body_case, solid_body_errors
from conftest import LAMBERT

pytestmark = pytest.mark.gpu

LDS_CHUNK = 384              # entries of a 64-row run the kernel keeps in LDS (k_wind_vector.hip WV_CHUNK)
# [point][lev] results leave through ONE LDS tile of at most 64 KB (r0 alone: all levels in the tile up to 127 float64 / 255 float32
# levels) or TWO of half the cap each (63 / 127), in level chunks beyond (apply_mesh.h am_tile_plan)
CHUNK_LEVELS = (63, 64, 65, 127, 128, 129, 257)
DT = {"f64": "float64", "f32": "float32"}
HANDLES = ("P", "E", "E_none", "coarse", "over_d")


def _random_frames(torch, R, n, seed):
    """frames of n random points turned by random angles: no block is zero by symmetry"""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    lon = (torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) * 2.0 - 1.0) * np.pi
    lat = (torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) - 0.5) * np.pi
    phi = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) * (2.0 * np.pi)
    return R.sphere_frames(lon, lat, torch.cos(phi), torch.sin(phi))


@pytest.fixture(scope="module")
def case(gpu_lib, global_mesh):
    import torch
    from mpassit_amd import _lib as L, regrid as R, synth, target_grid as tg
    m = synth.mesh_edges(global_mesh)
    d = dict(m=m, mesh=R.Mesh.from_mpas(m), tg={}, grid={})
    for name, (nxn, nyn) in (("72x36", (73, 37)), ("24x12", (25, 13))):
        g = tg.define_target_grid_params("lat-lon", nx=nxn, ny=nyn, stand_lon=0.0, is_regional=False)
        d["tg"][name], d["grid"][name] = g, R.Grid(g.lon, g.lat, periodic=L.GRID_PERIODIC_I)
    mesh = d["mesh"]
    d["P"] = R.regrid_store_periodic_to_mesh(d["grid"]["24x12"], mesh)
    d["E"] = R.regrid_store_periodic_to_mesh(d["grid"]["72x36"], mesh, meshloc=R.MESHLOC_EDGE)
    d["E_none"] = R.regrid_store_periodic_to_mesh(d["grid"]["24x12"], mesh, meshloc=R.MESHLOC_EDGE, pole_method=R.POLEMETHOD_NONE)
    gl = tg.define_target_grid_params("lambert", 61, 41, dx=30000.0, dy=30000.0, **LAMBERT)
    d["ga"] = R.Grid.from_proj(gl, fill_target=False)
    d["m_coarse"] = synth.regional_mesh_for_lambert(gl.proj, 61, 41, 201, margin=0.05, seed=13)
    d["m_over"] = synth.regional_mesh_for_lambert(gl.proj, 61, 41, 6001, margin=0.05, seed=11)
    d["mesh_coarse"], d["mesh_over"] = R.Mesh.from_mpas(d["m_coarse"]), R.Mesh.from_mpas(d["m_over"])
    d["coarse"] = R.regrid_store_conserve_to_mesh(d["ga"], d["mesh_coarse"], R.NORM_DSTAREA)
    d["over_d"] = R.regrid_store_conserve_to_mesh(d["ga"], d["mesh_over"], R.NORM_DSTAREA)
    # random frames, the blocks and the chain's four from-weights handles of every handle, once
    d["sf"], d["df"], d["blocks"], d["A"], d["csr"] = {}, {}, {}, {}, {}
    for i, k in enumerate(HANDLES):
        rh = d[k]
        assert rh.nnz_per_row == 0 and rh.pole()[0].size == 0
        d["sf"][k], d["df"][k] = _random_frames(torch, R, rh.n_src, 100 + i), _random_frames(torch, R, rh.n_dst, 200 + i)
        d["blocks"][k] = R.wind_vector_weights(rh, d["sf"][k], d["df"][k])
        rowptr, col, val = d["csr"][k] = rh.csr()
        row = np.repeat(np.arange(1, rh.n_dst + 1, dtype=np.int32), np.diff(rowptr))
        mh = d["blocks"][k].cpu().numpy()
        d["A"][k] = [R.RouteHandle.from_weights(rh.n_src, rh.n_dst, 1, row, (col + 1).astype(np.int32), mh[j]) for j in range(4)]
    yield d
    for k in HANDLES:
        for a in d["A"][k]:
            a.release()
        d[k].release()
    for k in ("mesh", "mesh_coarse", "mesh_over", "ga"):
        d[k].destroy()
    for grid in d["grid"].values():
        grid.destroy()


def test_the_handles_exercise_what_they_should(case):
    rp = case["csr"]["P"][0]
    assert case["P"].n_dst == 20000 and case["P"].n_dst % 64 != 0 and set(np.unique(np.diff(rp))) == {4, 24}
    assert case["E"].n_dst == case["E_none"].n_dst == 59994 and set(np.unique(np.diff(case["csr"]["E"][0]))) == {4, 72}
    assert int((np.diff(case["csr"]["E_none"][0]) == 0).sum()) == 505
    rp = case["csr"]["coarse"][0]
    run = rp[np.minimum(np.arange(0, rp.size - 1, 64) + 64, rp.size - 1)] - rp[np.arange(0, rp.size - 1, 64)]
    print("coarse mesh: %d cells, longest row %d entries, longest 64-row run %d" % (case["coarse"].n_dst, np.diff(rp).max(), run.max()))
    assert case["coarse"].n_dst < 300 and run.max() > 1024 > LDS_CHUNK, "the coarse mesh exercises the run chunking"
    assert case["over_d"].n_dst % 64 != 0 and (np.diff(case["csr"]["over_d"][0]) == 0).sum() > 10, "the overhanging mesh has empty rows"


# ---- frames and blocks ------------------------------------------------------------------------------------------------------------------
def test_frames_against_the_mirror(case):
    """1e-14 absolute: the project's bar for device sin / cos against a numpy mirror (test_mesh_edge_rotang)."""
    import torch
    from mpassit_amd import regrid as R, target_grid as tg
    m = case["m"]
    g = case["tg"]["24x12"]
    rng = np.random.default_rng(3)
    phi = rng.uniform(0.0, 2.0 * np.pi, m.nEdges)
    for lon, lat, c, s in ((m.lonEdge, m.latEdge, np.cos(m.angleEdge), np.sin(m.angleEdge)), (m.lonEdge, m.latEdge, np.cos(phi), np.sin(phi)),
                           (m.lonCell, m.latCell, None, None), (np.radians(g.lon).reshape(-1), np.radians(g.lat).reshape(-1), None, None),
                           (np.array([0.0, np.pi, -np.pi, 0.5, 0.0]), np.array([np.pi / 2, -np.pi / 2, 0.0, 0.0, 0.0]), None, None)):
        got = R.sphere_frames(lon, lat, c, s)
        want = tg.sphere_frames_at(lon, lat, c, s)
        assert tuple(got.shape) == want.shape == (6, np.size(lon)) and got.dtype == torch.float64 and got.is_cuda
        err = np.abs(got.cpu().numpy() - want).max()
        print("frames of %d points%s: |GPU - mirror| %.3g" % (np.size(lon), "" if c is None else " turned", err))
        assert err <= 1e-14
    # tensors go in as they are
    lon, lat = torch.as_tensor(m.lonCell, device="cuda"), torch.as_tensor(m.latCell, device="cuda")
    assert _bytes_equal(R.sphere_frames(lon, lat), R.sphere_frames(m.lonCell, m.latCell))
    with pytest.raises(ValueError):
        R.sphere_frames(lon, lat, lon, None)
    with pytest.raises(ValueError):
        R.sphere_frames(lon, lat[:-1])


@pytest.mark.parametrize("name", HANDLES)
def test_blocks_bit_for_bit(case, name):
    """The blocks of the DOWNLOADED frames and rh.csr(), computed in numpy (every operation rounded, nothing contracted): the same bits."""
    from mpassit_amd import target_grid as tg
    rowptr, col, val = case["csr"][name]
    want = tg.wind_vector_blocks(rowptr, col, val, case["sf"][name].cpu().numpy(), case["df"][name].cpu().numpy())
    got = case["blocks"][name].cpu().numpy()
    assert got.shape == want.shape == (4, case[name].nnz)
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), "%d of %d blocks differ" % ((got != want).sum(), got.size)
    assert (got != 0.0).all(), "random frames leave no block zero"


# ---- identity with the chain --------------------------------------------------------------------------------------------------------
def test_the_chain_handles_hold_the_blocks(case):
    for name in HANDLES:
        rowptr, col, _ = case["csr"][name]
        mh = case["blocks"][name].cpu().numpy()
        for j, a in enumerate(case["A"][name]):
            rp, c, v = a.csr()
            assert a.nnz_per_row == 0 and np.array_equal(rp, rowptr) and np.array_equal(c, col)
            assert np.array_equal(v.view(np.int64), mh[j].view(np.int64)), "the from-weights handle does not hold m[%d] as given" % j


def _chain(torch, A, u, v, nlev, ddt, second):
    """The route the fused call replaces, [lev][point]: four Regrids into float64 (scale 1, offset 0), ONE add per result, ONE cast."""
    t = [A[j].regrid_csr_to_mesh(u if j % 2 == 0 else v, nlev=nlev, out_dtype=torch.float64).reshape(nlev, -1) for j in range(4 if second else 2)]
    outs = [t[0] + t[1]] + ([t[2] + t[3]] if second else [])
    return [x.to(ddt) for x in outs]


def _fused(R, rh, m, u, v, nlev, layout, ddt=None, second=True, outs=None):
    got = R.wind_vector(rh, m, u, v, nlev, layout=layout, out_dtype=ddt, second=second, outs=outs)
    return list(got) if second else [got]


def _check_identity(R, case, name, nlev, sdt, ddt, second, seed):
    import torch
    rh, m = case[name], case["blocks"][name]
    u, v = _winds(torch, rh, rh, nlev, sdt, seed)
    want = _chain(torch, case["A"][name], u, v, nlev, ddt, second)
    n = rh.n_dst
    got = _fused(R, rh, m, u, v, nlev, R.LAYOUT_CELL_FAST, ddt, second)
    assert len(got) == len(want) == (2 if second else 1)
    for i, (x, w) in enumerate(zip(got, want)):
        assert tuple(x.shape) == (nlev, n) and x.dtype == ddt
        assert _bytes_equal(x, w), "[lev][point] result %d differs from the chain (%s, nlev %d)" % (i, name, nlev)
    lf = _fused(R, rh, m, u, v, nlev, R.LAYOUT_LEV_FAST, ddt, second)
    for i, (x, w) in enumerate(zip(lf, want)):
        assert tuple(x.shape) == (n, nlev)
        assert _bytes_equal(x, w.t().contiguous()), "[point][lev] result %d is not the transposition of the chain (%s, nlev %d)" % (i, name, nlev)
    again = _fused(R, rh, m, u, v, nlev, R.LAYOUT_LEV_FAST, ddt, second)
    assert all(_bytes_equal(x, y) for x, y in zip(again, lf)), "two calls differ"


@pytest.mark.parametrize("nlev", [1, 3, 55])
@pytest.mark.parametrize("types", ["f64f64", "f32f32", "f32f64", "f64f32"])
def test_identity_with_the_chain(case, types, nlev):
    import torch
    from mpassit_amd import regrid as R
    sdt, ddt = getattr(torch, DT[types[:3]]), getattr(torch, DT[types[3:]])
    for i, name in enumerate(("P", "E", "E_none", "over_d")):
        for second in (True, False):
            _check_identity(R, case, name, nlev, sdt, ddt, second, 300 + 10 * i + nlev)


@pytest.mark.parametrize("nlev", CHUNK_LEVELS)
@pytest.mark.parametrize("types", ["f64f64", "f32f32", "f32f64", "f64f32"])
def test_identity_at_the_chunk_edges(case, types, nlev):
    """The coarse handle -- its 64-row runs outgrow the LDS chunk, so they are staged again for every batch of levels -- on both sides
    of every level-chunk threshold of one and two result tiles."""
    import torch
    from mpassit_amd import regrid as R
    sdt, ddt = getattr(torch, DT[types[:3]]), getattr(torch, DT[types[3:]])
    for second in (True, False):
        _check_identity(R, case, "coarse", nlev, sdt, ddt, second, 400 + nlev)


# ---- empty rows, sources, bands, capture ------------------------------------------------------------------------------------------------
def test_empty_rows_hold_plus_zero(case):
    import torch
    from mpassit_amd import regrid as R
    nlev = 5
    for name in ("E_none", "over_d"):
        rh, m = case[name], case["blocks"][name]
        empty = torch.as_tensor(np.diff(case["csr"][name][0]) == 0, device="cuda")
        assert int(empty.sum()) > 10
        u, v = _winds(torch, rh, rh, nlev, torch.float64, 7)
        u, v = u.abs() + 1.0, v.abs() + 1.0
        for ddt, bits in ((torch.float64, torch.int64), (torch.float32, torch.int32)):
            for second in (True, False):
                for x in _fused(R, rh, m, u, v, nlev, R.LAYOUT_CELL_FAST, ddt, second):
                    assert bool((x.view(bits)[:, empty] == 0).all()), "an empty row does not hold +0.0 bits"
                    assert bool((x[:, ~empty] != 0).any())
                for x in _fused(R, rh, m, u, v, nlev, R.LAYOUT_LEV_FAST, ddt, second):
                    assert bool((x.view(bits)[empty] == 0).all()), "an empty row does not hold +0.0 bits ([point][lev])"


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_pitched_sources(case, dt):
    """U and V in plane-pitched views whose pad is NaN go into the call as they are: the bytes of the dense call, and no NaN."""
    import torch
    from mpassit_amd import regrid as R
    dt = torch.float64 if dt == "f64" else torch.float32
    nlev = 6
    for name, g in (("E_none", case["tg"]["24x12"]), ("E", case["tg"]["72x36"])):
        rh, m = case[name], case["blocks"][name]
        ny, nx = g.lat.shape
        assert ny * nx == rh.n_src
        du, dv = _winds(torch, rh, rh, nlev, dt, 8)
        _, pu = _pitched(torch, nlev, ny, nx, dt, ny * nx + 37)
        _, pv = _pitched(torch, nlev, ny, nx, dt, ny * nx + 5)
        pu.copy_(du.reshape(pu.shape))
        pv.copy_(dv.reshape(pv.shape))
        assert not pu.is_contiguous() and not pv.is_contiguous()
        for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
            for second in (True, False):
                want = _fused(R, rh, m, du, dv, nlev, layout, second=second)
                got = _fused(R, rh, m, pu, pv, nlev, layout, second=second)
                for x, w in zip(got, want):
                    assert _bytes_equal(x, w), "pitched sources differ from dense (their NaN pad was read?)"
                    assert not torch.isnan(x).any()
    with pytest.raises(ValueError):     # a strided view that is not plane-pitched is refused by the wrapper
        R.wind_vector(rh, m, pu.transpose(1, 2), pv, nlev)


def test_canaries(case):
    """Every result sits between NaN-filled bands: the bands stay untouched, in both layouts, with and without level chunks, for one
    result and for two, on a periodic handle and on the coarse one whose runs are staged in chunks."""
    import torch
    from mpassit_amd import regrid as R
    band = 4096
    for name, levels in (("E_none", ((55, torch.float32), (1, torch.float32))),
                         ("coarse", ((55, torch.float32), (64, torch.float64), (129, torch.float64), (1, torch.float32)))):
        rh, m = case[name], case["blocks"][name]
        n = rh.n_dst
        for nlev, ddt in levels:
            u, v = _winds(torch, rh, rh, nlev, torch.float32, 90 + nlev)
            for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
                for second in (True, False):
                    want = _fused(R, rh, m, u, v, nlev, layout, ddt, second)
                    bufs = [torch.full((2 * band + nlev * n,), float("nan"), dtype=ddt, device="cuda") for _ in want]
                    outs = tuple(b[band:band + nlev * n] for b in bufs)
                    got = _fused(R, rh, m, u, v, nlev, layout, second=second, outs=outs if second else outs[0])
                    for x, o, b, w in zip(got, outs, bufs, want):
                        assert x.data_ptr() == o.data_ptr()
                        assert torch.isnan(b[:band]).all() and torch.isnan(b[band + nlev * n:]).all(), "a canary band was written"
                        assert _bytes_equal(b[band:band + nlev * n], w.reshape(-1))


def test_graph_capture_on_the_first_call(gpu_lib):
    """The very first mpg_sphere_frames_dev, mpg_wind_vector_weights_dev and mpg_wind_vector_dev of fresh handles are captured (after
    mpg_warmup_wait) on one stream and replayed twice: the bytes of the eager calls."""
    import torch
    from mpassit_amd import _lib as L, regrid as R, synth, target_grid as tg
    g = tg.define_target_grid_params("lat-lon", nx=37, ny=19, stand_lon=0.0, is_regional=False)
    m = synth.mesh_edges(synth.global_voronoi_mesh(3001))
    grid, mesh = R.Grid(g.lon, g.lat, periodic=L.GRID_PERIODIC_I), R.Mesh.from_mpas(m)
    rh = R.regrid_store_periodic_to_mesh(grid, mesh, meshloc=R.MESHLOC_EDGE)
    rn = R.regrid_store_periodic_to_mesh(grid, mesh, meshloc=R.MESHLOC_EDGE, pole_method=R.POLEMETHOD_NONE)
    assert gpu_lib.load().mpg_warmup_wait() == 0
    nlev, n = 55, rh.n_dst
    assert n % 64 != 0 and (np.diff(rn.csr()[0]) == 0).any()
    dev = dict(dtype=torch.float64, device="cuda")
    glon, glat = torch.as_tensor(np.radians(g.lon).reshape(-1), **dev), torch.as_tensor(np.radians(g.lat).reshape(-1), **dev)
    elon, elat = torch.as_tensor(m.lonEdge, **dev), torch.as_tensor(m.latEdge, **dev)
    ce, se = torch.as_tensor(np.cos(m.angleEdge), **dev), torch.as_tensor(np.sin(m.angleEdge), **dev)
    sf, df = torch.full((6, rh.n_src), float("nan"), **dev), torch.full((6, n), float("nan"), **dev)
    mh, mn = torch.full((4, rh.nnz), float("nan"), **dev), torch.full((4, rn.nnz), float("nan"), **dev)
    u, v = _winds(torch, rh, rn, nlev, torch.float32, 5)
    lf = torch.full((n, nlev), float("nan"), dtype=torch.float32, device="cuda")
    cf = tuple(torch.full((nlev, n), float("nan"), **dev) for _ in range(2))
    ms = tuple(torch.full((n, nlev), float("nan"), **dev) for _ in range(2))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):        # one stream: a chain, no parallel branches
            s = torch.cuda.current_stream().cuda_stream
            assert L.sphere_frames_dev(rh.n_src, glon.data_ptr(), glat.data_ptr(), None, None, sf.data_ptr(), s) == 0
            assert L.sphere_frames_dev(n, elon.data_ptr(), elat.data_ptr(), ce.data_ptr(), se.data_ptr(), df.data_ptr(), s) == 0
            assert L.wind_vector_weights_dev(rh._h, sf.data_ptr(), df.data_ptr(), mh.data_ptr(), s) == 0
            assert L.wind_vector_weights_dev(rn._h, sf.data_ptr(), df.data_ptr(), mn.data_ptr(), s) == 0
            R.wind_vector(rh, mh, u, v, nlev, layout=R.LAYOUT_LEV_FAST, second=False, outs=lf)
            R.wind_vector(rn, mn, u, v, nlev, layout=R.LAYOUT_CELL_FAST, outs=cf)
            R.wind_vector(rh, mh, u, v, nlev, layout=R.LAYOUT_LEV_FAST, outs=ms)
    for trial in range(2):
        u.mul_(-0.5).add_(0.25)
        v.mul_(0.75).sub_(1.0)
        graph.replay()
        torch.cuda.synchronize()
        got = [lf.clone()] + [t.clone() for t in cf] + [t.clone() for t in ms]
        assert _bytes_equal(sf, R.sphere_frames(glon, glat)) and _bytes_equal(df, R.sphere_frames(elon, elat, ce, se))
        assert _bytes_equal(mh, R.wind_vector_weights(rh, sf, df)) and _bytes_equal(mn, R.wind_vector_weights(rn, sf, df))
        want_lf = R.wind_vector(rh, mh, u, v, nlev, layout=R.LAYOUT_LEV_FAST, second=False)
        want_cf = R.wind_vector(rn, mn, u, v, nlev, layout=R.LAYOUT_CELL_FAST, out_dtype=torch.float64)
        want_ms = R.wind_vector(rh, mh, u, v, nlev, layout=R.LAYOUT_LEV_FAST, out_dtype=torch.float64)
        for x, w in zip(got, [want_lf] + list(want_cf) + list(want_ms)):
            assert not torch.isnan(x).any() and _bytes_equal(x, w)
    rh.release()
    rn.release()
    mesh.destroy()
    grid.destroy()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(case, gpu_lib):
    import torch
    from mpassit_amd import _lib as L, regrid as R, target_grid as tg
    lib = L.load()
    rh, m = case["E_none"], case["blocks"]["E_none"]
    n = rh.n_dst
    src = torch.zeros(4 * n, dtype=torch.float64, device="cuda")
    r0 = torch.zeros(4 * n, dtype=torch.float64, device="cuda")
    r1 = torch.zeros_like(r0)
    fixed = R.regrid_store_to_mesh(case["ga"], case["mesh_over"])                       # a fixed 4-slot handle
    assert fixed.nnz_per_row == 4 and fixed.n_dst <= n and fixed.n_src <= n
    gp = R.Grid.from_target(tg.define_target_grid_params("lat-lon", nx=73, ny=37, stand_lon=0.0, is_regional=False))
    pole = R.regrid_store_grid(gp, R.STAGGERLOC_EDGE2)                                  # a handle with pole terms
    assert pole.pole()[0].size > 0 and pole.n_src <= n and pole.n_dst <= n

    def refused(rc, want, who, word=None):
        msg = lib.mpg_last_error().decode()
        assert rc == want and msg, (rc, want, msg)
        assert who in msg, msg
        if word:
            assert word in msg, msg

    # -- the apply
    def args(**kw):
        return [kw.get("h", rh._h), kw.get("m", m.data_ptr()), kw.get("u", src.data_ptr()), kw.get("v", src.data_ptr()), kw.get("st", 0),
                kw.get("ldu", 0), kw.get("ldv", 0), kw.get("nlev", 2), kw.get("r0", r0.data_ptr()), kw.get("r1", r1.data_ptr()), kw.get("dt", 0),
                kw.get("layout", 1), None]
    call, who = L.wind_vector_dev, "mpg_wind_vector"
    refused(call(*args(h=fixed._h)), L.MPG_ERR_UNSUPPORTED, who, "mpg_handle_from_weights")
    refused(call(*args(h=fixed._h)), L.MPG_ERR_UNSUPPORTED, who, "mpg_handle_get_weights")
    refused(call(*args(h=pole._h)), L.MPG_ERR_UNSUPPORTED, who, "pole")
    refused(call(*args(st=2)), L.MPG_ERR_UNSUPPORTED, who, "big-endian")
    refused(call(*args(dt=3)), L.MPG_ERR_UNSUPPORTED, who, "big-endian")
    refused(call(*args(h=None)), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(*args(m=None)), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(*args(u=None)), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(*args(v=None)), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(*args(r0=None)), L.MPG_ERR_INVALID_ARG, who, "NULL")
    assert call(*args(r1=None)) == 0                                                    # r1_dev may be NULL
    refused(call(*args(nlev=0)), L.MPG_ERR_INVALID_ARG, who, "nlev")
    refused(call(*args(layout=2)), L.MPG_ERR_INVALID_ARG, who, "dst_layout")
    refused(call(*args(st=4)), L.MPG_ERR_INVALID_ARG, who)
    refused(call(*args(dt=-1)), L.MPG_ERR_INVALID_ARG, who)
    refused(call(*args(ldu=rh.n_src - 1)), L.MPG_ERR_INVALID_ARG, who, "u_level_stride")
    refused(call(*args(ldv=rh.n_src - 1)), L.MPG_ERR_INVALID_ARG, who, "v_level_stride")
    refused(call(*args(r1=r0.data_ptr())), L.MPG_ERR_INVALID_ARG, who, "alias")
    refused(call(*args(r1=r0.data_ptr() + 8)), L.MPG_ERR_INVALID_ARG, who, "r0_dev and r1_dev")
    refused(call(*args(r0=src.data_ptr())), L.MPG_ERR_INVALID_ARG, who, "source")
    refused(call(*args(r1=src.data_ptr())), L.MPG_ERR_INVALID_ARG, who, "source")
    big = torch.zeros(max(4 * rh.nnz, 4 * n), dtype=torch.float64, device="cuda")      # blocks in an array large enough to lay a result over
    refused(call(*args(m=big.data_ptr(), r0=big.data_ptr())), L.MPG_ERR_INVALID_ARG, who, "m_dev")
    refused(call(*args(m=big.data_ptr(), r1=big.data_ptr() + 8 * 3 * rh.nnz)), L.MPG_ERR_INVALID_ARG, who, "m_dev")
    assert call(*args()) == 0 and call(*args(ldu=rh.n_src, ldv=rh.n_src + 5)) == 0
    # -- the blocks
    call, who = L.wind_vector_weights_dev, "mpg_wind_vector_weights"
    sf, df = case["sf"]["E_none"], case["df"]["E_none"]
    out = torch.zeros(4 * rh.nnz, dtype=torch.float64, device="cuda")
    refused(call(fixed._h, sf.data_ptr(), df.data_ptr(), out.data_ptr(), None), L.MPG_ERR_UNSUPPORTED, who, "mpg_handle_from_weights")
    refused(call(pole._h, sf.data_ptr(), df.data_ptr(), out.data_ptr(), None), L.MPG_ERR_UNSUPPORTED, who, "pole")
    refused(call(None, sf.data_ptr(), df.data_ptr(), out.data_ptr(), None), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(rh._h, None, df.data_ptr(), out.data_ptr(), None), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(rh._h, sf.data_ptr(), None, out.data_ptr(), None), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(rh._h, sf.data_ptr(), df.data_ptr(), None, None), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(rh._h, sf.data_ptr(), df.data_ptr(), df.data_ptr(), None), L.MPG_ERR_INVALID_ARG, who, "alias")
    assert call(rh._h, sf.data_ptr(), df.data_ptr(), out.data_ptr(), None) == 0
    # -- the frames
    call, who = L.sphere_frames_dev, "mpg_sphere_frames"
    lon = torch.zeros(16, dtype=torch.float64, device="cuda")
    fr = torch.zeros(6 * 16, dtype=torch.float64, device="cuda")
    refused(call(16, lon.data_ptr(), lon.data_ptr(), lon.data_ptr(), None, fr.data_ptr(), None), L.MPG_ERR_INVALID_ARG, who, "come together")
    refused(call(16, lon.data_ptr(), lon.data_ptr(), None, lon.data_ptr(), fr.data_ptr(), None), L.MPG_ERR_INVALID_ARG, who, "come together")
    refused(call(16, None, lon.data_ptr(), None, None, fr.data_ptr(), None), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(16, lon.data_ptr(), None, None, None, fr.data_ptr(), None), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(16, lon.data_ptr(), lon.data_ptr(), None, None, None, None), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(0, None, None, None, None, None, None), L.MPG_ERR_INVALID_ARG, who, "NULL")        # before the n == 0 success
    refused(call(-1, lon.data_ptr(), lon.data_ptr(), None, None, fr.data_ptr(), None), L.MPG_ERR_INVALID_ARG, who, "n must be")
    refused(call(16, fr.data_ptr() + 8, lon.data_ptr(), None, None, fr.data_ptr(), None), L.MPG_ERR_INVALID_ARG, who, "alias")
    assert call(0, lon.data_ptr(), lon.data_ptr(), None, None, fr.data_ptr(), None) == 0
    assert call(16, lon.data_ptr(), lon.data_ptr(), None, None, fr.data_ptr(), None) == 0
    torch.cuda.synchronize()
    for h in (fixed, pole):
        h.release()
    gp.destroy()
    # the wrappers' own checks
    u, v = _winds(torch, rh, rh, 2, torch.float64, 1)
    with pytest.raises(ValueError):
        R.wind_vector(rh, m, u, v.float(), 2)
    with pytest.raises(ValueError):
        R.wind_vector(rh, m, u[:1], v, 2)
    with pytest.raises(ValueError):
        R.wind_vector(rh, m[:2], u, v, 2)
    with pytest.raises(ValueError):
        R.wind_vector(rh, m, u, v, 2, outs=(torch.empty(2 * n, dtype=torch.float64, device="cuda"),))
    with pytest.raises(ValueError):
        R.wind_vector_weights(rh, sf, df[:, :-1])


def test_zero_entry_handle(case):
    """A handle with no entries (from-weights with an empty list): the blocks call writes nothing, every result is +0.0."""
    import torch
    from mpassit_amd import regrid as R
    E = case["E_none"]
    none = R.RouteHandle.from_weights(E.n_src, E.n_dst, 1, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    assert none.nnz == 0 and none.nnz_per_row == 0 and none.n_dst == E.n_dst
    m = R.wind_vector_weights(none, case["sf"]["E_none"], case["df"]["E_none"])
    assert tuple(m.shape) == (4, 0)
    nlev = 3
    u, v = _winds(torch, E, E, nlev, torch.float32, 3)
    for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
        outs = tuple(torch.full((nlev * E.n_dst,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2))
        for x in R.wind_vector(none, m, u, v, nlev, layout=layout, outs=outs):
            assert bool((x.view(torch.int32) == 0).all())
        one = R.wind_vector(none, m, u, v, nlev, layout=layout, out_dtype=torch.float64, second=False)
        assert bool((one.view(torch.int64) == 0).all())
    none.release()


# ---- the differentiable op ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("second", [True, False])
@pytest.mark.parametrize("layout", ["cell_fast", "lev_fast"])
def test_autograd_dot_product(case, layout, second):
    """Float64 dot-product test: |<F(u, v), y> - <(u, v), F^T y>| <= 1e-11 * sum |terms| (the bar of test_autograd_dot_product in
    tests/test_wind_csr_gpu.py); the gradients have the inputs' dtypes and shapes."""
    import torch
    from mpassit_amd import regrid as R
    layout = R.LAYOUT_CELL_FAST if layout == "cell_fast" else R.LAYOUT_LEV_FAST
    for name in ("P", "E_none"):
        rh, m = case[name], case["blocks"][name]
        nlev = 3
        u0, v0 = _winds(torch, rh, rh, nlev, torch.float64, 23)
        u, v = u0.clone().requires_grad_(True), v0.clone().requires_grad_(True)
        out = R.wind_vector_autograd(rh, m, u, v, nlev, layout=layout, second=second)
        want = R.wind_vector(rh, m, u0, v0, nlev, layout=layout, second=second)
        out, want = (out, want) if second else ((out,), (want,))
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
        print("dot-product test (%s): lhs %.17g rhs %.17g |diff| %.3g bound %.3g" % (name, lhs, rhs, abs(lhs - rhs), bound))
        assert abs(lhs - rhs) <= bound
        assert float(u.grad.abs().max()) > 0 and float(v.grad.abs().max()) > 0


def test_autograd_float32(case):
    """float32 inputs get float32 gradients, and they are the transposes' own: gu = A00^T g0 + A10^T g1, gv = A01^T g0 + A11^T g1."""
    import torch
    from mpassit_amd import regrid as R
    rh, m, A = case["P"], case["blocks"]["P"], case["A"]["P"]
    nlev = 2
    u0, v0 = _winds(torch, rh, rh, nlev, torch.float32, 31)
    u, v = u0.clone().requires_grad_(True), v0.clone().requires_grad_(True)
    r0, r1 = R.wind_vector_autograd(rh, m, u, v, nlev, layout=R.LAYOUT_LEV_FAST)
    assert r0.dtype == torch.float32 and tuple(r0.shape) == tuple(r1.shape) == (rh.n_dst, nlev)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(37)
    y0, y1 = (torch.randn(tuple(r0.shape), dtype=torch.float32, device="cuda", generator=gen) for _ in range(2))
    ((r0 * y0).sum() + (r1 * y1).sum()).backward()
    assert u.grad.dtype == torch.float32 and v.grad.dtype == torch.float32 and u.grad.shape == u.shape and v.grad.shape == v.shape
    g0, g1 = y0.t().contiguous(), y1.t().contiguous()
    want_u = A[0].regrid_transpose(g0, nlev=nlev).reshape(u.shape) + A[2].regrid_transpose(g1, nlev=nlev).reshape(u.shape)
    want_v = A[1].regrid_transpose(g0, nlev=nlev).reshape(v.shape) + A[3].regrid_transpose(g1, nlev=nlev).reshape(v.shape)
    assert torch.allclose(u.grad, want_u, rtol=1e-6, atol=1e-6) and torch.allclose(v.grad, want_v, rtol=1e-6, atol=1e-6)
    assert float(u.grad.abs().max()) > 0 and float(v.grad.abs().max()) > 0


# ---- a wind -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["E", "P"])
def test_solid_body_rotation_is_a_wind(case, oracle, name):
    """A solid-body rotation of unit speed about an axis tilted 45 degrees through E (72 x 36 onto the edges, frames turned by angleEdge:
    un, ut) and through P (24 x 12 onto the cells: ue, ve).  The GPU result and the numpy mirror's (the weights of
    tests/_periodic_to_mesh_ref.py, target_grid's frames and blocks) agree to 1e-13: unit-speed winds, rows summing to 1, as in
    test_solid_body_rotation_onto_the_edges of tests/test_wind_csr_gpu.py.  On cap rows and on quad rows alike the GPU's error against
    the analytic V . frame does not exceed the mirror's own by more than 1e-12, and on the cap rows it does not exceed what the scalar
    route leaves on its QUAD rows, while the scalar route's cap error exceeds 0.1 (0.55 and 0.66 when this was written; the vector
    route's 6.4e-4 and 6.0e-3: information, not constants of the test)."""
    import torch
    from mpassit_amd import regrid as R
    m, rh = case["m"], case[name]
    grid, onto = ("72x36", "edges") if name == "E" else ("24x12", "cells")
    g = case["tg"][grid]
    ref = solid_body_case(oracle, m, g, onto)
    assert int(ref["cap"].sum()) == CAP_ROWS[(grid, onto)]
    sf = R.sphere_frames(np.radians(g.lon).reshape(-1), np.radians(g.lat).reshape(-1))
    if onto == "edges":
        df = R.sphere_frames(m.lonEdge, m.latEdge, np.cos(m.angleEdge), np.sin(m.angleEdge))
    else:
        df = R.sphere_frames(m.lonCell, m.latCell)
    blocks = R.wind_vector_weights(rh, sf, df)
    u, v = (torch.as_tensor(x.reshape(1, -1), device="cuda") for x in (ref["u"], ref["v"]))
    got = [x.reshape(-1).cpu().numpy() for x in R.wind_vector(rh, blocks, u, v, 1)]
    d = max(np.abs(x - w).max() for x, w in zip(got, ref["vector"]))
    s_quad, s_cap, v_quad, v_cap = solid_body_errors(ref)
    _, _, g_quad, g_cap = solid_body_errors(ref, got)
    # the scalar route on the GPU, for the cap condition
    if onto == "edges":
        cn, sn = R.mesh_edge_rotang(None, case["mesh"])
        sc = R.wind_csr_to_edges(rh, rh, cn, sn, u, v, 1, tangential=True)
    else:
        sc = R.wind_csr_to_mesh(rh, rh, None, None, u, v, 1)
    sc = [x.reshape(-1).cpu().numpy() for x in sc]
    gs_quad = max(float(np.abs(x - e)[ref["quad"]].max()) for x, e in zip(sc, ref["exact"]))
    gs_cap = max(float(np.abs(x - e)[ref["cap"]].max()) for x, e in zip(sc, ref["exact"]))
    print("%s -> %s: |GPU - numpy mirror| %.3g (bar 1e-13); vector route: quad rows GPU %.6g mirror %.6g, cap rows GPU %.6g mirror %.6g; "
          "scalar route: quad rows GPU %.6g reference %.6g, cap rows GPU %.3g reference %.3g"
          % (grid, onto, d, g_quad, v_quad, g_cap, v_cap, gs_quad, s_quad, gs_cap, s_cap))
    assert d <= 1e-13
    assert g_quad <= v_quad + 1e-12 and g_cap <= v_cap + 1e-12
    assert g_cap <= gs_quad and g_cap <= s_quad, "the vector route's cap rows are worse than the scalar route's quad rows"
    assert gs_cap > 0.1 and s_cap > 0.1
    assert 1e-5 < s_quad < 5e-2, "the reference's own error is not that of a 5- or 15-degree grid: the check's inputs are wrong"
