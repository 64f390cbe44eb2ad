"""Winds from the edge-normal u on the GPU at small sizes (mpg_reconstruct_store, mpg_reconstruct_weights_dev, mpg_wind_reconstruct_dev):
the pattern against edgesOnCell, the values BIT FOR BIT against the numpy mirror, the apply BIT FOR BIT against the chain it replaces --
nout regrid_csr_to_mesh calls of from-weights handles with the values m[k] on the [lev][edge] view of the same source -- for every type
pair, all four layout pairs, two results and three, level counts on both sides of the kernel's tile thresholds and runs longer than its
LDS chunk; empty rows, pitched sources, canaries, graph capture from the first call, refusals, a handle without entries, the
differentiable op, and the solid-body rotation taken on to a Lambert grid.

Handles:
  A   icosahedral_mesh(3): 642 cells (10 blocks + 2), rows of 5 and 6
  B   the global mesh, 20 000 cells, nEdgesOnCell zeroed for cell 0, the last cell, the whole block 128..191 and 30 seeded others
  C   130 synthetic rows over A's 1 920 edges, maxEdges 1500: about 40 random ids per row (a 64-row run exceeds the LDS chunk), one row
      of 1 500 entries (longer than a chunk), one empty row; random coefficients"""
import numpy as np
import pytest

import _wind_reconstruct_helpers as H
from _wind_pair_helpers import _bytes_equal, _pitched

pytestmark = pytest.mark.gpu

LDS_CHUNK = 512              # entries of a 64-row run the kernel keeps in LDS (wind_reconstruct_checks.h WR_CHUNK)
WR_LB = 4                    # levels a wave carries at a time on [lev][edge] sources
DT = {"f64": "float64", "f32": "float32"}
NAMES = ("A", "B", "C")


def _turn(m):
    """a turn of the cell frames that is no symmetry of anything"""
    phi = 0.3 + 2.0 * np.asarray(m.lonCell) - np.asarray(m.latCell)
    return np.cos(phi), np.sin(phi)


@pytest.fixture(scope="module")
def case(gpu_lib, global_mesh):
    import torch
    from mpassit_amd import regrid as R, synth
    d = dict(mc={}, rh={}, coeffs={}, frames={}, m={}, A={}, csr={}, n_on={}, eoc={})
    d["mc"]["A"] = H.mesh_case(synth.icosahedral_mesh(3))
    d["mc"]["B"] = H.mesh_case(global_mesh)
    rng = np.random.default_rng(23)
    for name in ("A", "B"):
        mc = d["mc"][name]
        n_on = mc["n_on"].copy()
        if name == "B":
            n_on[0] = n_on[-1] = 0
            n_on[128:192] = 0
            n_on[rng.choice(np.arange(200, n_on.size - 1), 30, replace=False)] = 0
        d["n_on"][name], d["eoc"][name], d["coeffs"][name] = n_on, mc["eoc"], mc["coeffs"]
    # C: synthetic rows over A's edges
    ne, rows, me = d["mc"]["A"]["m"].nEdges, 130, 1500
    n_on = rng.integers(36, 45, rows).astype(np.int32)
    n_on[17], n_on[77] = me, 0
    eoc = np.zeros((rows, me), np.int32)
    for c in range(rows):
        eoc[c, :n_on[c]] = rng.integers(1, ne + 1, n_on[c])
    d["n_on"]["C"], d["eoc"]["C"], d["coeffs"]["C"] = n_on, eoc, rng.uniform(-1.0, 1.0, (rows, me, 3))
    d["nEdges"] = {"A": ne, "B": d["mc"]["B"]["m"].nEdges, "C": ne}
    for name in NAMES:
        rh = d["rh"][name] = R.reconstruct_store(d["n_on"][name], d["eoc"][name], d["nEdges"][name])
        rowptr, col, val = d["csr"][name] = rh.csr()
        n = rh.n_dst
        if name == "C":
            g = np.random.default_rng(31)
            lon, lat = g.uniform(0.0, 2.0 * np.pi, n), g.uniform(-1.5, 1.5, n)
            plain, turned = R.sphere_frames(lon, lat), R.sphere_frames(lon, lat, np.cos(lon + lat), np.sin(lon + lat))
        else:
            m = d["mc"][name]["m"]
            plain, turned = R.sphere_frames(m.lonCell, m.latCell), R.sphere_frames(m.lonCell, m.latCell, *_turn(m))
        d["frames"][name] = {"plain": plain, "turned": turned, "xyz": None}
        co = torch.as_tensor(d["coeffs"][name], device="cuda")
        d["m"][name] = {k: R.reconstruct_weights(rh, co, f) for k, f in d["frames"][name].items()}
        # the chain's from-weights handles: the turned frames' two planes and the three Cartesian ones
        row = np.repeat(np.arange(1, n + 1, dtype=np.int32), np.diff(rowptr))
        d["A"][name] = {k: [R.RouteHandle.from_weights(rh.n_src, n, 1, row, (col + 1).astype(np.int32), mk) for mk in d["m"][name][k].cpu().numpy()]
                        for k in ("turned", "xyz")}
    yield d
    for name in NAMES:
        for hs in d["A"][name].values():
            for a in hs:
                a.release()
        d["rh"][name].release()


def test_the_handles_exercise_what_they_should(case):
    for name in NAMES:
        rh, n_on, eoc = case["rh"][name], case["n_on"][name], case["eoc"][name]
        rowptr, col, val = case["csr"][name]
        assert rh.nnz_per_row == 0 and rh.n_src == case["nEdges"][name] and rh.n_dst == n_on.size and rh.nx_dst == n_on.size and rh.ny_dst == 1
        assert rh.nnz == int(n_on.sum()) and np.array_equal(np.diff(rowptr), n_on) and (val == 1.0).all()
        # the file's slot order is the entry order
        assert np.array_equal(col, eoc[np.arange(eoc.shape[1])[None, :] < n_on[:, None]] - 1)
    assert case["rh"]["A"].n_dst == 642 == 10 * 64 + 2 and set(case["n_on"]["A"].tolist()) == {5, 6}
    nb = case["n_on"]["B"]
    assert nb.size == 20000 and nb.size % 64 != 0 and nb[0] == 0 and nb[-1] == 0 and (nb[128:192] == 0).all() and int((nb == 0).sum()) == 96
    nc = case["n_on"]["C"]
    rp = case["csr"]["C"][0]
    run = rp[np.minimum(np.arange(0, nc.size, 64) + 64, nc.size)] - rp[np.arange(0, nc.size, 64)]
    print("C: %d rows, longest row %d, 64-row runs %s" % (nc.size, nc.max(), run.tolist()))
    assert nc.size == 130 and run[:2].min() > LDS_CHUNK and nc.max() == 1500 > LDS_CHUNK and (nc == 0).sum() == 1
    col = case["csr"]["C"][1]
    assert any(np.unique(col[rp[c]:rp[c + 1]]).size < nc[c] for c in range(nc.size)), "duplicate edge ids in a row"


def test_the_pattern_serves_the_csr_consumers(case):
    """The Store's handle is an ordinary from-weights CSR handle: regrid_csr_to_mesh, regrid_csr_rows and regrid_transpose take it."""
    import torch
    rh = case["rh"]["A"]
    rowptr, col, _ = case["csr"]["A"]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    u = torch.randn((3, rh.n_src), dtype=torch.float64, device="cuda", generator=gen)
    row = np.repeat(np.arange(rh.n_dst), np.diff(rowptr))
    want = np.stack([np.bincount(row, weights=x[col], minlength=rh.n_dst) for x in u.cpu().numpy()])
    got = rh.regrid_csr_to_mesh(u, nlev=3).reshape(3, -1).cpu().numpy()
    assert np.abs(got - want).max() <= 1e-12
    rows = rh.regrid_csr_rows(u.t().contiguous(), nlev=3).reshape(-1, 3).cpu().numpy()
    assert np.array_equal(rows, got.T)
    g = torch.randn((3, rh.n_dst), dtype=torch.float64, device="cuda", generator=gen)
    back = rh.regrid_transpose(g, nlev=3).reshape(3, -1).cpu().numpy()
    wantT = np.stack([np.bincount(col, weights=x[row], minlength=rh.n_src) for x in g.cpu().numpy()])
    assert np.abs(back - wantT).max() <= 1e-12


# ---- the values -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "turned", "xyz"])
@pytest.mark.parametrize("name", NAMES)
def test_blocks_bit_for_bit(case, name, kind):
    """The values of the DOWNLOADED frames and rh.csr(), computed in numpy (every operation rounded, nothing contracted): the same bits."""
    from mpassit_amd import target_grid as tg
    rowptr, col, val = case["csr"][name]
    f = case["frames"][name][kind]
    want = tg.reconstruct_blocks(rowptr, case["coeffs"][name], val, None if f is None else f.cpu().numpy())
    got = case["m"][name][kind].cpu().numpy()
    assert got.shape == want.shape == (3 if kind == "xyz" else 2, case["rh"][name].nnz)
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), "%d of %d values differ" % ((got != want).sum(), got.size)
    assert (got != 0.0).any()


# ---- identity with the chain ------------------------------------------------------------------------------------------------------------
def _source(torch, rh, nlev, sdt, seed):
    """u as [lev][edge] and the same values as [edge][lev]"""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    u = (torch.randn((nlev, rh.n_src), dtype=torch.float64, device="cuda", generator=gen) * 12.0).to(sdt)
    return u, u.t().contiguous()


def _chain(A, u, nlev, ddt):
    """The route the fused call replaces, [lev][cell]: one Regrid per result (scale 1, offset 0) straight into the destination type."""
    return [a.regrid_csr_to_mesh(u, nlev=nlev, out_dtype=ddt).reshape(nlev, -1) for a in A]


def _check_identity(R, case, name, kind, nlev, sdt, ddt, seed, src_layouts=None):
    import torch
    rh, m = case["rh"][name], case["m"][name][kind]
    u, ut = _source(torch, rh, nlev, sdt, seed)
    want = _chain(case["A"][name][kind], u, nlev, ddt)
    n = rh.n_dst
    for sl, src in ((R.LAYOUT_CELL_FAST, u), (R.LAYOUT_LEV_FAST, ut)):
        if src_layouts is not None and sl not in src_layouts:
            continue
        got = R.wind_reconstruct(rh, m, src, nlev, src_layout=sl, layout=R.LAYOUT_CELL_FAST, out_dtype=ddt)
        assert len(got) == len(want) == m.shape[0]
        for i, (x, w) in enumerate(zip(got, want)):
            assert tuple(x.shape) == (nlev, n) and x.dtype == ddt
            assert _bytes_equal(x, w), "[lev][cell] result %d differs from the chain (%s %s, nlev %d, src layout %d)" % (i, name, kind, nlev, sl)
        lf = R.wind_reconstruct(rh, m, src, nlev, src_layout=sl, layout=R.LAYOUT_LEV_FAST, out_dtype=ddt)
        for i, (x, w) in enumerate(zip(lf, want)):
            assert tuple(x.shape) == (n, nlev)
            assert _bytes_equal(x, w.t().contiguous()), "[cell][lev] result %d is not the chain's transposition (%s %s, nlev %d, src layout %d)" % (
                i, name, kind, nlev, sl)
        again = R.wind_reconstruct(rh, m, src, nlev, src_layout=sl, layout=R.LAYOUT_LEV_FAST, out_dtype=ddt)
        assert all(_bytes_equal(x, y) for x, y in zip(again, lf)), "two calls differ"


def test_the_chain_handles_hold_the_values(case):
    for name in NAMES:
        rowptr, col, _ = case["csr"][name]
        for kind, hs in case["A"][name].items():
            mh = case["m"][name][kind].cpu().numpy()
            assert len(hs) == mh.shape[0]
            for j, a in enumerate(hs):
                rp, c, v = a.csr()
                assert a.nnz_per_row == 0 and np.array_equal(rp, rowptr) and np.array_equal(c, col)
                assert np.array_equal(v.view(np.int64), mh[j].view(np.int64))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("types", ["f64f64", "f32f32", "f32f64", "f64f32"])
def test_identity_with_the_chain(case, types, name):
    """nlev = 55: 4 type pairs x 2 source layouts x 2 destination layouts x nout 2 and 3, on every handle."""
    import torch
    from mpassit_amd import regrid as R
    sdt, ddt = getattr(torch, DT[types[:3]]), getattr(torch, DT[types[3:]])
    for kind in ("turned", "xyz"):
        _check_identity(R, case, name, kind, 55, sdt, ddt, 500 + len(name + kind))


def _sweep_levels():
    th = H.tile_thresholds()
    assert set(th) == {(4, 2), (4, 3), (8, 2), (8, 3)} and len(set(th.values())) == 4 and all(H.tile_plan_kc(t + 1, *k) % 32 == 0 for k, t in th.items())
    levels = {1, 2, 4 * WR_LB - 1, 4 * WR_LB + 1}
    for t in th.values():
        levels |= {t, t + 1}
    return sorted(levels)


@pytest.mark.parametrize("nlev", _sweep_levels())
def test_identity_across_the_level_sweep(case, nlev):
    """float32 sources into float32 and float64 results on A and C: one and two levels, both sides of a full batch of 4 WR_LB levels,
    and both sides of every tile-plan threshold (2 and 3 tiles of either type), found from the plan."""
    import torch
    from mpassit_amd import regrid as R
    for name in ("A", "C"):
        for ddt in (torch.float32, torch.float64):
            for kind in ("turned", "xyz"):
                _check_identity(R, case, name, kind, nlev, torch.float32, ddt, 700 + nlev)


# ---- empty rows, sources, bands, capture ------------------------------------------------------------------------------------------------
def test_empty_rows_hold_plus_zero(case):
    import torch
    from mpassit_amd import regrid as R
    nlev = 5
    for name in ("B", "C"):
        rh = case["rh"][name]
        empty = torch.as_tensor(case["n_on"][name] == 0, device="cuda")
        u, ut = _source(torch, rh, nlev, torch.float64, 7)
        for kind in ("turned", "xyz"):
            m = case["m"][name][kind]
            for ddt, bits in ((torch.float64, torch.int64), (torch.float32, torch.int32)):
                for sl, src in ((R.LAYOUT_CELL_FAST, u), (R.LAYOUT_LEV_FAST, ut)):
                    for x in R.wind_reconstruct(rh, m, src, nlev, src_layout=sl, layout=R.LAYOUT_CELL_FAST, out_dtype=ddt):
                        assert bool((x.view(bits)[:, empty] == 0).all()), "an empty row does not hold +0.0 bits"
                        assert bool((x[:, ~empty] != 0).any())
                    for x in R.wind_reconstruct(rh, m, src, nlev, src_layout=sl, layout=R.LAYOUT_LEV_FAST, out_dtype=ddt):
                        assert bool((x.view(bits)[empty] == 0).all()), "an empty row does not hold +0.0 bits ([cell][lev])"


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_pitched_sources(case, dt):
    """u in a plane-pitched [lev][edge] view whose pad is NaN goes into the call as it is: the bytes of the dense call, and no NaN."""
    import torch
    from mpassit_amd import _lib as L, regrid as R
    dt = torch.float64 if dt == "f64" else torch.float32
    nlev = 6
    for name in ("A", "B"):
        rh = case["rh"][name]
        du, _ = _source(torch, rh, nlev, dt, 8)
        _, pu = _pitched(torch, nlev, 1, rh.n_src, dt, rh.n_src + 37)
        pu.copy_(du.reshape(pu.shape))
        assert not pu.is_contiguous()
        for kind in ("turned", "xyz"):
            m = case["m"][name][kind]
            for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
                want = R.wind_reconstruct(rh, m, du, nlev, src_layout=R.LAYOUT_CELL_FAST, layout=layout)
                got = R.wind_reconstruct(rh, m, pu, nlev, src_layout=R.LAYOUT_CELL_FAST, layout=layout)
                for x, w in zip(got, want):
                    assert _bytes_equal(x, w), "a pitched source differs from the dense one (its NaN pad was read?)"
                    assert not torch.isnan(x).any()
    with pytest.raises(ValueError):     # file order is dense: the wrapper takes no strided view there
        R.wind_reconstruct(rh, m, pu, nlev, src_layout=R.LAYOUT_LEV_FAST)


def test_canaries(case):
    """Every result sits between NaN-filled bands: the bands stay untouched for all four layout pairs, with and without level chunks."""
    import torch
    from mpassit_amd import regrid as R
    band = 4096
    for name, levels in (("B", ((55, torch.float32), (1, torch.float32))),
                         ("C", ((55, torch.float64), (64, torch.float64), (129, torch.float32), (1, torch.float64)))):
        rh = case["rh"][name]
        n = rh.n_dst
        for nlev, ddt in levels:
            u, ut = _source(torch, rh, nlev, torch.float32, 90 + nlev)
            for kind in ("turned", "xyz"):
                m = case["m"][name][kind]
                for sl, src in ((R.LAYOUT_CELL_FAST, u), (R.LAYOUT_LEV_FAST, ut)):
                    for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
                        want = R.wind_reconstruct(rh, m, src, nlev, src_layout=sl, layout=layout, out_dtype=ddt)
                        bufs = [torch.full((2 * band + nlev * n,), float("nan"), dtype=ddt, device="cuda") for _ in want]
                        outs = tuple(b[band:band + nlev * n] for b in bufs)
                        got = R.wind_reconstruct(rh, m, src, nlev, src_layout=sl, layout=layout, outs=outs)
                        for x, o, b, w in zip(got, outs, bufs, want):
                            assert x.data_ptr() == o.data_ptr()
                            assert torch.isnan(b[:band]).all() and torch.isnan(b[band + nlev * n:]).all(), "a canary band was written"
                            assert _bytes_equal(b[band:band + nlev * n], w.reshape(-1))


def test_graph_capture_on_the_first_call(gpu_lib):
    """The very first mpg_reconstruct_weights_dev and mpg_wind_reconstruct_dev of a fresh handle are captured (after mpg_warmup_wait) on
    one stream and replayed twice: the bytes of the eager calls."""
    import torch
    from mpassit_amd import _lib as L, regrid as R, synth
    mc = H.mesh_case(synth.global_voronoi_mesh(3001))
    m = mc["m"]
    n_on = mc["n_on"].copy()
    n_on[5] = 0
    rh = R.reconstruct_store(n_on, mc["eoc"], m.nEdges)
    assert gpu_lib.load().mpg_warmup_wait() == 0
    nlev, n = 55, rh.n_dst
    assert n % 64 != 0
    dev = dict(dtype=torch.float64, device="cuda")
    co = torch.as_tensor(mc["coeffs"], **dev)
    df = R.sphere_frames(m.lonCell, m.latCell)
    m2, m3 = torch.full((2, rh.nnz), float("nan"), **dev), torch.full((3, rh.nnz), float("nan"), **dev)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    u = torch.randn((m.nEdges, nlev), dtype=torch.float32, device="cuda", generator=gen)      # file order
    ul = u.t().contiguous()
    cf = tuple(torch.full((nlev, n), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2))
    lf = tuple(torch.full((n, nlev), float("nan"), **dev) for _ in range(3))
    cc = tuple(torch.full((nlev, n), float("nan"), **dev) for _ in range(3))
    ll = tuple(torch.full((n, nlev), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):        # one stream: a chain, no parallel branches
            s = torch.cuda.current_stream().cuda_stream
            assert L.reconstruct_weights_dev(rh._h, mc["eoc"].shape[1], co.data_ptr(), df.data_ptr(), m2.data_ptr(), s) == 0
            assert L.reconstruct_weights_dev(rh._h, mc["eoc"].shape[1], co.data_ptr(), None, m3.data_ptr(), s) == 0
            R.wind_reconstruct(rh, m2, u, nlev, src_layout=R.LAYOUT_LEV_FAST, layout=R.LAYOUT_CELL_FAST, outs=cf)
            R.wind_reconstruct(rh, m3, u, nlev, src_layout=R.LAYOUT_LEV_FAST, layout=R.LAYOUT_LEV_FAST, outs=lf)
            R.wind_reconstruct(rh, m3, ul, nlev, src_layout=R.LAYOUT_CELL_FAST, layout=R.LAYOUT_CELL_FAST, outs=cc)
            R.wind_reconstruct(rh, m2, ul, nlev, src_layout=R.LAYOUT_CELL_FAST, layout=R.LAYOUT_LEV_FAST, outs=ll)
    for trial in range(2):
        u.mul_(-0.5).add_(0.25)
        ul.copy_(u.t())
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in cf + lf + cc + ll]
        assert _bytes_equal(m2, R.reconstruct_weights(rh, co, df)) and _bytes_equal(m3, R.reconstruct_weights(rh, co))
        want = list(R.wind_reconstruct(rh, m2, u, nlev, layout=R.LAYOUT_CELL_FAST))
        want += list(R.wind_reconstruct(rh, m3, u, nlev, layout=R.LAYOUT_LEV_FAST, out_dtype=torch.float64))
        want += list(R.wind_reconstruct(rh, m3, ul, nlev, src_layout=R.LAYOUT_CELL_FAST, layout=R.LAYOUT_CELL_FAST, out_dtype=torch.float64))
        want += list(R.wind_reconstruct(rh, m2, ul, nlev, src_layout=R.LAYOUT_CELL_FAST, layout=R.LAYOUT_LEV_FAST))
        assert len(got) == len(want) == 10
        for x, w in zip(got, want):
            assert not torch.isnan(x).any() and _bytes_equal(x, w)
        # every layout pair holds the same numbers
        assert _bytes_equal(got[0], got[8].t().contiguous()) and _bytes_equal(got[2], got[5].t().contiguous())
    rh.release()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(case, gpu_lib, conus_grid_30km):
    import ctypes as C
    import torch
    from mpassit_amd import _lib as L, regrid as R, target_grid as tg
    lib = L.load()
    rh, m = case["rh"]["A"], case["m"]["A"]["xyz"]
    n, ne = rh.n_dst, rh.n_src
    src = torch.zeros(4 * ne, dtype=torch.float64, device="cuda")
    r = [torch.zeros(4 * n, dtype=torch.float64, device="cuda") for _ in range(3)]
    mesh = R.Mesh.from_mpas(case["mc"]["A"]["m"])
    grid = R.Grid.from_target(conus_grid_30km)
    fixed = R.regrid_store(mesh, grid, R.REGRIDMETHOD_BILINEAR)                         # a fixed 3-slot handle
    assert fixed.nnz_per_row == 3
    gp = R.Grid.from_target(tg.define_target_grid_params("lat-lon", nx=73, ny=37, stand_lon=0.0, is_regional=False))
    pole = R.regrid_store_grid(gp, R.STAGGERLOC_EDGE2)                                  # a handle with pole terms
    assert pole.pole()[0].size > 0

    def refused(rc, want, who, word=None):
        msg = lib.mpg_last_error().decode()
        assert rc == want and msg, (rc, want, msg)
        assert who in msg, msg
        if word:
            assert word in msg, msg

    # -- the apply
    def args(**kw):
        nout = kw.get("nout", 3)
        return [kw.get("h", rh._h), kw.get("m", m.data_ptr()), nout, kw.get("u", src.data_ptr()), kw.get("st", 0), kw.get("sl", 1), kw.get("ldu", 0),
                kw.get("nlev", 2), kw.get("r0", r[0].data_ptr()), kw.get("r1", r[1].data_ptr()), kw.get("r2", r[2].data_ptr() if nout == 3 else None),
                kw.get("dt", 0), kw.get("layout", 0), None]
    call, who = L.wind_reconstruct_dev, "mpg_wind_reconstruct"
    assert call(*args()) == 0 and call(*args(nout=2)) == 0 and call(*args(sl=0, ldu=ne + 5)) == 0 and call(*args(sl=0, ldu=ne)) == 0
    refused(call(*args(nout=1, r1=None)), L.MPG_ERR_INVALID_ARG, who, "mpg_regrid_csr_to_mesh_dev")
    refused(call(*args(nout=1, r1=None)), L.MPG_ERR_INVALID_ARG, who, "mpg_regrid_csr_rows_dev")
    refused(call(*args(nout=4)), L.MPG_ERR_INVALID_ARG, who, "nout")
    refused(call(*args(nout=0)), L.MPG_ERR_INVALID_ARG, who, "nout")
    refused(call(*args(nout=2, r2=r[2].data_ptr())), L.MPG_ERR_INVALID_ARG, who, "r2_dev")
    refused(call(*args(nout=3, r2=None)), L.MPG_ERR_INVALID_ARG, who, "r2_dev")
    refused(call(*args(h=fixed._h)), L.MPG_ERR_UNSUPPORTED, who, "fixed")
    refused(call(*args(h=pole._h)), L.MPG_ERR_UNSUPPORTED, who, "pole")
    refused(call(*args(st=2)), L.MPG_ERR_UNSUPPORTED, who, "mpg_bswap_dev")
    refused(call(*args(dt=3)), L.MPG_ERR_UNSUPPORTED, who, "mpg_bswap_dev")
    refused(call(*args(h=None)), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(*args(m=None)), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(*args(u=None)), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(*args(r0=None)), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(*args(r1=None)), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(*args(nlev=0)), L.MPG_ERR_INVALID_ARG, who, "nlev")
    refused(call(*args(nlev=-3)), L.MPG_ERR_INVALID_ARG, who, "nlev")
    refused(call(*args(layout=2)), L.MPG_ERR_INVALID_ARG, who, "dst_layout")
    refused(call(*args(sl=2)), L.MPG_ERR_INVALID_ARG, who, "src_layout")
    refused(call(*args(st=4)), L.MPG_ERR_INVALID_ARG, who)
    refused(call(*args(dt=-1)), L.MPG_ERR_INVALID_ARG, who)
    refused(call(*args(sl=1, ldu=ne)), L.MPG_ERR_INVALID_ARG, who, "must be 0")
    refused(call(*args(sl=0, ldu=ne - 1)), L.MPG_ERR_INVALID_ARG, who, "u_level_stride")
    refused(call(*args(r1=r[0].data_ptr())), L.MPG_ERR_INVALID_ARG, who, "alias")
    refused(call(*args(r2=r[1].data_ptr() + 8)), L.MPG_ERR_INVALID_ARG, who, "alias each other")
    refused(call(*args(r0=src.data_ptr())), L.MPG_ERR_INVALID_ARG, who, "source")
    refused(call(*args(r2=src.data_ptr() + 8 * (2 * ne - 1))), L.MPG_ERR_INVALID_ARG, who, "source")
    big = torch.zeros(max(3 * rh.nnz, 4 * n), dtype=torch.float64, device="cuda")      # values in an array large enough to lay a result over
    refused(call(*args(m=big.data_ptr(), r0=big.data_ptr())), L.MPG_ERR_INVALID_ARG, who, "m_dev")
    refused(call(*args(m=big.data_ptr(), r2=big.data_ptr() + 8 * (3 * rh.nnz - 1))), L.MPG_ERR_INVALID_ARG, who, "m_dev")
    # -- the values
    call, who = L.reconstruct_weights_dev, "mpg_reconstruct_weights"
    me = case["eoc"]["A"].shape[1]
    co = torch.as_tensor(case["coeffs"]["A"], device="cuda")
    df = case["frames"]["A"]["plain"]
    out = torch.zeros(3 * rh.nnz, dtype=torch.float64, device="cuda")
    assert call(rh._h, me, co.data_ptr(), df.data_ptr(), out.data_ptr(), None) == 0 and call(rh._h, me, co.data_ptr(), None, out.data_ptr(), None) == 0
    refused(call(fixed._h, me, co.data_ptr(), df.data_ptr(), out.data_ptr(), None), L.MPG_ERR_UNSUPPORTED, who, "fixed")
    refused(call(pole._h, me, co.data_ptr(), df.data_ptr(), out.data_ptr(), None), L.MPG_ERR_UNSUPPORTED, who, "pole")
    refused(call(None, me, co.data_ptr(), df.data_ptr(), out.data_ptr(), None), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(rh._h, me, None, df.data_ptr(), out.data_ptr(), None), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(rh._h, me, co.data_ptr(), df.data_ptr(), None, None), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(rh._h, me - 1, co.data_ptr(), df.data_ptr(), out.data_ptr(), None), L.MPG_ERR_INVALID_ARG, who, "exceeds maxEdges")
    refused(call(rh._h, me, co.data_ptr(), df.data_ptr(), df.data_ptr(), None), L.MPG_ERR_INVALID_ARG, who, "alias")
    refused(call(rh._h, me, co.data_ptr(), df.data_ptr(), co.data_ptr() + 8, None), L.MPG_ERR_INVALID_ARG, who, "alias")
    # -- the Store
    who = "mpg_reconstruct_store"
    n_on, eoc = np.ascontiguousarray(case["n_on"]["A"]), np.ascontiguousarray(case["eoc"]["A"])
    h = C.c_void_p()

    def store(n_on_, eoc_, nc=n, nedges=ne, maxe=me, out=C.byref(h)):
        return L.reconstruct_store(nc, nedges, maxe, n_on_.ctypes.data if n_on_ is not None else None, eoc_.ctypes.data if eoc_ is not None else None, out)
    bad = n_on.copy()
    bad[41] = me + 1
    refused(store(bad, eoc), L.MPG_ERR_INVALID_ARG, who, "cell 41")
    bad[41] = -1
    refused(store(bad, eoc), L.MPG_ERR_INVALID_ARG, who, "cell 41")
    bade = eoc.copy()
    bade[77, 2] = ne + 1
    refused(store(n_on, bade), L.MPG_ERR_INVALID_ARG, who, "cell 77")
    bade[77, 2] = 0
    refused(store(n_on, bade), L.MPG_ERR_INVALID_ARG, who, "cell 77")
    bade[77, 2] = eoc[77, 2]
    bade[77, me - 1] = -5 if n_on[77] < me else bade[77, me - 1]                       # a slot past the count is not read
    assert store(n_on, bade) == 0
    check = R.RouteHandle(h)
    assert check.nnz == rh.nnz
    check.release()
    refused(store(None, eoc), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(store(n_on, None), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(store(n_on, eoc, out=None), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(store(n_on, eoc, nc=0), L.MPG_ERR_INVALID_ARG, who, "sizes")
    refused(store(n_on, eoc, maxe=-1), L.MPG_ERR_INVALID_ARG, who, "sizes")
    refused(store(n_on, eoc, nedges=2 ** 31), L.MPG_ERR_OVERFLOW, who, "int32")
    torch.cuda.synchronize()
    for x in (fixed, pole):
        x.release()
    for x in (gp, grid, mesh):
        x.destroy()
    # the wrappers' own checks
    u = torch.zeros((2, ne), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        R.wind_reconstruct(rh, m, u[:1], 2, src_layout=R.LAYOUT_CELL_FAST)
    with pytest.raises(ValueError):
        R.wind_reconstruct(rh, m[:, :-1], u, 2, src_layout=R.LAYOUT_CELL_FAST)
    with pytest.raises(ValueError):
        R.wind_reconstruct(rh, m, u, 2, src_layout=R.LAYOUT_CELL_FAST, outs=(torch.empty(2 * n, dtype=torch.float64, device="cuda"),))
    with pytest.raises(ValueError):
        R.reconstruct_weights(rh, co[:, :, :2])
    with pytest.raises(ValueError):
        R.reconstruct_weights(rh, co, df[:, :-1])
    with pytest.raises(ValueError):
        R.reconstruct_store(n_on, eoc[:-1], ne)


def test_zero_entry_handle(case):
    """A handle with no entries (every nEdgesOnCell zero): the values call writes nothing, every result is +0.0."""
    import torch
    from mpassit_amd import regrid as R
    A = case["rh"]["A"]
    none = R.reconstruct_store(np.zeros(A.n_dst, np.int32), case["eoc"]["A"], A.n_src)
    assert none.nnz == 0 and none.nnz_per_row == 0 and none.n_dst == A.n_dst and none.n_src == A.n_src
    co = torch.as_tensor(case["coeffs"]["A"], device="cuda")
    nlev = 3
    u, ut = _source(torch, A, nlev, torch.float32, 3)
    for frames, nout in ((case["frames"]["A"]["plain"], 2), (None, 3)):
        m = R.reconstruct_weights(none, co, frames)
        assert tuple(m.shape) == (nout, 0)
        for sl, src in ((R.LAYOUT_CELL_FAST, u), (R.LAYOUT_LEV_FAST, ut)):
            for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
                outs = tuple(torch.full((nlev * A.n_dst,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(nout))
                for x in R.wind_reconstruct(none, m, src, nlev, src_layout=sl, layout=layout, outs=outs):
                    assert bool((x.view(torch.int32) == 0).all())
                for x in R.wind_reconstruct(none, m, src, nlev, src_layout=sl, layout=layout, out_dtype=torch.float64):
                    assert bool((x.view(torch.int64) == 0).all())
    none.release()


# ---- the differentiable op --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["turned", "xyz"])
def test_autograd_against_the_dense_matrix(case, kind):
    """On A in float64: the backward against the dense matrices assembled from m, 1e-12 relative, for all four layout pairs."""
    import torch
    from mpassit_amd import regrid as R
    rh, m = case["rh"]["A"], case["m"]["A"][kind]
    rowptr, col, _ = case["csr"]["A"]
    n, ne, nlev = rh.n_dst, rh.n_src, 3
    row = torch.as_tensor(np.repeat(np.arange(n), np.diff(rowptr)), device="cuda")
    colt = torch.as_tensor(col.astype(np.int64), device="cuda")
    dense = []
    for mk in m:
        D = torch.zeros((n, ne), dtype=torch.float64, device="cuda")
        D.index_put_((row, colt), mk, accumulate=True)
        dense.append(D)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(12)
    u0 = torch.randn((nlev, ne), dtype=torch.float64, device="cuda", generator=gen)
    gs = [torch.randn((nlev, n), dtype=torch.float64, device="cuda", generator=gen) for _ in dense]
    want = sum(g @ D for g, D in zip(gs, dense))                     # [lev][edge]
    for sl in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
        for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
            u = (u0 if sl == R.LAYOUT_CELL_FAST else u0.t().contiguous()).clone().requires_grad_(True)
            outs = R.wind_reconstruct_autograd(rh, m, u, nlev, src_layout=sl, layout=layout)
            assert len(outs) == len(dense)
            fwd = R.wind_reconstruct(rh, m, u.detach(), nlev, src_layout=sl, layout=layout)
            assert all(_bytes_equal(a.detach(), b) for a, b in zip(outs, fwd))
            loss = sum((o * (g if layout == R.LAYOUT_CELL_FAST else g.t())).sum() for o, g in zip(outs, gs))
            loss.backward()
            got = u.grad if sl == R.LAYOUT_CELL_FAST else u.grad.t()
            assert u.grad.shape == u.shape
            rel = float((got - want).abs().max() / want.abs().max())
            print("%s, src layout %d, layout %d: backward against the dense matrix %.3e relative" % (kind, sl, layout, rel))
            assert rel <= 1e-12


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_solid_body_onto_the_lambert_grid(case, oracle, conus_grid_30km):
    """The solid-body u on the global mesh (no zeroed rows): wind_reconstruct with east / north frames against the mirror to 1e-13 absolute
    (rows of at most 8 entries of magnitude at most 1), then through regrid_store(mesh, 180 x 106 Lambert) and rotate_winds_cgrid: finite
    and within 1e-12 of the mirror taken through the handle's weights and the rotation by the oracle, on mapped points."""
    import torch
    from mpassit_amd import regrid as R, target_grid as tg
    mc = case["mc"]["B"]
    m, g = mc["m"], conus_grid_30km
    rh = R.reconstruct_store(mc["n_on"], mc["eoc"], m.nEdges)
    rowptr, col, val = rh.csr()
    assert np.diff(rowptr).max() <= 8 and np.abs(mc["u"]).max() <= 1.0
    frames = tg.sphere_frames_at(m.lonCell, m.latCell)
    mm = R.reconstruct_weights(rh, mc["coeffs"], R.sphere_frames(m.lonCell, m.latCell))
    mirror_m = tg.reconstruct_blocks(rowptr, mc["coeffs"], val, frames)
    nlev = 3
    scale = np.array([1.0, -0.5, 0.25])
    u = np.ascontiguousarray(mc["u"][:, None] * scale[None, :])                              # [edge][lev], file order
    zonal, merid = R.wind_reconstruct(rh, mm, torch.as_tensor(u, device="cuda"), nlev)       # [lev][cell]
    got = np.stack([zonal.cpu().numpy(), merid.cpu().numpy()])
    want = np.stack([tg.reconstruct_apply(rowptr, col, mirror_m, u[:, k]) for k in range(nlev)], axis=1)      # [2][lev][cell]
    err = np.abs(got - want).max()
    exact = np.stack([(mc["exact"] * frames[:3].T).sum(axis=1), (mc["exact"] * frames[3:].T).sum(axis=1)])
    print("wind_reconstruct against the mirror %.3e; against the analytic wind %.3e" % (err, np.abs(got[:, 0] - exact).max()))
    assert err <= 1e-13
    assert np.abs(got[:, 0] - exact).max() <= 3.5e-3
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
    rg = R.regrid_store(mesh, grid, R.REGRIDMETHOD_BILINEAR)
    assert (g.nx, g.ny) == (180, 106) and rg.n_dst == 180 * 106
    U, V = (rg.regrid(np.ascontiguousarray(x), nlev=nlev).reshape(nlev, g.ny, g.nx) for x in got)
    R.rotate_winds_cgrid(g.cosa, g.sina, U, V)
    idx, w = rg.weights()
    mapped = idx[:, 0] >= 0
    Uo, Vo = oracle.rotate_winds(g.cosa, g.sina, oracle.apply_fixed(idx, w, want[0], nlev), oracle.apply_fixed(idx, w, want[1], nlev))
    assert mapped.sum() > 0.9 * mapped.size and np.isfinite(U).all() and np.isfinite(V).all()
    d = max(np.abs(U.reshape(nlev, -1)[:, mapped] - Uo.reshape(nlev, -1)[:, mapped]).max(),
            np.abs(V.reshape(nlev, -1)[:, mapped] - Vo.reshape(nlev, -1)[:, mapped]).max())
    print("after regrid and rotate_winds_cgrid: %.3e from the mirror-plus-oracle chain on %d mapped points" % (d, mapped.sum()))
    assert d <= 1e-12
    for x in (rg, rh):
        x.release()
    mesh.destroy()
    grid.destroy()
