"""Winds through CSR handles on the GPU at small sizes (mpg_wind_csr_to_mesh_dev, mpg_wind_csr_to_edges_dev): the fused call held BIT
FOR BIT to the chain it replaces -- two regrid_csr_to_mesh calls into float64, the torch products and sums, one cast, +0.0 where a row
is empty in either handle -- for every policy, every type pair, both layouts and level counts on both sides of the kernel's chunk
limits; the either rule, negative zeros, one handle twice against two equal handles, pitched sources, canaries, graph capture from the
first call, refusals, the differentiable ops, and a solid-body rotation from a 72 x 36 global grid onto the mesh's edges.

Handles:
  P               periodic 24 x 12 ALLAVG onto the 20 000 cells of the global mesh (no multiple of 64; cap rows of 24 entries)
  E               periodic 72 x 36 ALLAVG onto its 59 994 edges
  E_all, E_none   24 x 12 ALLAVG and NONE onto the edges: 505 edges are unmapped in E_none only
  conservative Grid -> Mesh handles of the 61 x 41 Lambert grid of tests/test_conserve_to_mesh_gpu.py: onto its coarse mesh (a 64-row
                  run longer than the kernel's LDS chunk) and onto its overhanging mesh (empty rows), DSTAREA and FRACAREA"""
import numpy as np
import pytest

import _periodic_to_mesh_ref as PR
from _wind_pair_helpers import _bytes_equal, _pitched, _winds
from conftest import LAMBERT

pytestmark = pytest.mark.gpu

LDS_CHUNK = 1024             # entries of a 64-row run the kernel keeps in LDS per handle (apply_mesh.h AM_CHUNK)
# [point][lev] results leave through ONE LDS tile of at most 64 KB (un alone: all levels in the tile up to 127 float64 / 255 float32
# levels) or TWO of half the cap each (63 / 127), in level chunks beyond (apply_mesh.h am_tile_plan)
CHUNK_LEVELS = (63, 64, 65, 127, 128, 129, 257)
DT = {"f64": "float64", "f32": "float32"}
POLICIES = ("rotated", "plain", "un", "both")


def _empty(torch, rh_u, rh_v):
    """the points whose row is empty in either handle, as a CUDA mask"""
    un = np.diff(rh_u.csr()[0]) == 0
    if rh_v is not rh_u:
        un = un | (np.diff(rh_v.csr()[0]) == 0)
    return torch.as_tensor(un, device="cuda")


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
    d["E_all"] = R.regrid_store_periodic_to_mesh(d["grid"]["24x12"], mesh, meshloc=R.MESHLOC_EDGE)
    d["E_none"] = R.regrid_store_periodic_to_mesh(d["grid"]["24x12"], mesh, meshloc=R.MESHLOC_EDGE, pole_method=R.POLEMETHOD_NONE)
    d["rot_edge"] = R.mesh_edge_rotang(None, mesh)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(77)
    phi = torch.rand(d["P"].n_dst, dtype=torch.float64, device="cuda", generator=gen) * (2.0 * np.pi)
    d["rot_P"] = (torch.cos(phi), torch.sin(phi))                     # random unit (c, s) at the cells
    # the conservative handles of the Lambert grid
    gl = tg.define_target_grid_params("lambert", 61, 41, dx=30000.0, dy=30000.0, **LAMBERT)
    d["gl"], d["ga"] = gl, R.Grid.from_proj(gl, fill_target=False)
    d["m_coarse"] = synth.regional_mesh_for_lambert(gl.proj, 61, 41, 201, margin=0.05, seed=13)
    d["m_over"] = synth.regional_mesh_for_lambert(gl.proj, 61, 41, 6001, margin=0.05, seed=11)
    d["mesh_coarse"], d["mesh_over"] = R.Mesh.from_mpas(d["m_coarse"]), R.Mesh.from_mpas(d["m_over"])
    d["coarse"] = R.regrid_store_conserve_to_mesh(d["ga"], d["mesh_coarse"], R.NORM_DSTAREA)
    d["over_d"] = R.regrid_store_conserve_to_mesh(d["ga"], d["mesh_over"], R.NORM_DSTAREA)
    d["over_f"] = R.regrid_store_conserve_to_mesh(d["ga"], d["mesh_over"], R.NORM_FRACAREA)
    d["rot_coarse"] = R.mesh_rotang(d["ga"], d["mesh_coarse"])
    d["rot_over"] = R.mesh_rotang(d["ga"], d["mesh_over"])
    handles = ("P", "E", "E_all", "E_none", "coarse", "over_d", "over_f")
    for k in handles:
        assert d[k].nnz_per_row == 0 and d[k].pole()[0].size == 0
    yield d
    for k in handles:
        d[k].release()
    for k in ("mesh", "mesh_coarse", "mesh_over", "ga"):
        d[k].destroy()
    for grid in d["grid"].values():
        grid.destroy()


def test_the_handles_exercise_what_they_should(case):
    rp = case["P"].csr()[0]
    assert case["P"].n_dst == 20000 and case["P"].n_dst % 64 != 0 and set(np.unique(np.diff(rp))) == {4, 24}
    assert case["E"].n_dst == case["E_all"].n_dst == case["E_none"].n_dst == 59994 and set(np.unique(np.diff(case["E"].csr()[0]))) == {4, 72}
    e_all, e_none = np.diff(case["E_all"].csr()[0]) == 0, np.diff(case["E_none"].csr()[0]) == 0
    assert int(e_all.sum()) == 0 and int(e_none.sum()) == 505, "505 edges are unmapped in rh_v only"
    rp = case["coarse"].csr()[0]
    run = rp[np.minimum(np.arange(0, rp.size - 1, 64) + 64, rp.size - 1)] - rp[np.arange(0, rp.size - 1, 64)]
    print("coarse mesh: %d cells, longest row %d entries, longest 64-row run %d" % (case["coarse"].n_dst, np.diff(rp).max(), run.max()))
    assert case["coarse"].n_dst == case["m_coarse"].nCells < 300 and run.max() > LDS_CHUNK, "the coarse mesh exercises the run chunking"
    rd, rf = case["over_d"].csr(), case["over_f"].csr()
    assert case["over_d"].n_dst == case["m_over"].nCells and case["over_d"].n_dst % 64 != 0
    assert (np.diff(rd[0]) == 0).sum() > 10, "the overhanging mesh has empty rows"
    assert case["over_d"]._h.value != case["over_f"]._h.value and not np.array_equal(rd[2], rf[2]), "two different handles"


def _chain(torch, policy, rh_u, rh_v, rot, un, u, v, nlev, ddt):
    """The route the fused call replaces, [lev][point]: every product and every sum a torch operation of its own (nothing to contract)."""
    a = rh_u.regrid_csr_to_mesh(u, nlev=nlev, out_dtype=torch.float64).reshape(nlev, -1)
    b = rh_v.regrid_csr_to_mesh(v, nlev=nlev, out_dtype=torch.float64).reshape(nlev, -1)
    if policy == "plain":
        outs = [a, b]
    else:
        c, s = rot
        t1 = a * c
        t2 = b * s
        if policy == "rotated":
            t3 = a * s
            t4 = b * c
            outs = [t1 - t2, t3 + t4]
        else:
            outs = [t1 + t2]
            if policy == "both":
                t3 = b * c
                t4 = a * s
                outs.append(t3 - t4)
    outs = [x.to(ddt) for x in outs]
    for x in outs:
        x[:, un] = 0.0
    return outs


def _fused(R, policy, rh_u, rh_v, rot, u, v, nlev, layout, ddt=None, outs=None):
    if policy in ("rotated", "plain"):
        c, s = rot if policy == "rotated" else (None, None)
        return list(R.wind_csr_to_mesh(rh_u, rh_v, c, s, u, v, nlev, layout=layout, out_dtype=ddt, outs=outs))
    tan = policy == "both"
    got = R.wind_csr_to_edges(rh_u, rh_v, rot[0], rot[1], u, v, nlev, layout=layout, out_dtype=ddt, tangential=tan,
                              outs=outs if tan or outs is None else outs[0])
    return list(got) if tan else [got]


def _check_identity(R, policy, rh_u, rh_v, rot, nlev, sdt, ddt, seed):
    import torch
    un = _empty(torch, rh_u, rh_v)
    u, v = _winds(torch, rh_u, rh_v, nlev, sdt, seed)
    want = _chain(torch, policy, rh_u, rh_v, rot, un, u, v, nlev, ddt)
    n = rh_u.n_dst
    got = _fused(R, policy, rh_u, rh_v, rot, u, v, nlev, R.LAYOUT_CELL_FAST, ddt)
    assert len(got) == len(want)
    for i, (x, w) in enumerate(zip(got, want)):
        assert tuple(x.shape) == (nlev, n) and x.dtype == ddt
        assert _bytes_equal(x, w), "[lev][point] result %d differs from the chain (%s, nlev %d)" % (i, policy, nlev)
    lf = _fused(R, policy, rh_u, rh_v, rot, u, v, nlev, R.LAYOUT_LEV_FAST, ddt)
    for i, (x, w) in enumerate(zip(lf, want)):
        assert tuple(x.shape) == (n, nlev)
        assert _bytes_equal(x, w.t().contiguous()), "[point][lev] result %d is not the transposition of the chain (%s, nlev %d)" % (i, policy, nlev)
    again = _fused(R, policy, rh_u, rh_v, rot, u, v, nlev, R.LAYOUT_LEV_FAST, ddt)
    assert all(_bytes_equal(x, y) for x, y in zip(again, lf)), "two calls differ"
    return u, v, want


def _cases(case):
    """(policy, rh_u, rh_v, rotation) of every identity case"""
    return [("rotated", case["P"], case["P"], case["rot_P"]), ("plain", case["P"], case["P"], None),
            ("un", case["E"], case["E"], case["rot_edge"]), ("both", case["E"], case["E"], case["rot_edge"]),
            ("both", case["E_all"], case["E_none"], case["rot_edge"]), ("un", case["E_none"], case["E_all"], case["rot_edge"]),
            ("rotated", case["over_d"], case["over_d"], case["rot_over"]), ("rotated", case["over_d"], case["over_f"], case["rot_over"]),
            ("plain", case["over_f"], case["over_d"], None)]


# ---- identity with the chain --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlev", [1, 3, 55])
@pytest.mark.parametrize("types", ["f64f64", "f32f32", "f32f64", "f64f32"])
def test_identity_with_the_chain(case, types, nlev):
    import torch
    from mpassit_amd import regrid as R
    sdt, ddt = getattr(torch, DT[types[:3]]), getattr(torch, DT[types[3:]])
    assert {c[0] for c in _cases(case)} == set(POLICIES)
    for i, (policy, rh_u, rh_v, rot) in enumerate(_cases(case)):
        _check_identity(R, policy, rh_u, rh_v, rot, nlev, sdt, ddt, 300 + 10 * i + nlev)


@pytest.mark.parametrize("nlev", CHUNK_LEVELS)
@pytest.mark.parametrize("types", ["f64f64", "f32f32", "f32f64", "f64f32"])
def test_identity_at_the_chunk_edges(case, types, nlev):
    """The coarse handle -- its 64-row runs outgrow the LDS chunk, so they are staged again for every batch of levels -- on both sides
    of every level-chunk threshold of one and two result tiles: one handle twice, every policy, and with its FRACAREA twin as a second
    handle (two runs resident, both staged in chunks)."""
    import torch
    from mpassit_amd import regrid as R
    sdt, ddt = getattr(torch, DT[types[:3]]), getattr(torch, DT[types[3:]])
    rh, rot = case["coarse"], case["rot_coarse"]
    for policy in POLICIES:
        _check_identity(R, policy, rh, rh, rot, nlev, sdt, ddt, 400 + nlev)
    other = R.regrid_store_conserve_to_mesh(case["ga"], case["mesh_coarse"], R.NORM_FRACAREA)
    assert other._h.value != rh._h.value
    for policy in ("rotated", "un"):
        _check_identity(R, policy, rh, other, rot, nlev, sdt, ddt, 500 + nlev)
    other.release()


# ---- the either rule, negative zero, equal handles ------------------------------------------------------------------------------------
def test_either_rule(case):
    """505 edges have a row in E_all and none in E_none: with sources that are nowhere zero they hold +0.0 BITS in every result, in both
    layouts and whichever side the emptier handle is on, and every other edge holds something else."""
    import torch
    from mpassit_amd import regrid as R
    one = torch.as_tensor(np.diff(case["E_none"].csr()[0]) == 0, device="cuda")
    assert int(one.sum()) == 505
    nlev = 5
    for rh_u, rh_v in ((case["E_all"], case["E_none"]), (case["E_none"], case["E_all"])):
        u, v = _winds(torch, rh_u, rh_v, nlev, torch.float64, 7)
        u, v = u.abs() + 1.0, v.abs() + 1.0
        for ddt, bits in ((torch.float64, torch.int64), (torch.float32, torch.int32)):
            for policy, rot in (("both", case["rot_edge"]), ("rotated", case["rot_edge"]), ("plain", None)):
                cf = _fused(R, policy, rh_u, rh_v, rot, u, v, nlev, R.LAYOUT_CELL_FAST, ddt)
                lf = _fused(R, policy, rh_u, rh_v, rot, u, v, nlev, R.LAYOUT_LEV_FAST, ddt)
                for x in cf:
                    assert bool((x.view(bits)[:, one] == 0).all()), "a one-sided edge does not hold +0.0 bits"
                for x in lf:
                    assert bool((x.view(bits)[one] == 0).all()), "a one-sided edge does not hold +0.0 bits ([point][lev])"
                if policy == "plain":
                    assert bool((cf[0][:, ~one] != 0).all()) and bool((cf[1][:, ~one] != 0).all())


def test_negative_zero(case):
    """Sources of all -0.0: each Regrid gives +0.0 (fma(w, -0.0, +0.0) and the epilogue fma(acc, 1.0, 0.0) are +0.0), so without a
    rotation, and with angles in the first quadrant (c, s > 0: every product is +0.0), every result holds +0.0 BITS everywhere -- in the
    chain and in the fused call.  With angles of any sign a product +0.0 * c is -0.0 where c < 0, in the chain as in the fused call: the
    bytes are the chain's there too, sign bits included."""
    import torch
    from mpassit_amd import regrid as R
    nlev = 3
    gen = torch.Generator(device="cuda")
    gen.manual_seed(78)
    for rh, any_rot in ((case["P"], case["rot_P"]), (case["E"], case["rot_edge"])):
        phi = torch.rand(rh.n_dst, dtype=torch.float64, device="cuda", generator=gen) * 1.5 + 0.03      # (0.03, 1.53): c, s > 0
        first = (torch.cos(phi), torch.sin(phi))
        assert float(first[0].min()) > 0 and float(first[1].min()) > 0 and float(any_rot[0].min()) < 0 and float(any_rot[1].min()) < 0
        un = _empty(torch, rh, rh)
        for sdt, ddt, bits in ((torch.float64, torch.float64, torch.int64), (torch.float32, torch.float32, torch.int32),
                               (torch.float32, torch.float64, torch.int64)):
            u = torch.full((nlev, rh.n_src), -0.0, dtype=sdt, device="cuda")
            v = torch.full((nlev, rh.n_src), -0.0, dtype=sdt, device="cuda")
            assert bool((u.view(torch.int64 if sdt == torch.float64 else torch.int32) != 0).all()), "the sources are not negative zeros"
            for policy, rot, all_plus in (("plain", None, True), ("rotated", first, True), ("un", first, True), ("both", first, True),
                                          ("rotated", any_rot, False), ("both", any_rot, False)):
                want = _chain(torch, policy, rh, rh, rot, un, u, v, nlev, ddt)
                if all_plus:
                    assert all(bool((w.view(bits) == 0).all()) for w in want), "the chain itself leaves a sign bit"
                for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
                    got = _fused(R, policy, rh, rh, rot, u, v, nlev, layout, ddt)
                    for x, w in zip(got, want):
                        assert _bytes_equal(x, w if layout == R.LAYOUT_CELL_FAST else w.t().contiguous()), (policy, all_plus)
                        if all_plus:
                            assert bool((x.view(bits) == 0).all()), "a -0.0 source left a sign bit (%s)" % policy


def test_one_handle_twice_equals_two_equal_handles(case):
    import torch
    from mpassit_amd import regrid as R
    P = case["P"]
    row, col, S = P.to_esmf_weights()
    twin = R.RouteHandle.from_weights(P.n_src, P.n_dst, 1, row, col, S)
    assert twin._h.value != P._h.value and twin.nnz_per_row == 0
    a, b = P.csr(), twin.csr()
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(a[2].view(np.int64), b[2].view(np.int64)), "the copy holds other bytes"
    for nlev, sdt, ddt in ((1, torch.float64, torch.float64), (55, torch.float32, torch.float32), (64, torch.float64, torch.float32)):
        u, v = _winds(torch, P, P, nlev, sdt, 900 + nlev)
        for policy, rot in (("rotated", case["rot_P"]), ("plain", None), ("both", case["rot_P"])):
            for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
                once = _fused(R, policy, P, P, rot, u, v, nlev, layout, ddt)
                for hu, hv in ((P, twin), (twin, P), (twin, twin)):
                    two = _fused(R, policy, hu, hv, rot, u, v, nlev, layout, ddt)
                    assert all(_bytes_equal(x, y) for x, y in zip(once, two)), "one handle twice differs from two equal handles"
    twin.release()


# ---- sources, bands, capture --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_pitched_sources(case, dt):
    """U and V in plane-pitched views whose pad is NaN go into the call as they are: the bytes of the dense call, and no NaN."""
    import torch
    from mpassit_amd import regrid as R
    dt = torch.float64 if dt == "f64" else torch.float32
    nlev = 6
    for rh_u, rh_v, g, rot in ((case["E_all"], case["E_none"], case["tg"]["24x12"], case["rot_edge"]),
                               (case["E"], case["E"], case["tg"]["72x36"], case["rot_edge"])):
        ny, nx = g.lat.shape
        assert ny * nx == rh_u.n_src == rh_v.n_src
        du, dv = _winds(torch, rh_u, rh_v, nlev, dt, 8)
        _, pu = _pitched(torch, nlev, ny, nx, dt, ny * nx + 37)
        _, pv = _pitched(torch, nlev, ny, nx, dt, ny * nx + 5)
        pu.copy_(du.reshape(pu.shape))
        pv.copy_(dv.reshape(pv.shape))
        assert not pu.is_contiguous() and not pv.is_contiguous()
        for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
            for policy in POLICIES:
                want = _fused(R, policy, rh_u, rh_v, rot, du, dv, nlev, layout)
                got = _fused(R, policy, rh_u, rh_v, rot, pu, pv, nlev, layout)
                for x, w in zip(got, want):
                    assert _bytes_equal(x, w), "pitched sources differ from dense (their NaN pad was read?)"
                    assert not torch.isnan(x).any()
    with pytest.raises(ValueError):     # a strided view that is not plane-pitched is refused by the wrapper
        R.wind_csr_to_edges(rh_u, rh_v, rot[0], rot[1], pu.transpose(1, 2), pv, nlev)


def test_canaries(case):
    """Every result sits between NaN-filled bands: the bands stay untouched, in both layouts, with and without level chunks, for one
    result and for two, on the periodic handle and on the coarse one whose runs are staged in chunks."""
    import torch
    from mpassit_amd import regrid as R
    band = 4096
    for rh_u, rh_v, rot, levels in ((case["E_all"], case["E_none"], case["rot_edge"], ((55, torch.float32), (1, torch.float32))),
                                    (case["coarse"], case["coarse"], case["rot_coarse"], ((55, torch.float32), (64, torch.float64),
                                                                                         (129, torch.float64), (1, torch.float32)))):
        n = rh_u.n_dst
        for nlev, ddt in levels:
            u, v = _winds(torch, rh_u, rh_v, nlev, torch.float32, 90 + nlev)
            for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
                for policy in ("un", "both", "rotated"):
                    want = _fused(R, policy, rh_u, rh_v, rot, u, v, nlev, layout, ddt)
                    bufs = [torch.full((2 * band + nlev * n,), float("nan"), dtype=ddt, device="cuda") for _ in want]
                    outs = tuple(b[band:band + nlev * n] for b in bufs)
                    got = _fused(R, policy, rh_u, rh_v, rot, u, v, nlev, layout, outs=outs)
                    for x, o, b, w in zip(got, outs, bufs, want):
                        assert x.data_ptr() == o.data_ptr()
                        assert torch.isnan(b[:band]).all() and torch.isnan(b[band + nlev * n:]).all(), "a canary band was written"
                        assert _bytes_equal(b[band:band + nlev * n], w.reshape(-1))


def test_graph_capture_on_the_first_call(gpu_lib):
    """The very first wind_csr_to_edges / wind_csr_to_mesh on fresh handles are captured (after mpg_warmup_wait) and replayed twice: the
    bytes of the eager calls."""
    import torch
    from mpassit_amd import _lib as L, regrid as R, synth, target_grid as tg
    g = tg.define_target_grid_params("lat-lon", nx=37, ny=19, stand_lon=0.0, is_regional=False)
    m = synth.mesh_edges(synth.global_voronoi_mesh(3001))
    grid, mesh = R.Grid(g.lon, g.lat, periodic=L.GRID_PERIODIC_I), R.Mesh.from_mpas(m)
    rh = R.regrid_store_periodic_to_mesh(grid, mesh, meshloc=R.MESHLOC_EDGE)
    rn = R.regrid_store_periodic_to_mesh(grid, mesh, meshloc=R.MESHLOC_EDGE, pole_method=R.POLEMETHOD_NONE)
    cn, sn = R.mesh_edge_rotang(None, mesh)
    assert gpu_lib.load().mpg_warmup_wait() == 0
    nlev, n = 55, rh.n_dst
    assert n % 64 != 0 and (np.diff(rn.csr()[0]) == 0).any()
    u, v = _winds(torch, rh, rn, nlev, torch.float32, 5)
    lf = torch.full((n, nlev), float("nan"), dtype=torch.float32, device="cuda")
    cf = tuple(torch.full((nlev, n), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2))
    ms = tuple(torch.full((n, nlev), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):        # one stream: a chain, no parallel branches
            R.wind_csr_to_edges(rh, rh, cn, sn, u, v, nlev, layout=R.LAYOUT_LEV_FAST, outs=lf)
            R.wind_csr_to_edges(rh, rn, cn, sn, u, v, nlev, layout=R.LAYOUT_CELL_FAST, tangential=True, outs=cf)
            R.wind_csr_to_mesh(rn, rh, cn, sn, u, v, nlev, layout=R.LAYOUT_LEV_FAST, outs=ms)
    for trial in range(2):
        u.mul_(-0.5).add_(0.25)
        v.mul_(0.75).sub_(1.0)
        graph.replay()
        torch.cuda.synchronize()
        got = [lf.clone()] + [t.clone() for t in cf] + [t.clone() for t in ms]
        want_lf = R.wind_csr_to_edges(rh, rh, cn, sn, u, v, nlev, layout=R.LAYOUT_LEV_FAST)
        want_cf = R.wind_csr_to_edges(rh, rn, cn, sn, u, v, nlev, layout=R.LAYOUT_CELL_FAST, out_dtype=torch.float64, tangential=True)
        want_ms = R.wind_csr_to_mesh(rn, rh, cn, sn, u, v, nlev, layout=R.LAYOUT_LEV_FAST, out_dtype=torch.float64)
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
    rh_u, rh_v, (cn, sn) = case["E_all"], case["E_none"], case["rot_edge"]
    n = rh_u.n_dst
    src = torch.zeros(4 * n, dtype=torch.float64, device="cuda")
    r0 = torch.zeros(4 * n, dtype=torch.float64, device="cuda")
    r1 = torch.zeros_like(r0)
    fixed = R.regrid_store_to_mesh(case["ga"], case["mesh_over"])                       # a fixed 4-slot handle
    assert fixed.nnz_per_row == 4 and fixed.n_dst <= n and fixed.n_src <= n
    gp = R.Grid.from_target(tg.define_target_grid_params("lat-lon", nx=73, ny=37, stand_lon=0.0, is_regional=False))
    pole = R.regrid_store_grid(gp, R.STAGGERLOC_EDGE2)                                  # a handle with pole terms
    assert pole.pole()[0].size > 0 and pole.n_src <= n and pole.n_dst <= n
    cells = case["P"]
    assert cells.n_dst != n

    for call, who, twin, results in ((L.wind_csr_to_mesh_dev, "mpg_wind_csr_to_mesh", "mpg_wind_to_mesh_dev", "ue_dev and ve_dev"),
                                     (L.wind_csr_to_edges_dev, "mpg_wind_csr_to_edges", "mpg_wind_to_edges_dev", "un_dev and ut_dev")):
        edges = call is L.wind_csr_to_edges_dev

        def refused(rc, want, word=None):
            msg = lib.mpg_last_error().decode()
            assert rc == want and msg, (rc, want, msg)
            assert who in msg, msg
            if word:
                assert word in msg, msg

        def args(**kw):
            return [kw.get("hu", rh_u._h), kw.get("hv", rh_v._h), kw.get("c", cn.data_ptr()), kw.get("s", sn.data_ptr()), kw.get("u", src.data_ptr()),
                    kw.get("v", src.data_ptr()), kw.get("st", 0), kw.get("ldu", 0), kw.get("ldv", 0), kw.get("nlev", 2), kw.get("r0", r0.data_ptr()),
                    kw.get("r1", r1.data_ptr()), kw.get("dt", 0), kw.get("layout", 1), None]

        # MPG_ERR_UNSUPPORTED: the handle kinds and the big-endian types
        refused(call(*args(hu=fixed._h)), L.MPG_ERR_UNSUPPORTED, twin)
        refused(call(*args(hv=fixed._h)), L.MPG_ERR_UNSUPPORTED, "fixed")
        refused(call(*args(hu=pole._h, hv=pole._h)), L.MPG_ERR_UNSUPPORTED, "pole")
        refused(call(*args(hv=pole._h)), L.MPG_ERR_UNSUPPORTED, "mpg_handle_pole_count")
        refused(call(*args(st=2)), L.MPG_ERR_UNSUPPORTED, "big-endian")
        refused(call(*args(dt=3)), L.MPG_ERR_UNSUPPORTED, "big-endian")
        # MPG_ERR_INVALID_ARG
        refused(call(*args(hv=cells._h)), L.MPG_ERR_INVALID_ARG, "same points")
        if edges:
            refused(call(*args(c=None)), L.MPG_ERR_INVALID_ARG, "NULL")        # the angles are required
            refused(call(*args(s=None)), L.MPG_ERR_INVALID_ARG, "NULL")
            refused(call(*args(c=None, s=None)), L.MPG_ERR_INVALID_ARG, "NULL")
            assert call(*args(r1=None)) == 0                                    # ut_dev may be NULL
        else:
            refused(call(*args(c=None)), L.MPG_ERR_INVALID_ARG, "come together")
            refused(call(*args(s=None)), L.MPG_ERR_INVALID_ARG, "come together")
            assert call(*args(c=None, s=None)) == 0                             # both NULL: no rotation
            refused(call(*args(r1=None)), L.MPG_ERR_INVALID_ARG, "NULL")
        refused(call(*args(ldu=rh_u.n_src - 1)), L.MPG_ERR_INVALID_ARG, "u_level_stride")
        refused(call(*args(ldv=rh_v.n_src - 1)), L.MPG_ERR_INVALID_ARG, "v_level_stride")
        refused(call(*args(nlev=0)), L.MPG_ERR_INVALID_ARG, "nlev")
        refused(call(*args(layout=2)), L.MPG_ERR_INVALID_ARG, "dst_layout")
        refused(call(*args(st=4)), L.MPG_ERR_INVALID_ARG)
        refused(call(*args(dt=-1)), L.MPG_ERR_INVALID_ARG)
        refused(call(*args(hu=None)), L.MPG_ERR_INVALID_ARG, "NULL")
        refused(call(*args(hv=None)), L.MPG_ERR_INVALID_ARG, "NULL")
        refused(call(*args(u=None)), L.MPG_ERR_INVALID_ARG, "NULL")
        refused(call(*args(v=None)), L.MPG_ERR_INVALID_ARG, "NULL")
        refused(call(*args(r0=None)), L.MPG_ERR_INVALID_ARG, "NULL")
        refused(call(*args(r1=r0.data_ptr())), L.MPG_ERR_INVALID_ARG, "alias")
        refused(call(*args(r1=r0.data_ptr() + 8)), L.MPG_ERR_INVALID_ARG, results)
        refused(call(*args(r0=src.data_ptr())), L.MPG_ERR_INVALID_ARG, "alias")
        refused(call(*args(r1=src.data_ptr())), L.MPG_ERR_INVALID_ARG, "alias")
        big = torch.zeros_like(r0)          # angles in a block of their own, large enough that a result laid over it touches nothing else
        a0, a1 = big.data_ptr(), big.data_ptr() + 8 * n
        refused(call(*args(c=a0, s=a1, r0=a0)), L.MPG_ERR_INVALID_ARG, "angles")
        refused(call(*args(c=a0, s=a1, r1=a1)), L.MPG_ERR_INVALID_ARG, "angles")
        # ... and the same arguments without a fault are accepted: dense and strided, one handle twice
        assert call(*args()) == 0 and call(*args(ldu=rh_u.n_src, ldv=rh_v.n_src + 5)) == 0 and call(*args(hv=rh_u._h)) == 0
        torch.cuda.synchronize()

    # the two fixed-handle calls go on refusing a CSR handle, and name the call that takes it
    fu = R.regrid_store_to_mesh(case["ga"], case["mesh_over"], staggerloc=R.STAGGERLOC_EDGE1)
    ang = torch.zeros(max(n, fu.n_dst), dtype=torch.float64, device="cuda")
    for call, new in ((L.wind_to_mesh_dev, "mpg_wind_csr_to_mesh_dev"), (L.wind_to_edges_dev, "mpg_wind_csr_to_edges_dev")):
        for kw in (dict(hu=rh_u._h, hv=fu._h), dict(hu=fu._h, hv=rh_u._h), dict(hu=rh_u._h, hv=rh_u._h)):
            rc = call(kw["hu"], kw["hv"], ang.data_ptr(), ang.data_ptr(), src.data_ptr(), src.data_ptr(), 0, 0, 0, 2, r0.data_ptr(), r1.data_ptr(), 0, 1, None)
            msg = lib.mpg_last_error().decode()
            assert rc == L.MPG_ERR_UNSUPPORTED and "CSR" in msg and new in msg, (rc, msg)
    for rh in (fu, fixed, pole):
        rh.release()
    gp.destroy()
    # the wrappers' own checks
    u, v = _winds(torch, rh_u, rh_v, 2, torch.float64, 1)
    with pytest.raises(ValueError):
        R.wind_csr_to_edges(rh_u, rh_v, cn, None, u, v, 2)
    with pytest.raises(ValueError):
        R.wind_csr_to_mesh(rh_u, rh_v, cn, None, u, v, 2)
    with pytest.raises(ValueError):
        R.wind_csr_to_edges(rh_u, rh_v, cn, sn, u, v.float(), 2)
    with pytest.raises(ValueError):
        R.wind_csr_to_mesh(rh_u, rh_v, cn, sn, u[:1], v, 2)
    with pytest.raises(ValueError):
        R.wind_csr_to_edges(rh_u, rh_v, cn[:-1], sn[:-1], u, v, 2)
    with pytest.raises(ValueError):
        R.wind_csr_to_mesh(rh_u, rh_v, cn, sn, u, v, 2, outs=(torch.empty(2 * n, dtype=torch.float64, device="cuda"),))


def test_zero_size_paths(case):
    """A handle with no entries (from-weights with an empty list) on either side: every row is empty in it, so every result is +0.0."""
    import torch
    from mpassit_amd import regrid as R
    E = case["E_all"]
    none = R.RouteHandle.from_weights(E.n_src, E.n_dst, 1, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    assert none.nnz == 0 and none.nnz_per_row == 0 and none.n_dst == E.n_dst
    cn, sn = case["rot_edge"]
    nlev = 3
    u, v = _winds(torch, E, E, nlev, torch.float32, 3)
    for hu, hv in ((E, none), (none, E), (none, none)):
        for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
            outs = tuple(torch.full((nlev * E.n_dst,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2))
            for x in R.wind_csr_to_edges(hu, hv, cn, sn, u, v, nlev, layout=layout, tangential=True, outs=outs):
                assert bool((x.view(torch.int32) == 0).all())
            one = R.wind_csr_to_edges(hu, hv, cn, sn, u, v, nlev, layout=layout)
            assert bool((one.view(torch.int32) == 0).all())
            for x in R.wind_csr_to_mesh(hu, hv, None, None, u, v, nlev, layout=layout, out_dtype=torch.float64):
                assert bool((x.view(torch.int64) == 0).all())
    none.release()


# ---- the differentiable ops ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", ["one_twice", "two"])
@pytest.mark.parametrize("layout", ["cell_fast", "lev_fast"])
@pytest.mark.parametrize("op", ["mesh", "un", "both"])
def test_autograd_dot_product(case, op, layout, pair):
    """Float64 dot-product test: |<F(u, v), y> - <(u, v), F^T y>| <= 1e-11 * sum |terms| (the bar of test_autograd_dot_product in
    tests/test_wind_to_edges_gpu.py); the gradients have the inputs' dtypes and shapes.  With two handles some points have a row in one
    handle only, where the forward stores +0.0 and the backward must pass nothing."""
    import torch
    from mpassit_amd import regrid as R
    layout = R.LAYOUT_CELL_FAST if layout == "cell_fast" else R.LAYOUT_LEV_FAST
    if op == "mesh":
        rh_u, rh_v, rot = (case["P"], case["P"], case["rot_P"]) if pair == "one_twice" else (case["over_d"], case["over_f"], case["rot_over"])
    else:
        rh_u, rh_v, rot = (case["E"], case["E"], case["rot_edge"]) if pair == "one_twice" else (case["E_all"], case["E_none"], case["rot_edge"])
    nlev = 3
    u0, v0 = _winds(torch, rh_u, rh_v, nlev, torch.float64, 23)
    u, v = u0.clone().requires_grad_(True), v0.clone().requires_grad_(True)
    if op == "mesh":
        out = R.wind_csr_to_mesh_autograd(rh_u, rh_v, rot[0], rot[1], u, v, nlev, layout=layout)
        want = R.wind_csr_to_mesh(rh_u, rh_v, rot[0], rot[1], u0, v0, nlev, layout=layout)
    else:
        out = R.wind_csr_to_edges_autograd(rh_u, rh_v, rot[0], rot[1], u, v, nlev, layout=layout, tangential=op == "both")
        want = R.wind_csr_to_edges(rh_u, rh_v, rot[0], rot[1], u0, v0, nlev, layout=layout, tangential=op == "both")
    out, want = (out, want) if op != "un" else ((out,), (want,))
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


def test_autograd_no_rotation(case):
    """cosa = sina = None: the gradients are each handle's regrid_transpose of the incoming gradient, masked."""
    import torch
    from mpassit_amd import regrid as R
    rh_u, rh_v, nlev = case["over_d"], case["over_f"], 2
    u0, v0 = _winds(torch, rh_u, rh_v, nlev, torch.float64, 41)
    u, v = u0.clone().requires_grad_(True), v0.clone().requires_grad_(True)
    ue, ve = R.wind_csr_to_mesh_autograd(rh_u, rh_v, None, None, u, v, nlev)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(43)
    y0, y1 = (torch.randn(tuple(ue.shape), dtype=torch.float64, device="cuda", generator=gen) for _ in range(2))
    ((ue * y0).sum() + (ve * y1).sum()).backward()
    mapped = (~_empty(torch, rh_u, rh_v)).to(torch.float64)
    assert torch.equal(u.grad, rh_u.regrid_transpose((y0 * mapped).contiguous(), nlev=nlev).reshape(u.shape))
    assert torch.equal(v.grad, rh_v.regrid_transpose((y1 * mapped).contiguous(), nlev=nlev).reshape(v.shape))


def test_autograd_float32_and_points_mapped_in_one_handle(case):
    """float32 inputs get float32 gradients; an incoming gradient that is non-zero only on the 505 edges with a row in ONE handle passes
    exactly nothing."""
    import torch
    from mpassit_amd import regrid as R
    rh_u, rh_v, (cn, sn) = case["E_all"], case["E_none"], case["rot_edge"]
    nlev = 2
    u0, v0 = _winds(torch, rh_u, rh_v, nlev, torch.float32, 31)
    u, v = u0.clone().requires_grad_(True), v0.clone().requires_grad_(True)
    un, ut = R.wind_csr_to_edges_autograd(rh_u, rh_v, cn, sn, u, v, nlev, layout=R.LAYOUT_LEV_FAST, tangential=True)
    assert un.dtype == torch.float32 and tuple(un.shape) == (rh_u.n_dst, nlev) and tuple(ut.shape) == (rh_u.n_dst, nlev)
    one_only = torch.as_tensor(np.diff(rh_v.csr()[0]) == 0, device="cuda")
    assert int(one_only.sum()) == 505
    y = torch.zeros_like(un)
    y[one_only] = 1.0
    ((un * y).sum() + (ut * y).sum()).backward()
    assert u.grad.dtype == torch.float32 and v.grad.dtype == torch.float32 and u.grad.shape == u.shape and v.grad.shape == v.shape
    assert float(u.grad.abs().max()) == 0.0 and float(v.grad.abs().max()) == 0.0, "an edge mapped in one handle only passed a gradient"
    # ... and a gradient on the points mapped in both arrives: d(sum un)/du = A_u^T cn, d(sum un)/dv = A_v^T sn
    u.grad = None
    v.grad = None
    R.wind_csr_to_edges_autograd(rh_u, rh_v, cn, sn, u, v, nlev).sum().backward()
    both = (~one_only).to(torch.float64)
    want_u = rh_u.regrid_transpose((both * cn).float().expand(nlev, -1).contiguous(), nlev=nlev, out_dtype=torch.float32).reshape(u.shape)
    want_v = rh_v.regrid_transpose((both * sn).float().expand(nlev, -1).contiguous(), nlev=nlev, out_dtype=torch.float32).reshape(v.shape)
    assert torch.allclose(u.grad, want_u, rtol=1e-6, atol=1e-6) and torch.allclose(v.grad, want_v, rtol=1e-6, atol=1e-6)
    assert float(u.grad.abs().max()) > 0


# ---- a wind -------------------------------------------------------------------------------------------------------------------------------
def test_solid_body_rotation_onto_the_edges(case, oracle):
    """A solid-body rotation of unit speed about an axis tilted 45 degrees, sampled at the 72 x 36 centres as (u_east, v_north), taken to
    un on the edges through E.  The GPU result and the numpy reference's own (the weights of tests/_periodic_to_mesh_ref.py applied in
    numpy, then the rotation) agree to 1e-13: unit-speed winds, rows of 4 entries summing to 1, two products and a sum.  On quad rows the
    GPU's largest error against the analytic V . n does not exceed the reference's own by more than 1e-12 (1.41e-3 when this was
    written: information, not a constant of the test).  Cap rows get the row mean of each COMPONENT, which is not a wind: they are left
    out and their error is printed (0.53 when this was written)."""
    import torch
    from mpassit_amd import regrid as R
    m, g, E = case["m"], case["tg"]["72x36"], case["E"]
    axis = np.array([np.sin(np.pi / 4), 0.0, np.cos(np.pi / 4)])

    def frame(lon, lat):
        east = np.stack([-np.sin(lon), np.cos(lon), np.zeros_like(lon)], axis=1)
        north = np.stack([-np.sin(lat) * np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat)], axis=1)
        return east, north

    cen = oracle.lonlat_deg_to_xyz(g.lon, g.lat).reshape(g.lat.shape + (3,))
    pts = oracle.lonlat_deg_to_xyz(*oracle.mesh_coords_deg(m.lonEdge, m.latEdge))
    east, north = frame(np.radians(g.lon).reshape(-1), np.radians(g.lat).reshape(-1))
    vel = np.cross(axis, cen.reshape(-1, 3))
    ue, vn = (vel * east).sum(axis=1), (vel * north).sum(axis=1)
    assert np.abs(np.hypot(ue, vn) - np.linalg.norm(vel, axis=1)).max() < 1e-14
    e_e, e_n = frame(m.lonEdge, m.latEdge)
    normal = np.cos(m.angleEdge)[:, None] * e_e + np.sin(m.angleEdge)[:, None] * e_n
    exact = (np.cross(axis, pts) * normal).sum(axis=1)
    r = PR.periodic_to_mesh(oracle, cen, pts)
    rows = np.repeat(np.arange(m.nEdges), np.diff(r["rowptr"]))
    a = np.bincount(rows, weights=r["val"] * ue[r["col"]], minlength=m.nEdges)
    b = np.bincount(rows, weights=r["val"] * vn[r["col"]], minlength=m.nEdges)
    ref = a * np.cos(m.angleEdge) + b * np.sin(m.angleEdge)
    cn, sn = case["rot_edge"]
    u, v = (torch.as_tensor(x.reshape(1, -1), device="cuda") for x in (ue, vn))
    got = R.wind_csr_to_edges(E, E, cn, sn, u, v, 1).reshape(-1).cpu().numpy()
    quad, cap = r["kind"] == PR.KIND_QUAD, r["kind"] == PR.KIND_CAP
    assert int(cap.sum()) == 57 and int(quad.sum()) == m.nEdges - 57
    d = np.abs(got - ref).max()
    err_gpu, err_ref = np.abs(got - exact)[quad].max(), np.abs(ref - exact)[quad].max()
    print("un: |GPU - numpy reference| %.3g (bar 1e-13); quad rows: GPU error %.6g, reference's own %.6g; the 57 cap rows: GPU error %.3g"
          % (d, err_gpu, err_ref, np.abs(got - exact)[cap].max()))
    assert d <= 1e-13
    assert err_gpu <= err_ref + 1e-12
    assert 1e-5 < err_ref < 1e-2, "the reference's own error is not that of a 5-degree grid: the check's inputs are wrong"
