"""Handle composition on the GPU at small sizes (mpg_handle_compose, mpg_compose_weights_dev): rowptr, col and val BIT FOR BIT against the
numpy mirror target_grid.compose_csr for fixed, nearest, conservative, periodic and from-weights operands; rows longer than anything a
workgroup could hold and every block seam; the composite as an ordinary CSR handle under every consumer; the composite against the chain
of two applies within a per-point bound; value planes through the composition, twice and from a replayed graph; winds from edge-normal
u straight onto a Lambert grid; the refusals.

Operands:
  ico3     icosahedral_mesh(3), 642 cells, 1 920 edges, with edgesOnCell and the stand-in reconstruction coefficients
  cut      the same cells, verticesOnCell emptied for the cells more than CUT_DEG from the grid's centre: a limited-area cut-out whose
           cell ids are ico3's, so that the 37 x 23 Lambert grid (200 km) overhangs it and a good part of its points is unmapped
  per      a 24 x 12 global lat-lon grid, periodic in i (cap rows of 24 entries under POLEMETHOD_ALLAVG)
  ico2     icosahedral_mesh(2), 162 cells: the destination of the Mesh -> Mesh outer"""
import dataclasses
import os
import re

import numpy as np
import pytest

import _wind_reconstruct_helpers as H
from _wind_pair_helpers import _bytes_equal
from conftest import LAMBERT

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
CUT_DEG = 25.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("bil_rec", "near_cons", "cons_cons", "mesh_per", "weights")


def _csr_of(h):
    """(rowptr, col, val) of any handle without pole terms: a CSR one's own, a fixed one's slots with the -1 entries dropped"""
    from mpassit_amd import target_grid as tg
    return h.csr() if h.nnz_per_row == 0 else tg.fixed_to_csr(*h.weights())


def _from_csr(R, n_src, nx, ny, csr):
    rowptr, col, val = csr
    row = np.repeat(np.arange(1, rowptr.size, dtype=np.int32), np.diff(rowptr))
    return R.RouteHandle.from_weights(n_src, nx, ny, row, (np.asarray(col) + 1).astype(np.int32), val)


def _random_csr(rng, n_dst, n_src, lens):
    lens = np.asarray(lens, dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = rng.integers(0, n_src, int(lens.sum())).astype(np.int32)          # with repetition: duplicate columns in a row
    return rowptr, col, rng.uniform(-1.0, 1.0, col.size)


def _same_csr(got, want):
    assert np.array_equal(got[0], want[0]), "rowptr differs"
    assert np.array_equal(got[1], want[1]), "col differs"
    g, w = np.asarray(got[2]).reshape(-1), np.asarray(want[2]).reshape(-1)
    assert g.size == w.size and np.array_equal(g.view(np.int64), w.view(np.int64)), "%d of %d values differ" % ((g != w).sum(), g.size)


def _mirror(a, b):
    from mpassit_amd import target_grid as tg
    ca, cb = _csr_of(a), _csr_of(b)
    rowptr, col, vals = tg.compose_csr(ca[0], ca[1], ca[2], cb[0], cb[1], cb[2])
    return rowptr, col, vals[0]


def _abs_apply(csr, x):
    """|M| x for [lev][n_src] x >= 0, in numpy"""
    rowptr, col, val = csr
    row = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    return np.stack([np.bincount(row, weights=np.abs(val) * xk[col], minlength=rowptr.size - 1) for xk in x])


@pytest.fixture(scope="module")
def world(gpu_lib):
    from mpassit_amd import _lib as L, regrid as R, synth, target_grid as tg
    d = dict(pairs={}, comp={}, own=[])
    mc = d["mc"] = H.mesh_case(synth.icosahedral_mesh(3))
    m = mc["m"]
    g = d["g"] = tg.define_target_grid_params("lambert", 38, 24, dx=200000.0, dy=200000.0, **LAMBERT)
    r = synth.latlon_rad_to_xyz(m.latCell, m.lonCell)
    c0 = synth.latlon_rad_to_xyz(np.deg2rad([LAMBERT["ref_lat"]]), np.deg2rad([LAMBERT["ref_lon"]]))[0]
    far = r @ c0 < np.cos(np.deg2rad(CUT_DEG))
    voc = np.array(m.verticesOnCell, copy=True)
    voc[far] = 0
    d["near"] = int((~far).sum())
    gp = tg.define_target_grid_params("lat-lon", nx=25, ny=13, stand_lon=0.0, is_regional=False)
    obj = d["obj"] = dict(ico3=R.Mesh.from_mpas(m), cut=R.Mesh.from_mpas(dataclasses.replace(m, verticesOnCell=voc)),
                          ico2=R.Mesh.from_mpas(synth.icosahedral_mesh(2)), grid=R.Grid.from_target(g), per=R.Grid.from_target(gp))
    rec = d["rec"] = R.reconstruct_store(mc["n_on"], mc["eoc"], m.nEdges)
    bil = R.regrid_store(obj["cut"], obj["grid"], R.REGRIDMETHOD_BILINEAR)
    near = R.regrid_store(obj["ico3"], obj["grid"], R.REGRIDMETHOD_NEAREST_STOD)
    cons = R.regrid_store(obj["ico3"], obj["grid"], R.REGRIDMETHOD_CONSERVE)
    g2m = R.regrid_store_conserve_to_mesh(obj["grid"], obj["ico3"])
    m2m = R.regrid_store_mesh(obj["ico3"], obj["ico2"])
    per = R.regrid_store_periodic_to_mesh(obj["per"], obj["ico3"], pole_method=R.POLEMETHOD_ALLAVG)
    rng = np.random.default_rng(24)
    la, lb = rng.integers(0, 7, 30), rng.integers(0, 6, 50)
    la[[0, 11, 29]] = 0
    lb[[3, 4, 49]] = 0
    wa = _from_csr(R, 50, 30, 1, _random_csr(rng, 30, 50, la))
    wb = _from_csr(R, 40, 10, 5, _random_csr(rng, 50, 40, lb))
    d["pairs"] = dict(bil_rec=(bil, rec), near_cons=(near, g2m), cons_cons=(cons, g2m), mesh_per=(m2m, per), weights=(wa, wb))
    d["own"] += [rec, bil, near, cons, g2m, m2m, per, wa, wb]
    for name, (a, b) in d["pairs"].items():
        d["comp"][name] = R.compose(a, b)
    yield d
    for h in list(d["comp"].values()) + d["own"]:
        h.release()
    for k in ("ico3", "cut", "ico2", "grid", "per"):
        obj[k].destroy()


def test_the_operands_exercise_what_they_should(world):
    p = world["pairs"]
    bil, rec = p["bil_rec"]
    assert (world["g"].nx, world["g"].ny) == (37, 23) and bil.n_dst == 851 and bil.n_src == 642 == rec.n_dst and rec.n_src == 1920
    assert bil.nnz_per_row == 3 and rec.nnz_per_row == 0
    mapped = bil.weights()[0][:, 0] >= 0
    print("cut-out: %d of 642 cells keep their vertices; %d of 851 grid points mapped" % (world["near"], mapped.sum()))
    assert 100 <= mapped.sum() <= 751, "the grid overhangs the cut-out: mapped and unmapped points in numbers"
    near, g2m = p["near_cons"]
    idx, w = near.weights()
    assert near.nnz_per_row == 1 and (idx >= 0).all() and (w == 1.0).all()
    rp = g2m.csr()[0]
    assert g2m.nnz_per_row == 0 and g2m.n_src == 851 and g2m.n_dst == 642 and (np.diff(rp) == 0).sum() > 300 and (np.diff(rp) > 0).sum() > 20
    assert p["cons_cons"][0].nnz_per_row == 0 and p["cons_cons"][0].n_dst == 851
    m2m, per = p["mesh_per"]
    assert m2m.nnz_per_row == 3 and m2m.n_dst == 162 and per.nnz_per_row == 0 and per.n_src == 24 * 12 and per.pole()[0].size == 0
    lens = np.diff(per.csr()[0])
    assert set(lens.tolist()) == {4, 24}, "quad rows of 4 and cap rows of nx"
    wa, wb = p["weights"]
    ca, cb = wa.csr(), wb.csr()
    assert wa.nnz_per_row == 0 and wb.nnz_per_row == 0 and (np.diff(ca[0]) == 0).sum() >= 3 and (np.diff(cb[0]) == 0).sum() >= 3
    for rp_, col in ((ca[0], ca[1]), (cb[0], cb[1])):
        assert any(np.unique(col[rp_[i]:rp_[i + 1]]).size < rp_[i + 1] - rp_[i] for i in range(rp_.size - 1)), "duplicate columns in a row"


# ---- 1. the bits of the mirror ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_bits_of_the_mirror(world, name):
    a, b = world["pairs"][name]
    c = world["comp"][name]
    assert c.nnz_per_row == 0 and c.n_src == b.n_src and (c.n_dst, c.nx_dst, c.ny_dst) == (a.n_dst, a.nx_dst, a.ny_dst)
    want = _mirror(a, b)
    got = c.csr()
    print("%s: %d x %d, nnz %d, longest row %d, build %.3f ms" % (name, c.n_dst, c.n_src, c.nnz, np.diff(got[0]).max(initial=0), c.store_ms))
    assert c.nnz == want[1].size and c.nnz > 0 and c.store_ms > 0.0
    _same_csr(got, want)
    for i in range(c.n_dst):
        assert (np.diff(got[1][got[0][i]:got[0][i + 1]].astype(np.int64)) > 0).all()
    # rows of A that are empty, unmapped or reach only empty rows of B are empty, and only those
    ca, cb = _csr_of(a), _csr_of(b)
    blen = np.diff(cb[0])
    reach = np.array([blen[ca[1][ca[0][i]:ca[0][i + 1]]].sum() for i in range(a.n_dst)])
    assert np.array_equal(np.diff(got[0]) == 0, reach == 0)
    if name in ("bil_rec", "weights"):
        assert (reach == 0).any() and (reach > 0).any()
    # the same bytes from a second build, and to_esmf_weights is the composite in ESMF's form
    from mpassit_amd import regrid as R
    again = R.compose(a, b)
    _same_csr(again.csr(), got)
    again.release()
    row, col, S = c.to_esmf_weights()
    assert np.array_equal(col - 1, got[1]) and np.array_equal(S.view(np.int64), got[2].view(np.int64))
    assert np.array_equal(row - 1, np.repeat(np.arange(c.n_dst), np.diff(got[0])))


def test_nothing_on_either_side(world):
    from mpassit_amd import regrid as R
    wa, wb = world["pairs"]["weights"]
    none = np.empty(0, np.int32)
    za = R.RouteHandle.from_weights(50, 30, 1, none, none, np.empty(0))
    zb = R.RouteHandle.from_weights(40, 10, 5, none, none, np.empty(0))
    assert za.nnz == 0 and zb.nnz == 0
    for a, b in ((za, wb), (wa, zb), (za, zb)):
        c = R.compose(a, b)
        assert c.nnz == 0 and c.nnz_per_row == 0 and (c.n_dst, c.n_src) == (30, 40)
        rowptr, col, val = c.csr()
        assert (rowptr == 0).all() and col.size == 0
        import torch
        out = c.regrid_typed(torch.ones((2, 40), dtype=torch.float64, device="cuda"), nlev=2)
        assert bool((out.view(torch.int64) == 0).all())
        m = R.compose_weights(c, a, b, torch.ones((2, b.nnz), dtype=torch.float64, device="cuda"))
        assert tuple(m.shape) == (2, 0)
        c.release()
    za.release()
    zb.release()


# ---- 2. long rows and block seams ---------------------------------------------------------------------------------------------------------
def test_long_rows_and_block_seams(world, gpu_lib):
    """One row of 5 000 entries among short ones over an inner of 2 000 rows of 3: more than a workgroup could sort in LDS, whatever
    capacity the kernel states (compose_checks.h CO_LDS_ROW_ENTRIES), and the same bits whatever the blocks of destination rows are."""
    from mpassit_amd import regrid as R
    text = open(os.path.join(ROOT, "mpassit_amd", "csrc", "compose_checks.h")).read()
    cap = int(re.search(r"#define\s+CO_LDS_ROW_ENTRIES\s+(\d+)", text).group(1))
    long_row = 5000
    assert long_row > cap, "the long row must exceed the per-row LDS capacity"
    rng = np.random.default_rng(5)
    n_rows, n_mid, n_src = 41, 2000, 700
    lens = rng.integers(0, 9, n_rows)
    lens[17], lens[40], lens[0] = long_row, 0, 0
    a = _from_csr(R, n_mid, n_rows, 1, _random_csr(rng, n_rows, n_mid, lens))
    b = _from_csr(R, n_src, n_mid, 1, _random_csr(rng, n_mid, n_src, np.full(n_mid, 3)))
    assert a.nnz_per_row == 0 and b.nnz_per_row == 3 and np.diff(a.csr()[0]).max() == long_row
    want = _mirror(a, b)
    assert np.diff(want[0]).max() > 600, "the long row's composite row is long too"
    try:
        for block_rows in (0, 1, 7, 1000):
            gpu_lib.tune("compose_block_rows", block_rows)
            c = R.compose(a, b)
            print("compose_block_rows %d: nnz %d, build %.3f ms" % (block_rows, c.nnz, c.store_ms))
            _same_csr(c.csr(), want)
            c.release()
    finally:
        gpu_lib.tune("compose_block_rows", 0)
    with pytest.raises(gpu_lib.MpgError):
        gpu_lib.tune("compose_block_rows", -1)
    a.release()
    b.release()


# ---- 3. an ordinary handle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bil_rec", "mesh_per"])
def test_an_ordinary_handle(world, name):
    """Every consumer gives the bits it gives for RouteHandle.from_weights of the composite's csr()."""
    import torch
    from mpassit_amd import regrid as R
    c = world["comp"][name]
    twin = _from_csr(R, c.n_src, c.nx_dst, c.ny_dst, c.csr())
    assert twin.nnz_per_row == 0 and twin.nnz == c.nnz
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    for nlev in (1, 3, 5):
        x = torch.randn((nlev, c.n_src), dtype=torch.float64, device="cuda", generator=gen) * 7.0
        xt = x.t().contiguous()
        for src in (x, x.to(torch.float32)):
            for ddt in (torch.float64, torch.float32):
                for layout, s in ((R.LAYOUT_CELL_FAST, src), (R.LAYOUT_LEV_FAST, src.t().contiguous())):
                    assert _bytes_equal(c.regrid_typed(s, nlev=nlev, layout=layout, out_dtype=ddt), twin.regrid_typed(s, nlev=nlev, layout=layout, out_dtype=ddt))
                for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
                    assert _bytes_equal(c.regrid_csr_to_mesh(src, nlev=nlev, layout=layout, out_dtype=ddt),
                                        twin.regrid_csr_to_mesh(src, nlev=nlev, layout=layout, out_dtype=ddt))
                assert _bytes_equal(c.regrid_masked(src, nlev=nlev, out_dtype=ddt), twin.regrid_masked(src, nlev=nlev, out_dtype=ddt))
        assert _bytes_equal(c.regrid_csr_rows(xt, nlev=nlev), twin.regrid_csr_rows(xt, nlev=nlev))
        # float32 results are the cast of the float64 bits
        assert _bytes_equal(c.regrid_typed(x, nlev=nlev, out_dtype=torch.float32), c.regrid_typed(x, nlev=nlev, out_dtype=torch.float64).to(torch.float32))
        gy = torch.randn((nlev, c.n_dst), dtype=torch.float64, device="cuda", generator=gen)
        assert _bytes_equal(c.regrid_transpose(gy, nlev=nlev), twin.regrid_transpose(gy, nlev=nlev))
    # the differentiable op takes it
    x = torch.randn((2, c.n_src), dtype=torch.float64, device="cuda", generator=gen).requires_grad_(True)
    y = R.regrid_autograd(c, x, nlev=2)
    gy = torch.randn(y.shape, dtype=torch.float64, device="cuda", generator=gen)
    (y * gy).sum().backward()
    assert _bytes_equal(x.grad.reshape(2, -1), twin.regrid_transpose(gy.reshape(2, c.n_dst), nlev=2).reshape(2, -1))
    twin.release()


def test_the_longest_row_is_recorded(world, gpu_lib):
    """mpg_reconstruct_weights_dev reads the handle's longest row without a device read-back: it accepts the composite against maxEdges."""
    import torch
    from mpassit_amd import regrid as R
    c = world["comp"]["bil_rec"]
    longest = int(np.diff(c.csr()[0]).max())
    co = torch.zeros((c.n_dst, longest, 3), dtype=torch.float64, device="cuda")
    assert tuple(R.reconstruct_weights(c, co).shape) == (3, c.nnz)
    with pytest.raises(gpu_lib.MpgError) as e:
        R.reconstruct_weights(c, co[:, :longest - 1].contiguous())
    assert e.value.rc == gpu_lib.MPG_ERR_INVALID_ARG and "exceeds maxEdges" in str(e.value)


def test_released_operands(world):
    """The composite owns its arrays: outer and inner may be released before it is used."""
    import torch
    from mpassit_amd import regrid as R
    wa, wb = world["pairs"]["weights"]
    a, b = _from_csr(R, wa.n_src, wa.nx_dst, wa.ny_dst, wa.csr()), _from_csr(R, wb.n_src, wb.nx_dst, wb.ny_dst, wb.csr())
    c = R.compose(a, b)
    a.release()
    b.release()
    junk = [torch.full((1 << 16,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(4)]      # whatever takes the freed blocks
    _same_csr(c.csr(), world["comp"]["weights"].csr())
    x = torch.ones((1, c.n_src), dtype=torch.float64, device="cuda")
    assert _bytes_equal(c.regrid_typed(x), world["comp"]["weights"].regrid_typed(x))
    del junk
    c.release()


# ---- 4. against the chain -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlev", [1, 3, 5])
@pytest.mark.parametrize("name", CASES)
def test_against_the_chain(world, name, nlev):
    """C x in float64 against A (B x) through a float64 intermediate: |diff| <= (L_A + L_B + L_C + 8) 2^-53 S_i per point, S = |A| (|B| |x|)
    computed in numpy, L the longest rows: L_B + 1 and L_A + 1 roundings of the chain's two applies, those of the composite's values
    (at most L_A terms and products) and L_C + 1 of its apply, each relative to a partial sum that S bounds."""
    import torch
    a, b = world["pairs"][name]
    c = world["comp"][name]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(40 + nlev)
    x = torch.randn((nlev, c.n_src), dtype=torch.float64, device="cuda", generator=gen) * 10.0
    mid = b.regrid_typed(x, nlev=nlev, out_dtype=torch.float64).reshape(nlev, b.n_dst)
    chain = a.regrid_typed(mid.contiguous(), nlev=nlev, out_dtype=torch.float64).reshape(nlev, a.n_dst).cpu().numpy()
    comp = c.regrid_typed(x, nlev=nlev, out_dtype=torch.float64).reshape(nlev, c.n_dst).cpu().numpy()
    ca, cb, cc = _csr_of(a), _csr_of(b), c.csr()
    L = [int(np.diff(z[0]).max(initial=0)) for z in (ca, cb, cc)]
    S = _abs_apply(ca, _abs_apply(cb, np.abs(x.cpu().numpy())))
    bound = (sum(L) + 8) * EPS * S
    diff = np.abs(comp - chain)
    worst = float((diff / np.maximum(bound, 1e-300)).max())
    print("%s L%d: longest rows A %d B %d C %d; max |diff| %.3e, largest |diff| / bound %.3f" % (name, nlev, L[0], L[1], L[2], diff.max(), worst))
    assert (diff <= bound).all()
    assert (comp[:, S[0] == 0.0] == 0.0).all() and np.abs(comp).max() > 0.0


# ---- 5. planes ----------------------------------------------------------------------------------------------------------------------------
def _rec_planes(world):
    from mpassit_amd import regrid as R
    mc, rec = world["mc"], world["rec"]
    m = mc["m"]
    return R.reconstruct_weights(rec, mc["coeffs"], R.sphere_frames(m.lonCell, m.latCell)), R.reconstruct_weights(rec, mc["coeffs"])


def test_planes(world):
    import torch
    from mpassit_amd import regrid as R, target_grid as tg
    for name in CASES:                                           # K = 1 with inner's own values: the composite's values
        a, b = world["pairs"][name]
        if b.nnz_per_row:
            continue
        c = world["comp"][name]
        own = torch.as_tensor(b.csr()[2], device="cuda").reshape(1, -1)
        got = R.compose_weights(c, a, b, own)
        assert tuple(got.shape) == (1, c.nnz)
        assert np.array_equal(got.cpu().numpy()[0].view(np.int64), c.csr()[2].view(np.int64)), name
    a, rec = world["pairs"]["bil_rec"]
    c = world["comp"]["bil_rec"]
    ca, cb = _csr_of(a), rec.csr()
    for m_in in _rec_planes(world):                              # K = 2 (frames) and K = 3 (X, Y, Z)
        want = tg.compose_csr(ca[0], ca[1], ca[2], cb[0], cb[1], m_in.cpu().numpy())[2]
        got = R.compose_weights(c, a, rec, m_in)
        assert got.shape == want.shape == (m_in.shape[0], c.nnz) and (want != 0.0).any()
        assert np.array_equal(got.cpu().numpy().view(np.int64), want.view(np.int64)), "%d values differ" % (got.cpu().numpy() != want).sum()
        assert _bytes_equal(got, R.compose_weights(c, a, rec, m_in))
    # K = 4, and a CSR outer
    a, b = world["pairs"]["weights"]
    c = world["comp"]["weights"]
    ca, cb = a.csr(), b.csr()
    planes = torch.as_tensor(np.random.default_rng(8).uniform(-1.0, 1.0, (4, b.nnz)), device="cuda")
    want = tg.compose_csr(ca[0], ca[1], ca[2], cb[0], cb[1], planes.cpu().numpy())[2]
    assert np.array_equal(R.compose_weights(c, a, b, planes).cpu().numpy().view(np.int64), want.view(np.int64))


def test_planes_in_a_graph_from_the_first_call(world, gpu_lib):
    """The very first mpg_compose_weights_dev calls on a fresh composite are captured on one stream and replayed twice: the eager bytes."""
    import torch
    from mpassit_amd import _lib as L, regrid as R
    a, rec = world["pairs"]["bil_rec"]
    c = R.compose(a, rec)
    assert gpu_lib.load().mpg_warmup_wait() == 0
    m2, m3 = (t.clone() for t in _rec_planes(world))
    o2, o3 = (torch.full((k, c.nnz), float("nan"), dtype=torch.float64, device="cuda") for k in (2, 3))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):        # one stream: a chain, no parallel branches
            s = torch.cuda.current_stream().cuda_stream
            assert L.compose_weights_dev(c._h, a._h, rec._h, 2, m2.data_ptr(), o2.data_ptr(), s) == 0
            assert L.compose_weights_dev(c._h, a._h, rec._h, 3, m3.data_ptr(), o3.data_ptr(), s) == 0
    for trial in range(2):
        m2.mul_(-0.5).add_(0.125)
        m3.mul_(1.5)
        graph.replay()
        torch.cuda.synchronize()
        assert not torch.isnan(o2).any() and not torch.isnan(o3).any()
        assert _bytes_equal(o2, R.compose_weights(c, a, rec, m2)) and _bytes_equal(o3, R.compose_weights(c, a, rec, m3))
    c.release()


# ---- 6. winds end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlev", [1, 3, 5])
def test_winds_from_edges_onto_the_grid(world, nlev):
    """The solid-body u through the composite (edges -> grid, one pass) against the chain (wind_reconstruct at the cells, then one Regrid
    per component), within the bound of test_against_the_chain with B's values m_k; and no further from the exact wind than the chain is
    plus that bound, on the grid's mapped points."""
    import torch
    from mpassit_amd import regrid as R, synth
    mc, rec, g = world["mc"], world["rec"], world["g"]
    a = world["pairs"]["bil_rec"][0]
    c = world["comp"]["bil_rec"]
    m3 = _rec_planes(world)[1]
    mc3 = R.compose_weights(c, a, rec, m3)
    scale = np.array([1.0, -0.5, 0.25, 2.0, -1.0])[:nlev]
    u = np.ascontiguousarray(mc["u"][:, None] * scale[None, :])                               # [edge][lev], file order
    ud = torch.as_tensor(u, device="cuda")
    comp = np.stack([t.cpu().numpy() for t in R.wind_reconstruct(c, mc3, ud, nlev, out_dtype=torch.float64)])       # [3][lev][ny * nx]
    cells = R.wind_reconstruct(rec, m3, ud, nlev, out_dtype=torch.float64)
    chain = np.stack([a.regrid_typed(t.contiguous(), nlev=nlev, out_dtype=torch.float64).reshape(nlev, -1).cpu().numpy() for t in cells])
    assert comp.shape == chain.shape == (3, nlev, 851)
    ca, cb, cc = _csr_of(a), rec.csr(), c.csr()
    L = [int(np.diff(z[0]).max()) for z in (ca, cb, cc)]
    mapped = a.weights()[0][:, 0] >= 0
    xyz = synth.latlon_rad_to_xyz(np.deg2rad(g.lat).reshape(-1), np.deg2rad(g.lon).reshape(-1))
    exact = np.cross(H.AXIS, xyz).T                                                           # [3][ny * nx]
    for k in range(3):
        S = _abs_apply(ca, _abs_apply((cb[0], cb[1], m3[k].cpu().numpy()), np.abs(u.T)))
        bound = (sum(L) + 8) * EPS * S
        diff = np.abs(comp[k] - chain[k])
        assert (diff <= bound).all(), "component %d: %.3e over" % (k, (diff - bound).max())
        e_comp, e_chain = np.abs(comp[k][0] - exact[k]), np.abs(chain[k][0] - exact[k])
        print("L%d component %d: composite against chain %.3e; against the exact wind %.3e (chain %.3e) on %d mapped points" % (
            nlev, k, diff.max(), e_comp[mapped].max(), e_chain[mapped].max(), mapped.sum()))
        assert (e_comp[mapped] <= e_chain[mapped] + bound[0][mapped]).all()
        assert (comp[k][:, ~mapped] == 0.0).all()
    assert np.abs(comp[:, 0][:, mapped]).max() > 0.3


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(world, gpu_lib):
    import ctypes as C
    import torch
    from mpassit_amd import _lib as L, regrid as R, target_grid as tg
    lib = L.load()
    a, rec = world["pairs"]["bil_rec"]
    c = world["comp"]["bil_rec"]
    wa, wb = world["pairs"]["weights"]
    gp = R.Grid.from_target(tg.define_target_grid_params("lat-lon", nx=73, ny=37, stand_lon=0.0, is_regional=False))
    pole = R.regrid_store_grid(gp, R.STAGGERLOC_EDGE2)                                  # a handle with pole terms
    assert pole.pole()[0].size > 0
    one = np.ones(1, np.int32)
    after_pole = R.RouteHandle.from_weights(pole.n_dst, 1, 1, one, one, np.ones(1))     # chains as an outer of `pole`
    before_pole = R.RouteHandle.from_weights(5, pole.n_src, 1, one, one, np.ones(1))    # ... as an inner
    h = C.c_void_p()

    def refused(rc, want, who, *words):
        msg = lib.mpg_last_error().decode()
        assert rc == want and msg, (rc, want, msg)
        assert who in msg, msg
        for word in words:
            assert word in msg, msg

    who = "mpg_handle_compose"
    refused(L.handle_compose(None, rec._h, C.byref(h)), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(L.handle_compose(a._h, None, C.byref(h)), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(L.handle_compose(a._h, rec._h, None), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(L.handle_compose(rec._h, a._h, C.byref(h)), L.MPG_ERR_INVALID_ARG, who, "n_dst = 851", "n_src = 1920")
    loc = _from_csr(R, a.n_src, a.nx_dst, a.ny_dst, _csr_of(a))
    loc.localize()
    assert loc.n_src < a.n_src
    refused(L.handle_compose(loc._h, rec._h, C.byref(h)), L.MPG_ERR_INVALID_ARG, who, "n_dst = 642", "n_src = %d" % loc.n_src, "localized")
    refused(L.handle_compose(pole._h, before_pole._h, C.byref(h)), L.MPG_ERR_UNSUPPORTED, who, "`outer`", "mpg_handle_pole_count > 0")
    refused(L.handle_compose(after_pole._h, pole._h, C.byref(h)), L.MPG_ERR_UNSUPPORTED, who, "`inner`", "mpg_handle_from_weights")
    assert h.value is None, "a refused call leaves *out alone"

    who = "mpg_compose_weights"
    m3 = _rec_planes(world)[1]
    out = torch.zeros((4, c.nnz), dtype=torch.float64, device="cuda")

    def call(composed=c, outer=a, inner=rec, k=3, bm=m3.data_ptr(), m=out.data_ptr()):
        return L.compose_weights_dev(composed._h if composed is not None else None, outer._h if outer is not None else None,
                                     inner._h if inner is not None else None, k, bm, m, None)
    assert call() == 0
    refused(call(composed=None), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(outer=None), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(inner=None), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(bm=None), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(m=None), L.MPG_ERR_INVALID_ARG, who, "NULL")
    refused(call(k=0), L.MPG_ERR_INVALID_ARG, who, "1..4")
    refused(call(k=5), L.MPG_ERR_INVALID_ARG, who, "1..4")
    refused(call(inner=a), L.MPG_ERR_UNSUPPORTED, who, "fixed", "mpg_handle_get_weights", "mpg_handle_from_weights")
    refused(call(composed=a), L.MPG_ERR_UNSUPPORTED, who, "`composed` is a fixed")
    refused(call(composed=pole), L.MPG_ERR_UNSUPPORTED, who, "pole")
    refused(call(outer=pole), L.MPG_ERR_UNSUPPORTED, who, "pole")
    refused(call(inner=pole), L.MPG_ERR_UNSUPPORTED, who, "pole")
    refused(call(composed=world["comp"]["weights"]), L.MPG_ERR_INVALID_ARG, who, "chain")
    refused(call(outer=wa), L.MPG_ERR_INVALID_ARG, who, "chain")
    refused(call(inner=wb), L.MPG_ERR_INVALID_ARG, who, "chain")
    refused(call(m=m3.data_ptr()), L.MPG_ERR_INVALID_ARG, who, "alias")
    refused(call(m=m3.data_ptr() + 8 * (3 * rec.nnz - 1)), L.MPG_ERR_INVALID_ARG, who, "alias")
    # the wrappers' own checks
    with pytest.raises(ValueError):
        R.compose_weights(c, a, rec, m3[:, :-1])
    with pytest.raises(ValueError):
        R.compose_weights(c, a, rec, m3.to(torch.float32))
    # the library still works afterwards
    torch.cuda.synchronize()
    again = R.compose(a, rec)
    _same_csr(again.csr(), c.csr())
    for x in (again, loc, after_pole, before_pole, pole):
        x.release()
    gp.destroy()
