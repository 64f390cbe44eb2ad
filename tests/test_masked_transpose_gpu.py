"""The adjoint of the masked Regrid (mpg_regrid_masked_transpose_dev, RouteHandle.regrid_masked_transpose, regrid_masked_autograd) held
to its header contract by identity: every output and every element of the workspace compared as bits with the host restatement of
tests/_masked_transpose_ref.py, on the smallest handles that reach every kernel path -- the synthetic from-weights handle whose transposed
segments sit either side of the 4-slot form, TR_SHORT and a wave, and store-made 3-, 1- and 4-slot and CSR handles of a 2 500-cell mesh
under a 61 x 37 grid -- at 1, 3 and 65 levels (65 crosses the 64-level LDS chunks), 1 and 2 fields, both layouts and float32 / float64
on each of g, src and dst."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _contract_ref as cr
from _masked_transpose_ref import jacobian_product, masked_transpose_ref

pytestmark = pytest.mark.gpu

SENTINEL = -9999.0                      # a float32 value: float32 and float64 sources then hold equal values
HANDLES = ["synthetic", "bilinear", "nearest", "grid4", "conserve", "to_mesh_conserve"]
NLEVS = [1, 3, 65]
# (gap modes, min_valid_frac, scale)
CONFIGS = [(("nan",), 0.5, 1.0), (("value", "mask"), 0.0, -2.5), (("nan", "value", "mask"), 1.0, 1.0)]


@pytest.fixture(scope="module")
def handles(gpu_lib):
    """{name: (RouteHandle, Pattern)}"""
    from conftest import LAMBERT
    from mpassit_amd import regrid as R, synth, target_grid as tg
    g = tg.define_target_grid_params("lambert", 62, 38, dx=60000.0, dy=60000.0, **LAMBERT)
    gc = tg.define_target_grid_params("lambert", 16, 10, dx=240000.0, dy=240000.0, **LAMBERT)   # coarse: a grid cell meets tens of mesh cells
    m = synth.regional_mesh_for_lambert(g.proj, 54, 31, 2500, margin=0.0)
    mesh, grid, coarse = R.Mesh.from_mpas(m), R.Grid.from_target(g), R.Grid.from_target(gc)
    (row, col, S), pat = cr.synthetic_transpose_case()
    h = {"synthetic": R.RouteHandle.from_weights(cr.SYN_N_SRC, cr.SYN_NX, cr.SYN_NY, row, col, S),
         "bilinear": R.regrid_store(mesh, grid, R.REGRIDMETHOD_BILINEAR),
         "nearest": R.regrid_store(mesh, grid, R.REGRIDMETHOD_NEAREST_STOD),
         "grid4": R.regrid_store_grid(grid, R.STAGGERLOC_EDGE1),
         "conserve": R.regrid_store(mesh, grid, R.REGRIDMETHOD_CONSERVE),
         "to_mesh_conserve": R.regrid_store_conserve_to_mesh(coarse, mesh)}
    assert [h[k].nnz_per_row for k in HANDLES] == [0, 3, 1, 4, 0, 0]
    out = {k: (rh, cr.Pattern.of(rh)) for k, rh in h.items()}
    got = out["synthetic"][1]
    assert np.array_equal(got.rowptr, pat.rowptr) and np.array_equal(got.col, pat.col) and np.array_equal(got.val, pat.val)
    assert sorted(set(cr.SYN_LENGTHS) - set(cr.segment_lengths(pat))) == [], "the synthetic handle holds every listed segment length"
    assert cr.segment_lengths(out["to_mesh_conserve"][1]).max() > 16, "the coarse grid's cells have long transposed segments"
    assert out["bilinear"][1].unmapped.any() and not out["grid4"][1].unmapped.all()
    yield out
    for rh in h.values():
        rh.release()
    mesh.destroy()
    grid.destroy()
    coarse.destroy()


def _gaps(pat, nlev, nf, modes, seed):
    """-> (src (nf, nlev, n_src) float64 holding float32 values, `missing` argument, (nan, missing_value) of the reference, mask or None).
    NaN on 30 % of the elements i.i.d., the sentinel on 15 %, a static mask on 20 % of the sources; from three levels on, level 1 is
    entirely missing and level 2 has no gaps (the static mask still covers its sources)."""
    rng = np.random.default_rng(7000 + 13 * nlev + seed)
    clean = cr.to_f32(cr.ordinary(pat.n_src, nlev, nf, seed)).astype(np.float64)
    x = clean.copy()
    nan, mv, missing, mask = False, None, [], None
    if "nan" in modes:
        x[rng.uniform(size=x.shape) < 0.3] = np.nan
        nan = True
        missing.append("nan")
    if "value" in modes:
        x[rng.uniform(size=x.shape) < 0.15] = SENTINEL
        mv = SENTINEL
        missing.append(SENTINEL)
    if "mask" in modes:
        mask = rng.uniform(size=pat.n_src) < 0.2
    if nlev >= 3 and missing:
        x[:, 1] = np.nan if nan else SENTINEL
        x[:, 2] = clean[:, 2]
    return x, (tuple(missing) if missing else None), (nan, mv), mask


def _gradient(pat, nlev, nf, defined, seed):
    """special_g as float32 values (so that both types hold equal values), a NaN planted at every undefined and unmapped output"""
    g, _, _ = cr.special_g(pat, nlev, nf, seed)
    g = cr.to_f32(g).astype(np.float64)
    g[~defined] = np.nan
    return g


def _dev(x, f32=False):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(x), device="cuda")
    return t.float() if f32 else t


def _call(rh, g, src, nlev, nf, lev_fast, g32, s32, d32, missing, mask, frac, scale, pitch=0):
    """-> (dst, work) as numpy; src (nf, nlev, n_src) values, laid out here"""
    import torch
    gt = _dev(g, g32)
    if pitch:
        ld = rh.n_dst + pitch
        base = torch.full((nf * nlev * ld,), float("nan"), dtype=gt.dtype, device="cuda")
        view = base.as_strided((nf, nlev, rh.ny_dst, rh.nx_dst), (nlev * ld, ld, rh.nx_dst, 1))
        view.copy_(gt.reshape(nf, nlev, rh.ny_dst, rh.nx_dst))
        gt = view
        assert not gt.is_contiguous()
    st = _dev(src, s32)
    if lev_fast:
        st = st.transpose(1, 2).contiguous()
    mt = None if mask is None else torch.as_tensor(mask, device="cuda")
    work = torch.full((nf, nlev, rh.n_dst), -7.0, dtype=torch.float64, device="cuda")
    dst = rh.regrid_masked_transpose(gt, st.reshape(-1), nlev=nlev, nfields=nf, layout=int(lev_fast), missing=missing, src_mask=mt,
                                     min_valid_frac=frac, scale=scale, out_dtype=torch.float32 if d32 else torch.float64, work=work)
    torch.cuda.synchronize()
    assert tuple(dst.shape) == ((nf, rh.n_src, nlev) if lev_fast else (nf, nlev, rh.n_src))
    return dst.cpu().numpy(), work.cpu().numpy()


def _reference(pat, g, src, nlev, nf, ref_missing, mask, frac, scale):
    """{(d32, lev_fast): dst}, h, defined -- once per case, shared by every type and layout combination"""
    nan, mv = ref_missing
    out = {}
    for d32, lf in itertools.product((False, True), (False, True)):
        out[d32, lf], h, defined = masked_transpose_ref(pat, g, src, nlev, nf, nan, mv, mask, frac, scale, np.float32 if d32 else np.float64, lf)
    return out, h, defined


def _defined(pat, src, nlev, nf, ref_missing, mask, frac):
    from _masked_transpose_ref import weight_sums
    return np.stack([weight_sums(pat, src[f], ref_missing[0], ref_missing[1], mask, frac)[2] for f in range(nf)])


# ---- 1, 3, 4: the contract, bit for bit, on every handle, shape, gap mode, type and layout ------------------------------------------------
@pytest.mark.parametrize("nlev", NLEVS)
@pytest.mark.parametrize("name", HANDLES)
def test_bits_of_the_contract(handles, name, nlev):
    rh, pat = handles[name]
    nf = 2
    for ci, (modes, frac, scale) in enumerate(CONFIGS):
        src, missing, ref_missing, mask = _gaps(pat, nlev, nf, modes, ci)
        defined = _defined(pat, src, nlev, nf, ref_missing, mask, frac)
        g = _gradient(pat, nlev, nf, defined, ci)
        want, h, d2 = _reference(pat, g, src, nlev, nf, ref_missing, mask, frac, scale)
        assert np.array_equal(d2, defined) and np.isnan(g[~defined]).all() and (~defined).any() and defined.any()
        assert (cr.bits(h[~defined]) == 0).all()
        if scale != 1.0:                                               # the scale is part of h
            unit = masked_transpose_ref(pat, g, src, nlev, nf, ref_missing[0], ref_missing[1], mask, frac, 1.0)[1]
            assert cr.differs(h, unit)[defined].mean() > 0.5
        ok = np.stack([~np.isnan(src[f]) if ref_missing[0] else np.ones(src[f].shape, bool) for f in range(nf)])
        ok &= src != SENTINEL if ref_missing[1] is not None else True
        ok &= ~mask[None, None, :] if mask is not None else True
        tag0 = "%s nlev %d %s frac %g scale %g" % (name, nlev, "+".join(modes), frac, scale)
        print("%s: %.1f %% of the outputs undefined, %.1f %% of the sources invalid" % (tag0, 100 * (~defined).mean(), 100 * (~ok).mean()))
        for lf, g32, s32, d32 in itertools.product((False, True), (False, True), (False, True), (False, True)):
            tag = "%s lev_fast %d g32 %d src32 %d dst32 %d" % (tag0, lf, g32, s32, d32)
            dst, work = _call(rh, g, src, nlev, nf, lf, g32, s32, d32, missing, mask, frac, scale)
            bad = cr.differs(dst, want[d32, lf])
            assert not bad.any(), "%s: %d outputs differ from the reference, first %s: got %r want %r" % (
                tag, int(bad.sum()), np.argwhere(bad)[0], dst[bad][0], want[d32, lf][bad][0])
            bad = cr.differs(work, h)
            assert not bad.any(), "%s: %d elements of the workspace differ, first %s: got %r want %r" % (
                tag, int(bad.sum()), np.argwhere(bad)[0], work[bad][0], h[bad][0])
            okl = ok.transpose(0, 2, 1) if lf else ok
            assert (cr.bits(dst[~okl]) == 0).all(), tag + ": an invalid source is not exactly +0.0"
            if (lf, g32, s32) == (False, False, False):
                for f in range(nf):                                # nfields batching: single calls give the batch's slices
                    one, w1 = _call(rh, g[f:f + 1], src[f:f + 1], nlev, 1, lf, g32, s32, d32, missing, mask, frac, scale)
                    assert cr.same(one[0], dst[f]) and cr.same(w1[0], work[f]), tag + ": nfields=2 differs from single calls"
        # no NaN of g at a filled output reaches a source: with finite values at the defined outputs the result is finite
        gf = np.where(defined & ~(np.abs(g) < 1e30), 1.0, g)
        dst, work = _call(rh, gf, src, nlev, nf, False, False, False, False, missing, mask, frac, scale)
        assert np.isnan(gf).any() and np.isfinite(dst).all() and np.isfinite(work).all(), tag0 + ": a NaN of g at a filled output spread"


@pytest.mark.parametrize("name", ["synthetic", "bilinear"])
def test_pitched_gradient(handles, name):
    rh, pat = handles[name]
    nlev, nf = 3, 2
    modes, frac, scale = CONFIGS[2]
    src, missing, ref_missing, mask = _gaps(pat, nlev, nf, modes, 5)
    g = _gradient(pat, nlev, nf, _defined(pat, src, nlev, nf, ref_missing, mask, frac), 5)
    want, h, _ = _reference(pat, g, src, nlev, nf, ref_missing, mask, frac, scale)
    for lf, g32 in itertools.product((False, True), (False, True)):
        dst, work = _call(rh, g, src, nlev, nf, lf, g32, False, False, missing, mask, frac, scale, pitch=3)   # the pad holds NaN
        assert cr.same(dst, want[False, lf]) and cr.same(work, h), "%s lev_fast %d g32 %d: a pitched gradient changes the result" % (name, lf, g32)


# ---- 2: nothing missing, scale 1, finite g: the unmasked transpose ----------------------------------------------------------------------
@pytest.mark.parametrize("name", HANDLES)
def test_no_gaps_is_regrid_transpose(handles, name):
    import torch
    rh, pat = handles[name]
    nf = 2
    for nlev in NLEVS:
        g = cr.to_f32(cr.ordinary(pat.n_dst, nlev, nf, 3)).astype(np.float64)
        src = cr.ordinary(pat.n_src, nlev, nf, 4)
        for lf, g32, d32 in itertools.product((False, True), (False, True), (False, True)):
            dst, work = _call(rh, g, src, nlev, nf, lf, g32, False, d32, "nan", None, 0.5, 1.0)
            want = rh.regrid_transpose(_dev(g, g32), nlev=nlev, nfields=nf, layout=int(lf), out_dtype=torch.float32 if d32 else torch.float64)
            assert cr.same(dst, want.cpu().numpy()), "%s nlev %d lev_fast %d g32 %d dst32 %d: differs from regrid_transpose" % (name, nlev, lf, g32, d32)
            assert cr.same(work[:, :, ~pat.unmapped], g[:, :, ~pat.unmapped]), name + ": h is not (double)g on the mapped points"
            assert (cr.bits(work[:, :, pat.unmapped]) == 0).all()


# ---- 5: the torch op ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["synthetic", "bilinear", "conserve"])
def test_autograd_is_the_direct_call(handles, name):
    import torch
    from mpassit_amd import regrid as R
    rh, pat = handles[name]
    nlev, nf = 3, 2
    modes, frac, _ = CONFIGS[0]
    src, missing, ref_missing, mask = _gaps(pat, nlev, nf, ("nan", "mask"), 9)
    defined = _defined(pat, src, nlev, nf, ref_missing, mask, frac)
    g = _gradient(pat, nlev, nf, defined, 9)
    mt = torch.as_tensor(mask, device="cuda")
    for lf, f32 in itertools.product((False, True), (False, True)):
        x = _dev(src, f32)
        x = (x.transpose(1, 2).contiguous() if lf else x).requires_grad_(True)
        out = R.regrid_masked_autograd(rh, x, nlev=nlev, nfields=nf, layout=int(lf), missing=missing, src_mask=mt, min_valid_frac=frac)
        assert out.dtype == x.dtype and np.array_equal(~np.isnan(out.detach().cpu().numpy().reshape(nf, nlev, -1)), defined)
        gt = _dev(g, f32).reshape(out.shape)
        out.backward(gt)
        direct = rh.regrid_masked_transpose(gt, x.detach().reshape(-1), nlev=nlev, nfields=nf, layout=int(lf), missing=missing, src_mask=mt,
                                            min_valid_frac=frac, out_dtype=x.dtype)
        torch.cuda.synchronize()
        assert x.grad.shape == x.shape and x.grad.dtype == x.dtype
        assert cr.same(x.grad.cpu().numpy().reshape(-1), direct.cpu().numpy().reshape(-1)), "%s lev_fast %d f32 %d" % (name, lf, f32)
        assert not torch.isnan(x.grad[torch.isnan(x.detach())]).any(), "the gradient at a missing source is 0, not NaN"


def test_autograd_matches_the_dense_jacobian(handles):
    """float64 on the synthetic handle: loss.backward() against J^T g of tests/test_masked_transpose_cpu.py, within its bound"""
    import torch
    from mpassit_amd import regrid as R
    from _masked_transpose_ref import CASE_NLEV as NLEV, gappy_case
    rh, _ = handles["synthetic"]
    pat, src, mask, g, defined = gappy_case()
    want, bound, ok = jacobian_product(pat, g, src, NLEV, src_mask=mask, min_valid_frac=0.5)
    x = _dev(src).requires_grad_(True)
    out = R.regrid_masked_autograd(rh, x, nlev=NLEV, src_mask=torch.as_tensor(mask, device="cuda"))
    loss = (out.reshape(NLEV, -1)[torch.as_tensor(defined, device="cuda")] * _dev(g[defined])).sum()
    loss.backward()
    got = x.grad.cpu().numpy()
    assert (cr.bits(got[~ok]) == 0).all() and not np.isnan(got).any()
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    assert (err <= bound).all(), "%d gradients outside the bound, worst %r over its bound" % (int((err > bound).sum()), float((err / np.maximum(bound, 1e-300)).max()))


# ---- 6: refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(handles):
    import torch
    from mpassit_amd import _lib as L, regrid as R, target_grid as T
    rh, _ = handles["bilinear"]
    nlev = 2
    g = torch.zeros((nlev, rh.n_dst), dtype=torch.float64, device="cuda")
    src = torch.zeros((nlev, rh.n_src), dtype=torch.float64, device="cuda")
    dst = torch.full((nlev, rh.n_src), 777.0, dtype=torch.float64, device="cuda")
    work = torch.full((nlev, rh.n_dst), 555.0, dtype=torch.float64, device="cuda")
    s0 = torch.cuda.current_stream().cuda_stream
    INV, UNS = L.MPG_ERR_INVALID_ARG, L.MPG_ERR_UNSUPPORTED

    def call(hh="rh", gp="g", gt=0, ld=0, sp="src", st=0, lay=0, nl=nlev, nf=1, dp="dst", dt=0, opts="default", wp="work", **o):
        if opts == "default":
            f = dict(flags=1, missing_value=0.0, src_mask_dev=None, min_valid_frac=0.5, fill_value=0.0, scale=1.0, offset=0.0)
            f.update(o)
            opts = C.byref(L.MaskOpts(**f))
        ptr = {"g": g.data_ptr(), "src": src.data_ptr(), "dst": dst.data_ptr(), "work": work.data_ptr(), None: None, "rh": rh._h}
        return L.regrid_masked_transpose_dev(ptr[hh], ptr[gp], gt, ld, ptr[sp], st, lay, nl, nf, ptr[dp], dt, opts, ptr[wp], s0)

    assert call(gt=2) == UNS and call(st=2) == UNS and call(dt=3) == UNS
    assert call(hh=None) == INV and call(opts=None) == INV and call(gp=None) == INV and call(sp=None) == INV and call(dp=None) == INV
    assert call(wp=None) == INV
    assert call(lay=2) == INV and call(nl=0) == INV and call(nf=0) == INV and call(gt=4) == INV and call(dt=-1) == INV
    assert call(min_valid_frac=-0.01) == INV and call(min_valid_frac=1.01) == INV and call(min_valid_frac=float("nan")) == INV
    assert call(flags=2, missing_value=float("nan")) == INV and call(flags=4) == INV and call(flags=7) == INV
    assert call(ld=rh.n_dst - 1) == INV
    assert call(wp="g") == INV and call(wp="src") == INV and call(wp="dst") == INV, "an aliased workspace"
    assert L.load().mpg_regrid_masked_transpose_dev(*([C.c_void_p(0)] * 14)) == INV
    # a periodic Grid -> Grid handle with pole caps
    grid = R.Grid.from_target(T.define_target_grid_params("lat-lon", nx=73, ny=37, stand_lon=0.0, is_regional=False))
    rp = R.regrid_store_grid(grid, R.STAGGERLOC_EDGE2)
    assert len(rp.pole()[0]) > 0
    pg = torch.zeros(rp.n_dst, dtype=torch.float64, device="cuda")
    ps = torch.zeros(rp.n_src, dtype=torch.float64, device="cuda")
    pd = torch.full((rp.n_src,), 777.0, dtype=torch.float64, device="cuda")
    pw = torch.full((rp.n_dst,), 555.0, dtype=torch.float64, device="cuda")
    opts = L.MaskOpts(1, 0.0, None, 0.5, 0.0, 1.0, 0.0)
    assert L.regrid_masked_transpose_dev(rp._h, pg.data_ptr(), 0, 0, ps.data_ptr(), 0, 0, 1, 1, pd.data_ptr(), 0, C.byref(opts), pw.data_ptr(), s0) == UNS
    with pytest.raises(L.MpgError, match="pole"):
        rp.regrid_masked_transpose(pg, ps)
    torch.cuda.synchronize()
    for t, v in ((dst, 777.0), (work, 555.0), (pd, 777.0), (pw, 555.0)):
        assert bool((t == v).all()), "a refused call wrote to its destination or workspace"
    with pytest.raises(ValueError):
        rh.regrid_masked_transpose(g.reshape(-1)[:-1], src.reshape(-1), nlev=nlev)
    with pytest.raises(ValueError):
        rh.regrid_masked_transpose(g, src.reshape(-1)[:-1], nlev=nlev)
    with pytest.raises(ValueError):
        rh.regrid_masked_transpose(g, src.reshape(-1), nlev=nlev, missing="none")
    with pytest.raises(ValueError):
        rh.regrid_masked_transpose(g, src.reshape(-1), nlev=nlev, work=work.float())
    assert call() == 0                                                           # the handle and the stream still work
    torch.cuda.synchronize()
    assert bool((dst == 0.0).all()) and bool((work == 0.0).all())
    rp.release()
    grid.destroy()


# ---- 7: re-indexed handles ------------------------------------------------------------------------------------------------------------
def test_reindexed_handle_takes_the_mask_in_its_current_index_space(gpu_lib, regional_case):
    import torch
    from mpassit_amd import regrid as R
    m, g = regional_case
    nlev = 3
    rng = np.random.default_rng(31)
    x = rng.uniform(-50.0, 50.0, size=(nlev, m.nCells))
    x[rng.uniform(size=x.shape) < 0.15] = np.nan
    mask = rng.uniform(size=m.nCells) < 0.2
    src, mt = torch.as_tensor(x, device="cuda"), torch.as_tensor(mask, device="cuda")
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g, rows=(20, 55))
    hs = [R.regrid_store(mesh, grid, md) for md in (R.REGRIDMETHOD_BILINEAR, R.REGRIDMETHOD_CONSERVE, R.REGRIDMETHOD_NEAREST_STOD)]
    grads = [torch.as_tensor(rng.normal(size=(nlev, h.n_dst)), device="cuda") for h in hs]
    full = [h.regrid_masked_transpose(gr, src.reshape(-1), nlev=nlev, src_mask=mt) for h, gr in zip(hs, grads)]
    rngs = [h.source_range() for h in hs]
    lo, hi = min(a for a, _ in rngs), max(b for _, b in rngs)
    assert 0 < lo < hi < m.nCells
    mesh.set_source_window(lo, hi - lo)
    for h, gr, want in zip(hs, grads, full):
        h._refresh()
        assert h.n_src == hi - lo
        want = want.reshape(nlev, m.nCells)
        assert bool((want != 0).any()) and bool((want[:, :lo] == 0).all()) and bool((want[:, hi:] == 0).all())
        got = h.regrid_masked_transpose(gr, src[:, lo:hi].t().contiguous().reshape(-1), nlev=nlev, layout=R.LAYOUT_LEV_FAST,
                                        src_mask=mt[lo:hi].contiguous())
        assert torch.equal(got.reshape(hi - lo, nlev).t(), want[:, lo:hi]), "source window: the result changed"
    mesh.set_source_window(0, m.nCells)
    for h in hs:
        h.release()
    mesh.destroy()
    grid.destroy()


# ---- 8: graph capture -----------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_same_bits(handles):
    import torch
    nlev = 6
    cases = []
    for name, lf, dt in (("bilinear", False, torch.float64), ("bilinear", True, torch.float32), ("conserve", False, torch.float64),
                         ("grid4", True, torch.float64), ("synthetic", True, torch.float64)):
        rh, pat = handles[name]
        x, missing, _, mask = _gaps(pat, nlev, 1, ("nan", "value", "mask"), 17)
        src = _dev(x)
        src = (src.transpose(1, 2).contiguous() if lf else src).reshape(-1)
        g = _dev(np.random.default_rng(3).normal(size=(1, nlev, pat.n_dst)))
        out = torch.empty((1, rh.n_src, nlev) if lf else (1, nlev, rh.n_src), dtype=dt, device="cuda")
        work = torch.empty((1, nlev, rh.n_dst), dtype=torch.float64, device="cuda")
        cases.append((rh, g, src, dict(nlev=nlev, layout=int(lf), missing=missing, src_mask=torch.as_tensor(mask, device="cuda"), out=out, work=work)))

    def step():
        for rh, g, src, kw in cases:
            rh.regrid_masked_transpose(g, src, **kw)

    step()                                            # the first call builds the transposed index: eager
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):    # one stream: a chain, no parallel branches
            step()
    for trial in range(2):
        for _, g, src, _ in cases:
            g.mul_(-0.5)
            src.mul_(-0.5)                            # NaN stays NaN, the sentinel changes into data
        graph.replay()
        torch.cuda.synchronize()
        got = [(c[3]["out"].clone(), c[3]["work"].clone()) for c in cases]
        step()
        torch.cuda.synchronize()
        for (a, w), c in zip(got, cases):
            assert torch.equal(a, c[3]["out"]) and torch.equal(w, c[3]["work"]), "replay %d differs from the eager call" % trial
