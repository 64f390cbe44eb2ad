"""Transpose Regrid (mpg_regrid_transpose_dev, RouteHandle.regrid_transpose): mesh_out = A^T grid_in for every kind of handle,
against A^T g built from the handle's own ESMF weight list (pole terms included), and the call's contract: zeros for
unreferenced sources, pitched inputs, types, layouts, batching, determinism, the adjoint identity, re-indexing and errors."""
import ctypes as C

import numpy as np
import pytest

from _transpose_ref import assert_f32_close, assert_f64_close, transpose_ref

pytestmark = pytest.mark.gpu


def _g(rh, nlev, seed=0, nfields=1):
    rng = np.random.default_rng(seed)
    return rng.uniform(-50.0, 50.0, size=(nfields, nlev, rh.n_dst))


def _check_handle(rh, what, nlev=3):
    import torch
    from mpassit_amd import regrid as R
    g = _g(rh, nlev)
    want, bound = transpose_ref(rh, g[0])
    gt = torch.as_tensor(g, device="cuda")
    cf = rh.regrid_transpose(gt, nlev=nlev)
    lf = rh.regrid_transpose(gt, nlev=nlev, layout=R.LAYOUT_LEV_FAST)
    torch.cuda.synchronize()
    assert tuple(cf.shape) == (1, nlev, rh.n_src) and tuple(lf.shape) == (1, rh.n_src, nlev)
    assert_f64_close(cf.cpu().numpy(), want, bound, what + " cell-fast")
    assert torch.equal(lf[0].t().contiguous(), cf[0]), what + ": the layouts differ"
    return cf


@pytest.fixture(scope="module")
def lattice(gpu_lib, regional_case, global_mesh, conus_grid_30km):
    from mpassit_amd import regrid as R
    m, g = regional_case
    cases = {"regional": (R.Mesh.from_mpas(m), R.Grid.from_target(g)), "global": (R.Mesh.from_mpas(global_mesh), R.Grid.from_target(conus_grid_30km))}
    yield cases
    for mesh, grid in cases.values():
        mesh.destroy()
        grid.destroy()


@pytest.mark.parametrize("case", ["regional", "global"])
@pytest.mark.parametrize("kind", ["bilinear", "node", "nearest", "conserve"])
def test_mesh_handles_match_reference(lattice, case, kind):
    from mpassit_amd import regrid as R
    mesh, grid = lattice[case]
    kw = {"bilinear": dict(regridmethod=R.REGRIDMETHOD_BILINEAR), "node": dict(regridmethod=R.REGRIDMETHOD_BILINEAR, meshloc=R.MESHLOC_NODE),
          "nearest": dict(regridmethod=R.REGRIDMETHOD_NEAREST_STOD), "conserve": dict(regridmethod=R.REGRIDMETHOD_CONSERVE)}[kind]
    rh = R.regrid_store(mesh, grid, **kw)
    _check_handle(rh, "%s %s" % (case, kind))
    nref, mx = rh.transpose_stats()
    assert 0 < nref <= rh.n_src and mx >= 1
    rh.release()


@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("stagger", ["EDGE1", "EDGE2"])
def test_grid_handles_match_reference(gpu_lib, conus_grid_30km, periodic, stagger):
    from mpassit_amd import regrid as R, target_grid as T
    t = T.define_target_grid_params("lat-lon", nx=73, ny=37, stand_lon=0.0, is_regional=False) if periodic else conus_grid_30km
    grid = R.Grid.from_target(t)
    rh = R.regrid_store_grid(grid, getattr(R, "STAGGERLOC_" + stagger))
    if periodic and stagger == "EDGE2":
        assert len(rh.pole()[0]) > 0, "the periodic grid's EDGE2 handle carries pole caps"
    _check_handle(rh, "grid %s %s" % ("periodic" if periodic else "lambert", stagger), nlev=4)
    rh.release()
    grid.destroy()


def test_from_weights_duplicates_hand_computed(gpu_lib):
    import torch
    from mpassit_amd import regrid as R
    # 2 x 2 destination points (1-based rows), 5 sources; (row 1, col 2) appears twice, source 5 is never referenced
    row = [1, 1, 1, 2, 3, 3, 4]
    col = [2, 2, 1, 3, 4, 1, 3]
    S = [0.25, 0.5, 0.125, 1.0, -2.0, 0.75, 3.0]
    rh = R.RouteHandle.from_weights(5, 2, 2, row, col, S)
    g = np.array([2.0, -4.0, 8.0, 16.0])
    want = np.array([0.125 * 2.0 + 0.75 * 8.0, 0.25 * 2.0 + 0.5 * 2.0, 1.0 * -4.0 + 3.0 * 16.0, -2.0 * 8.0, 0.0])
    out = torch.full((1, 1, 5), float("nan"), dtype=torch.float64, device="cuda")
    rh.regrid_transpose(torch.as_tensor(g, device="cuda"), out=out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(-1), want)
    assert rh.transpose_stats() == (4, 2)
    rh.release()


@pytest.fixture(scope="module")
def block(gpu_lib, regional_case):
    """A bilinear handle of a grid row block: most of the mesh is referenced by nothing."""
    from mpassit_amd import regrid as R
    m, g = regional_case
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g, rows=(20, 55))
    rh = R.regrid_store(mesh, grid, R.REGRIDMETHOD_BILINEAR)
    yield rh
    rh.release()
    mesh.destroy()
    grid.destroy()


def test_unreferenced_sources_are_exact_zero(block):
    import torch
    from mpassit_amd import regrid as R
    rh, nlev = block, 4
    nref, _ = rh.transpose_stats()
    assert 0 < nref < rh.n_src // 2
    g = torch.as_tensor(_g(rh, nlev), device="cuda")
    for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
        shape = (1, nlev, rh.n_src) if layout == R.LAYOUT_CELL_FAST else (1, rh.n_src, nlev)
        out = torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
        rh.regrid_transpose(g, nlev=nlev, layout=layout, out=out)
        o = out.cpu().numpy().reshape(shape[1:])
        if layout == R.LAYOUT_LEV_FAST:
            o = o.T
        assert not np.isnan(o).any(), "out was not fully overwritten"
        assert int((np.abs(o).sum(axis=0) != 0).sum()) <= nref
    _, col, _ = rh.to_esmf_weights()
    unref = np.setdiff1d(np.arange(rh.n_src), col - 1)
    assert unref.size == rh.n_src - nref and np.all(o[:, unref] == 0.0)


def test_pitched_nan_padded_source_is_dense_bitwise(block):
    import torch
    rh, nlev, nf = block, 5, 2
    g = torch.as_tensor(_g(rh, nlev, nfields=nf), device="cuda")
    dense = rh.regrid_transpose(g, nlev=nlev, nfields=nf)
    for dt in (torch.float64, torch.float32):
        pitched = rh.empty_pitched(nlev, nf, dtype=dt)
        pitched.as_strided((nf * nlev * rh.level_stride(dt),), (1,)).fill_(float("nan"))   # the pad of every plane too
        pitched.copy_(g.view(nf, nlev, rh.ny_dst, rh.nx_dst))
        got = rh.regrid_transpose(pitched, nlev=nlev, nfields=nf, out_dtype=torch.float64)
        want = dense if dt == torch.float64 else rh.regrid_transpose(g.to(dt), nlev=nlev, nfields=nf, out_dtype=torch.float64)
        torch.cuda.synchronize()
        assert torch.equal(got, want)
        assert not torch.isnan(got).any()


def test_types_layouts_batching_determinism(block):
    import torch
    from mpassit_amd import regrid as R
    rh, nlev = block, 6
    g64 = _g(rh, nlev, seed=7, nfields=3)
    g32 = g64.astype(np.float32)
    t64, t32 = torch.as_tensor(g64, device="cuda"), torch.as_tensor(g32, device="cuda")
    t32w = t32.to(torch.float64)          # float64 holding the float32 values
    a = rh.regrid_transpose(t32, nlev=nlev, nfields=3, out_dtype=torch.float64)
    b = rh.regrid_transpose(t32w, nlev=nlev, nfields=3)
    assert torch.equal(a, b), "float32 and float64 inputs holding the same values differ"
    want, bound = transpose_ref(rh, g32[0].astype(np.float64))
    assert_f64_close(a[0].cpu().numpy(), want, bound, "f32 in, f64 out")
    assert_f32_close(rh.regrid_transpose(t32, nlev=nlev, nfields=3)[0].cpu().numpy(), want, bound, "f32 in, f32 out")
    want, bound = transpose_ref(rh, g64[0])
    assert_f32_close(rh.regrid_transpose(t64, nlev=nlev, nfields=3, out_dtype=torch.float32)[0].cpu().numpy(), want, bound, "f64 in, f32 out")
    c = rh.regrid_transpose(t64, nlev=nlev, nfields=3)
    assert_f64_close(c[0].cpu().numpy(), want, bound, "f64 in, f64 out")
    # a float32 result is the float64 one rounded once
    assert torch.equal(rh.regrid_transpose(t64, nlev=nlev, nfields=3, out_dtype=torch.float32), c.to(torch.float32))
    lf = rh.regrid_transpose(t64, nlev=nlev, nfields=3, layout=R.LAYOUT_LEV_FAST)
    assert torch.equal(lf.transpose(1, 2), c), "the two layouts differ"
    for f in range(3):
        assert torch.equal(rh.regrid_transpose(t64[f].contiguous(), nlev=nlev), c[f:f + 1]), "nfields=3 differs from single calls"
    assert torch.equal(rh.regrid_transpose(t64, nlev=nlev, nfields=3), c), "two calls differ"


@pytest.mark.parametrize("kind", ["bilinear", "conserve"])
def test_dot_product_identity(lattice, kind):
    import torch
    from mpassit_amd import regrid as R
    mesh, grid = lattice["global"]
    rh = R.regrid_store(mesh, grid, R.REGRIDMETHOD_BILINEAR if kind == "bilinear" else R.REGRIDMETHOD_CONSERVE)
    rng = np.random.default_rng(11)
    nlev = 2
    x = torch.as_tensor(rng.normal(size=(nlev, rh.n_src)), device="cuda")
    y = torch.as_tensor(rng.normal(size=(nlev, rh.n_dst)), device="cuda")
    ax = rh.regrid(x.reshape(-1), nlev=nlev).reshape(nlev, -1)
    aty = rh.regrid_transpose(y, nlev=nlev).reshape(nlev, -1)
    lhs, rhs = float((ax * y).sum()), float((x * aty).sum())
    assert abs(lhs - rhs) <= 1e-13 * float(ax.norm() * y.norm())     # relative to the Cauchy-Schwarz scale of the products
    rh.release()


def test_long_segments_coarse_mesh_to_fine_grid(gpu_lib, conus_grid_30km):
    import torch
    from mpassit_amd import regrid as R, synth
    m = synth.global_voronoi_mesh(642)
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(conus_grid_30km)
    for method in (R.REGRIDMETHOD_NEAREST_STOD, R.REGRIDMETHOD_CONSERVE):
        rh = R.regrid_store(mesh, grid, method)
        nref, mx = rh.transpose_stats()
        assert mx > 64, "the coarse mesh should give long transposed rows (%d)" % mx
        cf = _check_handle(rh, "coarse method %d" % method, nlev=70)     # more levels than a wave has lanes
        assert torch.equal(rh.regrid_transpose(torch.as_tensor(_g(rh, 70), device="cuda"), nlev=70), cf)
        rh.release()
    mesh.destroy()
    grid.destroy()


def test_localize_drops_the_cached_transpose(gpu_lib, regional_case):
    import torch
    from mpassit_amd import regrid as R
    m, g = regional_case
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g, rows=(10, 40))
    rh = R.regrid_store(mesh, grid, R.REGRIDMETHOD_BILINEAR)
    nlev = 3
    gt = torch.as_tensor(_g(rh, nlev, seed=5), device="cuda")
    before = rh.regrid_transpose(gt, nlev=nlev)           # builds the transposed index in global ids
    ids = rh.localize()
    assert rh.n_src == ids.size < m.nCells
    after = rh.regrid_transpose(gt, nlev=nlev)
    assert tuple(after.shape) == (1, nlev, ids.size)
    assert torch.equal(after, before[:, :, torch.as_tensor(ids, device="cuda", dtype=torch.int64)])
    assert rh.transpose_stats()[0] == ids.size
    rh.release()
    mesh.destroy()
    grid.destroy()


def test_source_window_gives_the_windows_rows(gpu_lib, regional_case):
    import torch
    from mpassit_amd import regrid as R
    m, g = regional_case
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g, rows=(20, 55))
    hs = [R.regrid_store(mesh, grid, md) for md in (R.REGRIDMETHOD_BILINEAR, R.REGRIDMETHOD_CONSERVE)]
    nlev = 3
    gt = torch.as_tensor(_g(hs[0], nlev, seed=9), device="cuda")
    full = [h.regrid_transpose(gt, nlev=nlev) for h in hs]
    rngs = [h.source_range() for h in hs]
    lo, hi = min(a for a, _ in rngs), max(b for _, b in rngs)
    assert 0 < lo < hi < m.nCells
    mesh.set_source_window(lo, hi - lo)
    for h, want in zip(hs, full):
        h._refresh()
        assert h.n_src == hi - lo
        got = h.regrid_transpose(gt, nlev=nlev, layout=R.LAYOUT_LEV_FAST)
        assert torch.equal(got.transpose(1, 2), want[:, :, lo:hi])
        assert float(want[:, :, :lo].abs().sum()) == 0.0 and float(want[:, :, hi:].abs().sum()) == 0.0
    mesh.set_source_window(0, m.nCells)
    for h, want in zip(hs, full):
        h._refresh()
        assert torch.equal(h.regrid_transpose(gt, nlev=nlev), want)
        h.release()
    mesh.destroy()
    grid.destroy()


def test_errors_do_not_fault(block):
    import torch
    from mpassit_amd import _lib as L, regrid as R
    from mpassit_amd._lib import MpgError
    rh, nlev = block, 2
    lib = L.load()
    src = torch.zeros((nlev, rh.n_dst), dtype=torch.float64, device="cuda")
    dst = torch.zeros((nlev, rh.n_src), dtype=torch.float64, device="cuda")
    sp, dp, s0 = C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(h=rh._h, s=sp, st=0, ld=0, nl=nlev, nf=1, d=dp, dt=0, lay=0):
        return lib.mpg_regrid_transpose_dev(h, s, C.c_int(st), C.c_int64(ld), C.c_int(nl), C.c_int(nf), d, C.c_int(dt), C.c_int(lay), s0)

    assert call() == 0
    assert call(ld=rh.n_dst - 1) == L.MPG_ERR_INVALID_ARG
    assert call(ld=-5) == L.MPG_ERR_INVALID_ARG
    assert call(st=2) == L.MPG_ERR_UNSUPPORTED and call(dt=3) == L.MPG_ERR_UNSUPPORTED
    assert call(st=4) == L.MPG_ERR_INVALID_ARG
    assert call(h=None) == L.MPG_ERR_INVALID_ARG
    assert call(s=None) == L.MPG_ERR_INVALID_ARG and call(d=None) == L.MPG_ERR_INVALID_ARG
    assert call(nl=0) == L.MPG_ERR_INVALID_ARG and call(nf=0) == L.MPG_ERR_INVALID_ARG
    assert call(lay=2) == L.MPG_ERR_INVALID_ARG
    a = C.c_int64()
    assert lib.mpg_handle_transpose_stats(None, C.byref(a), C.byref(a)) == L.MPG_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        rh.regrid_transpose(src[:, ::2], nlev=nlev)                       # a strided source that is not plane-pitched
    with pytest.raises(ValueError):
        rh.regrid_transpose(src.reshape(-1)[:-1], nlev=nlev)               # wrong size
    with pytest.raises(MpgError, match="below the plane size"):
        L.check(call(ld=1))
    assert call() == 0                                                     # the handle and the stream still work
    torch.cuda.synchronize()
