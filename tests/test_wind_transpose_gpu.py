"""The adjoint of the wind chain on the GPU: mpg_rotate_winds_transpose_dev and the fused mpg_wind_destagger_transpose_dev
(csrc/k_wind_transpose.hip), their wrappers and the differentiable wind_destagger_autograd.

The bar: the fused call equals, BIT FOR BIT, the three-call chain -- rh.regrid_transpose on each handle into float64 (pinned to
tests/c/contract_ref.c by test_contract_gpu.py: the adjoint hangs from that contract), the optional adds, then
rotate_winds_cgrid_transpose (pinned here to its numpy mirror) -- and the whole is the transpose of the forward wind_destagger and of
the oracle's forward, by dot products.

Two notes on the cases.  (1) "float32 forward results" in the dot products: a forward result ROUNDED to float32 is 2^-24 away from the
linear map, which no pairing can hold to 1e-11 * sum|terms| (random signs leave about 6e-8 * sqrt(N) against 1e-11 * N relative to one
term); the case therefore feeds float32 gradients -- what a float32 forward hands its backward, widened exactly by the kernel -- and pairs
them with the unrounded forward.  The float32 forward itself runs in the autograd test.  (2) The refusal of a level plane of 4 GiB or
more is the forward's own test (one function serves both calls); a pair of handles that large takes tens of GB and is not built here."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAMBERT = dict(ref_lat=38.5, ref_lon=-97.5, truelat1=38.5, truelat2=38.5, stand_lon=-97.5)
SHAPES = [(33, 9, 1), (64, 16, 2), (65, 17, 4), (203, 35, 3), (17, 131, 2)]
_CASES = {}


class _Case:
    """One grid with its CENTER -> EDGE1 / EDGE2 handles and, on a Lambert grid, its angles on the device."""

    def __init__(self, key):
        import torch
        from mpassit_amd import regrid as R, target_grid as T
        if key[0] == "lambert":
            self.t = T.define_target_grid_params("lambert", key[1] + 1, key[2] + 1, dx=30000.0, dy=30000.0, **LAMBERT)
            self.cosa = torch.as_tensor(np.ascontiguousarray(self.t.cosa, dtype=np.float64), device="cuda")
            self.sina = torch.as_tensor(np.ascontiguousarray(self.t.sina, dtype=np.float64), device="cuda")
        else:
            self.t = T.define_target_grid_params("lat-lon", nx=key[1], ny=key[2], stand_lon=0.0, is_regional=False)
            self.cosa = self.sina = None
        self.grid = R.Grid.from_target(self.t)
        self.rh_u = R.regrid_store_grid(self.grid, R.STAGGERLOC_EDGE1)
        self.rh_v = R.regrid_store_grid(self.grid, R.STAGGERLOC_EDGE2)
        self.nx, self.ny = self.t.nx, self.t.ny

    def close(self):
        self.rh_u.release()
        self.rh_v.release()
        self.grid.destroy()


@pytest.fixture(scope="module")
def cases(gpu_lib):
    def get(nx, ny, kind="lambert"):
        key = (kind, nx, ny)
        if key not in _CASES:
            _CASES[key] = _Case(key)
        return _CASES[key]
    yield get
    for c in _CASES.values():
        c.close()
    _CASES.clear()


def _same_bits(torch, a, b):
    it = {8: torch.int64, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.contiguous().view(it) == b.contiguous().view(it)).all())


def _rand(torch, shape, seed, dtype=None):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    x = (torch.rand(shape, dtype=torch.float64, device="cuda", generator=gen) - 0.5) * 8.0
    return x if dtype in (None, torch.float64) else x.to(dtype)


def _grads(torch, c, nlev, seed, dtype=None):
    """(gu [nlev][ny][nx+1], gv [nlev][ny+1][nx]) of dtype; the float64 ones hold float32 values when dtype is float32's twin "f32 in f64"."""
    return _rand(torch, (nlev, c.ny, c.nx + 1), seed, dtype), _rand(torch, (nlev, c.ny + 1, c.nx), seed + 1, dtype)


def _pitched(torch, x, ld, pad=float("nan")):
    """x [nlev][ny][nx] as a view of a buffer whose level planes lie ld elements apart, the pad filled with `pad`."""
    nlev, ny, nx = x.shape
    buf = torch.full((nlev, ld), pad, dtype=x.dtype, device=x.device)
    buf[:, :ny * nx] = x.reshape(nlev, -1)
    return buf.as_strided((nlev, ny, nx), (ld, nx, 1))


def _chain(torch, R, c, rot, which, gu, gv, nlev, gur=None, gvr=None):
    """Two regrid_transpose calls into float64, the adds, the rotation's adjoint: the contract the fused call is held to."""
    shape = (nlev, c.ny, c.nx)
    s1 = c.rh_u.regrid_transpose(gu, nlev=nlev, out_dtype=torch.float64).reshape(shape) if "u" in which else None
    s2 = c.rh_v.regrid_transpose(gv, nlev=nlev, out_dtype=torch.float64).reshape(shape) if "v" in which else None
    if gur is not None:
        s1 = s1 + gur
    if gvr is not None:
        s2 = s2 + gvr
    if rot:
        R.rotate_winds_cgrid_transpose(c.cosa, c.sina, s1, s2)
    return s1, s2


def _fused(R, c, rot, which, gu, gv, nlev, gur=None, gvr=None, outs=None):
    return R.wind_destagger_transpose(c.rh_u if "u" in which else None, c.rh_v if "v" in which else None, c.cosa if rot else None,
                                      c.sina if rot else None, gu if "u" in which else None, gv if "v" in which else None, nlev,
                                      g_umass_rot=gur, g_vmass_rot=gvr, outs=outs)


# ---- 1. the rotation's adjoint ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny,nlev", SHAPES)
def test_rotation_adjoint_equals_the_numpy_mirror(cases, nx, ny, nlev):
    import torch
    from mpassit_amd import regrid as R, target_grid as T
    c = cases(nx, ny)
    gu, gv = _rand(torch, (nlev, ny, nx), 10 + nx), _rand(torch, (nlev, ny, nx), 20 + nx)
    want_u, want_v = T.rotate_winds_transpose_at(c.t.cosa, c.t.sina, gu.cpu().numpy(), gv.cpu().numpy())   # the angles reused over the levels
    pu, pv = gu.data_ptr(), gv.data_ptr()
    ru, rv = R.rotate_winds_cgrid_transpose(c.cosa, c.sina, gu, gv)
    torch.cuda.synchronize()
    assert ru is gu and rv is gv and gu.data_ptr() == pu and gv.data_ptr() == pv, "in place"
    assert np.array_equal(gu.cpu().numpy().view(np.int64), want_u.view(np.int64))
    assert np.array_equal(gv.cpu().numpy().view(np.int64), want_v.view(np.int64))


# ---- 2. fused == chain, bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", [True, False])
@pytest.mark.parametrize("nx,ny,nlev", SHAPES)
def test_fused_equals_chain_bit_for_bit(cases, nx, ny, nlev, rot):
    import torch
    from mpassit_amd import regrid as R
    c = cases(nx, ny)
    gu32, gv32 = _grads(torch, c, nlev, 100 + nx, torch.float32)
    gur, gvr = _rand(torch, (nlev, ny, nx), 7), _rand(torch, (nlev, ny, nx), 8)
    plane = max(c.rh_u.n_dst, c.rh_v.n_dst)
    ran = 0
    for which in (("uv",) if rot else ("uv", "u", "v")):
        ref = {}
        for dtype in (torch.float64, torch.float32):
            gu, gv = gu32.to(dtype), gv32.to(dtype)           # the same values in both types
            for ld in (0, plane, plane + 37):
                if ld and nlev == 1:
                    continue                                  # a single plane has no stride
                su, sv = (gu, gv) if ld == 0 else (_pitched(torch, gu, ld), _pitched(torch, gv, ld))
                for adds in ((False, True) if rot else (False,)):
                    a, b = (gur, gvr) if adds else (None, None)
                    want = _chain(torch, R, c, rot, which, su, sv, nlev, a, b)
                    got = _fused(R, c, rot, which, su, sv, nlev, a, b)
                    torch.cuda.synchronize()
                    for w, g, name in zip(want, got, "uv"):
                        assert (g is None) == (name not in which)
                        if g is not None:
                            assert g.dtype == torch.float64 and tuple(g.shape) == (nlev, ny, nx)
                            assert _same_bits(torch, g, w), (which, dtype, ld, adds, name)
                            # the same bits across dense / pitched sources and across F32 / F64 inputs of the same values
                            first = ref.setdefault((adds, name), g.clone())
                            assert _same_bits(torch, g, first), (which, dtype, ld, adds, name)
                    ran += 1
    assert ran >= (2 if nlev == 1 else 6)
    # one gradient of the rotated mass winds alone is one add on its side only
    if rot:
        gu, gv = gu32.double(), gv32.double()
        want = _chain(torch, R, c, True, "uv", gu, gv, nlev, gur, None)
        got = _fused(R, c, True, "uv", gu, gv, nlev, gur, None)
        assert _same_bits(torch, got[0], want[0]) and _same_bits(torch, got[1], want[1])
    # outs= are written in place
    o = (torch.full((nlev, ny, nx), float("nan"), dtype=torch.float64, device="cuda"), torch.full((nlev, ny, nx), float("nan"), dtype=torch.float64, device="cuda"))
    got = _fused(R, c, rot, "uv", gu32, gv32, nlev, outs=o)
    want = _chain(torch, R, c, rot, "uv", gu32, gv32, nlev)
    assert got[0] is o[0] and got[1] is o[1] and _same_bits(torch, o[0], want[0]) and _same_bits(torch, o[1], want[1])


# ---- 3. a periodic grid with pole caps ----------------------------------------------------------------------------------------------------
def test_periodic_grid_with_pole_caps(cases):
    import torch
    from mpassit_amd import regrid as R
    c = cases(73, 37, "lat-lon")
    assert c.rh_v.pole()[0].size > 0, "the V rows at the poles are capped"
    nlev = 3
    for dtype in (torch.float64, torch.float32):
        gu, gv = _grads(torch, c, nlev, 5, dtype)
        want_u = c.rh_u.regrid_transpose(gu, nlev=nlev, out_dtype=torch.float64).reshape(nlev, c.ny, c.nx)
        want_v = c.rh_v.regrid_transpose(gv, nlev=nlev, out_dtype=torch.float64).reshape(nlev, c.ny, c.nx)
        for which in ("uv", "u", "v"):
            got = _fused(R, c, False, which, gu, gv, nlev)
            torch.cuda.synchronize()
            assert "u" not in which or _same_bits(torch, got[0], want_u)
            assert "v" not in which or _same_bits(torch, got[1], want_v)
    assert float(want_v[:, 0, :].abs().min()) > 0.0, "the pole term reaches the whole CENTER row"


# ---- 4. canaries: what must never be read ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", [True, False])
def test_unmapped_points_and_the_pad_are_never_read(cases, rot):
    import torch
    from mpassit_amd import regrid as R
    c = cases(65, 17)
    nlev = 2
    gu, gv = _grads(torch, c, nlev, 31)
    clean = _fused(R, c, rot, "uv", gu, gv, nlev)
    un_u = torch.as_tensor(c.rh_u.weights()[0][:, 0] < 0, device="cuda").reshape(c.ny, c.nx + 1)
    un_v = torch.as_tensor(c.rh_v.weights()[0][:, 0] < 0, device="cuda").reshape(c.ny + 1, c.nx)
    assert bool(un_u.any()) and bool(un_v.any()), "the outer half-cell ring is unmapped"
    bu, bv = gu.clone(), gv.clone()
    bu[:, un_u] = float("nan")
    bv[:, un_v] = float("nan")
    ld = max(c.rh_u.n_dst, c.rh_v.n_dst) + 19
    for su, sv in ((bu, bv), (_pitched(torch, gu, ld), _pitched(torch, gv, ld)), (_pitched(torch, bu, ld), _pitched(torch, bv, ld))):
        got = _fused(R, c, rot, "uv", su, sv, nlev)
        torch.cuda.synchronize()
        for g, w in zip(got, clean):
            assert bool(torch.isfinite(g).all()) and _same_bits(torch, g, w)


# ---- 5. the transpose of the forward --------------------------------------------------------------------------------------------------------
def _dot(torch, a, b):
    p = a.double() * b.double()
    return float(p.sum()), float(p.abs().sum())


@pytest.mark.parametrize("rot,keep,ydtype", [(True, False, "float64"), (True, True, "float64"), (False, False, "float64"), (True, True, "float32"),
                                             (False, False, "float32")])
@pytest.mark.parametrize("nx,ny,nlev", SHAPES)
def test_dot_product_against_the_forward(cases, nx, ny, nlev, rot, keep, ydtype):
    """|<wind_destagger(um, vm), y> - <(um, vm), F^T y>| <= 1e-11 * sum|terms|, y on every result the forward returns; float32: see the
    module docstring."""
    import torch
    from mpassit_amd import regrid as R
    c = cases(nx, ny)
    um, vm = _rand(torch, (nlev, ny, nx), 41) * 7.5, _rand(torch, (nlev, ny, nx), 42) * 7.5
    res = R.wind_destagger(c.rh_u, c.rh_v, c.cosa if rot else None, c.sina if rot else None, um, vm, nlev, keep_mass=keep)
    assert (res[2] is not None) == (keep and rot)
    dt = getattr(torch, ydtype)
    ys = [_rand(torch, tuple(r.shape), 50 + i, dt) if r is not None else None for i, r in enumerate(res)]
    gum, gvm = R.wind_destagger_transpose(c.rh_u, c.rh_v, c.cosa if rot else None, c.sina if rot else None, ys[0], ys[1], nlev,
                                          g_umass_rot=ys[2].double() if ys[2] is not None else None,
                                          g_vmass_rot=ys[3].double() if ys[3] is not None else None)
    lhs = [_dot(torch, r, y) for r, y in zip(res, ys) if r is not None]
    rhs = [_dot(torch, um, gum), _dot(torch, vm, gvm)]
    resid = abs(sum(s for s, _ in lhs) - sum(s for s, _ in rhs))
    terms = sum(a for _, a in lhs) + sum(a for _, a in rhs)
    print("forward dot product: residual %.3e, bound %.3e" % (resid, 1e-11 * terms))
    assert terms > 0.0 and resid <= 1e-11 * terms


# ---- 6. the transpose of the oracle's forward -----------------------------------------------------------------------------------------------
def test_dot_product_against_the_oracle(cases, oracle):
    """The forward on the CPU from oracle primitives (rotate_winds + grid_bilinear + apply_fixed, as test_interp_gpu.py builds U and V), y zero on
    the outer ring (implementation-defined, App. A4): the bound is the forward's own parity bound 1e-9 per element times sum|y|, plus the
    pairing's 1e-11 * sum|terms|."""
    import torch
    from mpassit_amd import regrid as R
    o = oracle
    nx, ny, nlev = 65, 17, 2
    c = cases(nx, ny)
    t = c.t
    rng = np.random.default_rng(3)
    um, vm = (rng.random((nlev, ny, nx)) - 0.5) * 60.0, (rng.random((nlev, ny, nx)) - 0.5) * 60.0
    ur, vr = o.rotate_winds(t.cosa, t.sina, um.reshape(nlev, -1), vm.reshape(nlev, -1))
    cen = o.lonlat_deg_to_xyz(t.lon, t.lat)
    fwd, ys = [], []
    for src, st, lon, lat in ((ur, 1, t.lon_u, t.lat_u), (vr, 2, t.lon_v, t.lat_v)):
        gi, gw = o.grid_bilinear(nx, ny, cen, st, o.lonlat_deg_to_xyz(lon, lat))
        fwd.append(o.apply_fixed(gi, gw, src.reshape(nlev, -1), nlev).reshape((nlev,) + lon.shape))
        y = rng.standard_normal((nlev,) + lon.shape)
        y[:, [0, -1], :] = 0.0
        y[:, :, [0, -1]] = 0.0
        ys.append(y)
    assert fwd[0].shape == (nlev, ny, nx + 1) and fwd[1].shape == (nlev, ny + 1, nx)
    gum, gvm = R.wind_destagger_transpose(c.rh_u, c.rh_v, c.cosa, c.sina, torch.as_tensor(ys[0], device="cuda"), torch.as_tensor(ys[1], device="cuda"), nlev)
    gum, gvm = gum.cpu().numpy(), gvm.cpu().numpy()
    parts = [fwd[0] * ys[0], fwd[1] * ys[1], um * gum, vm * gvm]
    resid = abs((parts[0].sum() + parts[1].sum()) - (parts[2].sum() + parts[3].sum()))
    bound = 1e-9 * (np.abs(ys[0]).sum() + np.abs(ys[1]).sum()) + 1e-11 * sum(np.abs(p).sum() for p in parts)
    print("oracle dot product: residual %.3e, bound %.3e" % (resid, bound))
    assert resid <= bound


# ---- 7. autograd ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", ["float64", "float32"])
def test_autograd_rotated_with_the_mass_winds(cases, out_dtype):
    import torch
    from mpassit_amd import regrid as R
    c = cases(65, 17)
    nlev, dt = 4, getattr(torch, out_dtype)
    um, vm = _rand(torch, (nlev, c.ny, c.nx), 61), _rand(torch, (nlev, c.ny, c.nx), 62)
    plain = R.wind_destagger(c.rh_u, c.rh_v, c.cosa, c.sina, um, vm, nlev, out_dtype=dt, keep_mass=True)
    ua, va = um.clone().requires_grad_(True), vm.clone().requires_grad_(True)
    res = R.wind_destagger_autograd(c.rh_u, c.rh_v, c.cosa, c.sina, ua, va, nlev, out_dtype=dt, keep_mass=True)
    assert len(res) == 4
    for r, p in zip(res, plain):
        assert _same_bits(torch, r.detach(), p)
    assert res[0].dtype == dt and res[2].dtype == torch.float64
    ys = [_rand(torch, tuple(r.shape), 70 + i, r.dtype) for i, r in enumerate(res)]
    sum((r * y).sum().double() for r, y in zip(res, ys)).backward()
    want = R.wind_destagger_transpose(c.rh_u, c.rh_v, c.cosa, c.sina, ys[0], ys[1], nlev, g_umass_rot=ys[2], g_vmass_rot=ys[3])
    for g, w, x in zip((ua.grad, va.grad), want, (um, vm)):
        assert g.dtype == torch.float64 and g.shape == x.shape and _same_bits(torch, g, w)
    # without keep_mass the 4-tuple ends in None, None and the gradient is the transpose of (y_U, y_V) alone
    ua.grad = va.grad = None
    res = R.wind_destagger_autograd(c.rh_u, c.rh_v, c.cosa, c.sina, ua, va, nlev, out_dtype=dt)
    assert res[2] is None and res[3] is None
    ((res[0] * ys[0]).sum().double() + (res[1] * ys[1]).sum().double()).backward()
    want = R.wind_destagger_transpose(c.rh_u, c.rh_v, c.cosa, c.sina, ys[0], ys[1], nlev)
    assert _same_bits(torch, ua.grad, want[0]) and _same_bits(torch, va.grad, want[1])


def test_autograd_single_component(cases):
    import torch
    from mpassit_amd import regrid as R
    c = cases(33, 9)
    nlev = 2
    um, vm = _rand(torch, (nlev, c.ny, c.nx), 63), _rand(torch, (nlev, c.ny, c.nx), 64)
    ua, va = um.clone().requires_grad_(True), vm.clone().requires_grad_(True)
    # U alone, V's mass wind not given
    res = R.wind_destagger_autograd(c.rh_u, None, None, None, ua, None, nlev)
    plain = R.wind_destagger(c.rh_u, None, None, None, um, None, nlev)
    assert res[1] is None and res[2] is None and res[3] is None and _same_bits(torch, res[0].detach(), plain[0])
    y = _rand(torch, tuple(res[0].shape), 65)
    (res[0] * y).sum().backward()
    want = R.wind_destagger_transpose(c.rh_u, None, None, None, y, None, nlev)
    assert want[1] is None and _same_bits(torch, ua.grad, want[0])
    # V alone with both mass winds given: U's takes no part, its gradient is None
    res = R.wind_destagger_autograd(None, c.rh_v, None, None, ua, va, nlev)
    y = _rand(torch, tuple(res[1].shape), 66)
    g = torch.autograd.grad((res[1] * y).sum(), [ua, va], allow_unused=True)
    want = R.wind_destagger_transpose(None, c.rh_v, None, None, None, y, nlev)
    assert g[0] is None and want[0] is None and g[1].dtype == torch.float64 and _same_bits(torch, g[1], want[1])


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(cases):
    import torch
    from mpassit_amd import _lib as L, regrid as R
    c, other, polar = cases(64, 16), cases(65, 17), cases(73, 37, "lat-lon")
    nlev = 2
    gu, gv = _grads(torch, c, nlev, 81)
    gum, gvm = torch.zeros((nlev, c.ny, c.nx), dtype=torch.float64, device="cuda"), torch.zeros((nlev, c.ny, c.nx), dtype=torch.float64, device="cuda")
    extra = torch.zeros_like(gum)
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None   # noqa: E731
    hu, hv, ca, sa = c.rh_u._h, c.rh_v._h, c.cosa, c.sina

    def call(h1, h2, cosa, sina, a, b, src_type, ld, n, ar, br, oa, ob):
        rc = L.wind_destagger_transpose_dev(h1, h2, p(cosa), p(sina), p(a), p(b), src_type, ld, n, p(ar), p(br), p(oa), p(ob), None)
        return rc, L.load().mpg_last_error().decode()
    bad, unsup = L.MPG_ERR_INVALID_ARG, L.MPG_ERR_UNSUPPORTED
    assert call(hu, hv, ca, sa, gu, gv, 0, 0, nlev, None, None, gum, gvm)[0] == 0                       # the call that is then spoilt
    assert call(None, None, None, None, gu, gv, 0, 0, nlev, None, None, gum, gvm)[0] == bad            # both handles NULL
    assert call(hu, hv, ca, None, gu, gv, 0, 0, nlev, None, None, gum, gvm)[0] == bad                  # cosa without sina
    assert call(hu, hv, None, sa, gu, gv, 0, 0, nlev, None, None, gum, gvm)[0] == bad                  # ... and the reverse
    assert call(hu, None, ca, sa, gu, gv, 0, 0, nlev, None, None, gum, gvm)[0] == bad                  # rotation without both handles
    assert call(hu, hv, None, None, gu, gv, 0, 0, nlev, extra, None, gum, gvm)[0] == bad               # gumass_rot without rotation
    assert call(hu, hv, None, None, gu, gv, 0, 0, nlev, None, extra, gum, gvm)[0] == bad
    assert call(hu, hv, ca, sa, gu, gv, 0, 0, 0, None, None, gum, gvm)[0] == bad                       # nlev < 1
    assert call(hu, hv, ca, sa, gu, gv, 0, max(c.rh_u.n_dst, c.rh_v.n_dst) - 1, nlev, None, None, gum, gvm)[0] == bad   # stride below the larger plane
    assert call(hu, hv, ca, sa, gu, gv, 0, 0, nlev, None, None, gu, gvm)[0] == bad                     # an output that is an input
    assert call(hu, hv, ca, sa, gu, gv, 0, 0, nlev, extra, None, extra, gvm)[0] == bad
    assert call(hu, hv, ca, sa, gu, gv, 0, 0, nlev, None, None, gum, ca)[0] == bad
    assert call(hu, hv, ca, sa, gu, gv, 0, 0, nlev, None, None, gum, gum)[0] == bad
    assert call(hu, hv, ca, sa, None, gv, 0, 0, nlev, None, None, gum, gvm)[0] == bad                  # a NULL array that is needed
    assert call(hu, hv, ca, sa, gu, gv, 0, 0, nlev, None, None, gum, None)[0] == bad
    assert call(hu, hv, ca, sa, gu, gv, 4, 0, nlev, None, None, gum, gvm)[0] == bad                    # no such type
    assert call(hu, hv, ca, sa, gu, gv, 2, 0, nlev, None, None, gum, gvm)[0] == unsup                  # MPG_TYPE_BE
    fwd_text = "mpg_wind_destagger: the handles are not the CENTER -> EDGE1 / EDGE2 pair of one grid"
    assert call(hv, hu, None, None, gu, gv, 0, 0, nlev, None, None, gum, gvm) == (unsup, fwd_text)     # EDGE2 handle in the EDGE1 slot
    assert call(hu, other.rh_v._h, None, None, gu, gv, 0, 0, nlev, None, None, gum, gvm) == (unsup, fwd_text)   # two grids
    # a rotation under pole caps, as in the forward (the angles' values do not matter: nothing is launched)
    pgu, pgv = _grads(torch, polar, nlev, 82)
    pa = torch.ones((polar.ny, polar.nx), dtype=torch.float64, device="cuda")
    po = torch.zeros((nlev, polar.ny, polar.nx), dtype=torch.float64, device="cuda")
    assert call(polar.rh_u._h, polar.rh_v._h, pa, pa.clone(), pgu, pgv, 0, 0, nlev, None, None, po, po.clone())[0] == unsup
    # no refused call wrote: the outputs still hold what the one valid call left
    torch.cuda.synchronize()
    after = _fused(R, c, True, "uv", gu, gv, nlev)
    assert _same_bits(torch, gum, after[0]) and _same_bits(torch, gvm, after[1]), "the first, valid call's results; no refused call wrote"
    # the rotation's own refusals
    assert L.rotate_winds_transpose_dev(c.nx * c.ny, nlev, p(ca), None, p(gum), p(gvm), None) == bad
    assert L.rotate_winds_transpose_dev(c.nx * c.ny, 0, p(ca), p(sa), p(gum), p(gvm), None) == bad
    # the wrappers' own
    with pytest.raises(ValueError):
        R.wind_destagger_transpose(c.rh_u, c.rh_v, c.cosa, None, gu, gv, nlev)                         # cosa without sina
    with pytest.raises(ValueError):
        R.wind_destagger_transpose(c.rh_u, c.rh_v, None, None, gu.to(torch.float16), gv.to(torch.float16), nlev)   # wrong dtype
    with pytest.raises(ValueError):
        R.wind_destagger_transpose(c.rh_u, c.rh_v, None, None, gu, gv.float(), nlev)                   # two dtypes
    with pytest.raises(ValueError):
        R.wind_destagger_transpose(c.rh_u, c.rh_v, None, None, gu, gv[:, :-1, :].contiguous(), nlev)   # wrong shape
    with pytest.raises(ValueError):
        R.wind_destagger_transpose(c.rh_u, c.rh_v, c.cosa, c.sina, gu, gv, nlev, g_umass_rot=extra.float())
    with pytest.raises(ValueError):
        R.rotate_winds_cgrid_transpose(c.cosa, c.sina, gum.float(), gvm.float())
    with pytest.raises(ValueError):
        R.rotate_winds_cgrid_transpose(c.cosa, c.sina, gum[:, :-1].contiguous(), gvm[:, :-1].contiguous())
    with pytest.raises(L.MpgError) as e:
        R.wind_destagger_transpose(c.rh_v, c.rh_u, None, None, gv, gu, nlev)
    assert e.value.rc == unsup


# ---- 9. graph capture -------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_same_bits(cases):
    import torch
    from mpassit_amd import regrid as R
    c = cases(203, 35)
    nlev = 3
    gu, gv = _grads(torch, c, nlev, 91, torch.float32)
    gur = _rand(torch, (nlev, c.ny, c.nx), 92)
    outs = tuple(torch.full((nlev, c.ny, c.nx), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2))
    _fused(R, c, True, "uv", gu, gv, nlev)        # the first call builds the transposed indices
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):        # one stream: a chain, no parallel branches
            _fused(R, c, True, "uv", gu, gv, nlev, gur, None, outs=outs)
    for trial in range(2):
        gu.mul_(-0.5).add_(0.25)
        gv.mul_(0.75).sub_(1.0)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in outs]
        want = _fused(R, c, True, "uv", gu, gv, nlev, gur, None)
        torch.cuda.synchronize()
        assert _same_bits(torch, got[0], want[0]) and _same_bits(torch, got[1], want[1])
