"""target_grid.rotate_winds_transpose_at, the numpy mirror of mpg_rotate_winds_transpose_dev, is the transpose of rotate_winds_cgrid:
<R x, y> == <x, R^T y> with the forward written inline from the header (interp.F90:737-748) on 1e5 random points, within
1e-11 * sum|terms| -- the bound test_wind_to_mesh_gpu.py holds its dot products to."""
import numpy as np


def _forward(ca, sa, uo, vo):
    """include/mpassit_amd.h, mpg_rotate_winds: tana = sa / ca; den = ca + sa * tana; un = (uo + vo * tana) / den; vn = (vo - un * sa) / ca."""
    tana = sa / ca
    den = ca + sa * tana
    un = (uo + vo * tana) / den
    vn = (vo - un * sa) / ca
    return un, vn


def _case(n=100000, seed=5):
    rng = np.random.default_rng(seed)
    alpha = rng.uniform(-1.2, 1.2, n)            # a Lambert grid's angle stays well inside (-pi/2, pi/2): ca > 0
    ca, sa = np.cos(alpha), np.sin(alpha)
    x = [(rng.random(n) - 0.5) * 60.0 for _ in range(2)]
    y = [rng.standard_normal(n) for _ in range(2)]
    return ca, sa, x, y


def test_mirror_is_the_transpose_of_the_forward():
    from mpassit_amd import target_grid as tg
    ca, sa, (uo, vo), (yu, yv) = _case()
    un, vn = _forward(ca, sa, uo, vo)
    gu, gv = tg.rotate_winds_transpose_at(ca, sa, yu, yv)
    lhs = un * yu + vn * yv
    rhs = uo * gu + vo * gv
    resid = abs(float(np.sum(lhs)) - float(np.sum(rhs)))
    terms = float(np.sum(np.abs(un * yu)) + np.sum(np.abs(vn * yv)) + np.sum(np.abs(uo * gu)) + np.sum(np.abs(vo * gv)))
    print("dot-product residual %.3e, bound %.3e" % (resid, 1e-11 * terms))
    assert resid <= 1e-11 * terms
    # what the expressions amount to: the rotation by -alpha turned round
    assert np.max(np.abs(gu - (yu * ca - yv * sa))) < 1e-13 and np.max(np.abs(gv - (yu * sa + yv * ca))) < 1e-13


def test_mirror_returns_new_arrays_and_reuses_the_angles_over_levels():
    from mpassit_amd import target_grid as tg
    ca, sa, _, (yu, yv) = _case(n=6 * 7, seed=2)
    ca, sa = ca.reshape(6, 7), sa.reshape(6, 7)
    g = np.stack([yu.reshape(6, 7), 2.0 * yu.reshape(6, 7), yv.reshape(6, 7)])
    h = np.stack([yv.reshape(6, 7), yu.reshape(6, 7), -yv.reshape(6, 7)])
    g0, h0 = g.copy(), h.copy()
    gu, gv = tg.rotate_winds_transpose_at(ca, sa, g, h)
    assert np.array_equal(g, g0) and np.array_equal(h, h0) and gu is not g and gv is not h
    assert gu.shape == g.shape and gv.shape == h.shape and gu.dtype == np.float64
    for k in range(3):
        a, b = tg.rotate_winds_transpose_at(ca, sa, g[k], h[k])
        assert np.array_equal(a, gu[k]) and np.array_equal(b, gv[k])


def test_mirror_follows_ieee_for_a_zero_cosine_and_non_finite_inputs():
    from mpassit_amd import target_grid as tg
    ca = np.array([0.0, -0.0, 1.0, 0.8])
    sa = np.array([1.0, 1.0, 0.0, 0.6])
    gu, gv = tg.rotate_winds_transpose_at(ca, sa, np.array([1.0, 1.0, np.inf, 2.0]), np.array([1.0, 1.0, 3.0, 1.0]))
    assert np.isnan(gu[0]) and np.isnan(gu[1])        # a = +-inf, t = +-inf, b = -+inf, den = +-inf: inf / inf
    assert gu[2] == np.inf and np.isnan(gv[2])        # b = inf, guo = inf, p = inf * 0
    assert np.isfinite(gu[3]) and np.isfinite(gv[3])  # a point's trouble stays its own
