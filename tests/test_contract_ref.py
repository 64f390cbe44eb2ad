"""The host restatement of the header's arithmetic (tests/c/contract_ref.c through tests/_contract_ref.py), tested on the CPU before
anything on a GPU is held to it:

  * its fma is exact on the machine the test runs on (against rational arithmetic);
  * hand-made rows on which fma(w, x, acc) and w * x + acc differ come out as the header's expression, step by step in rational
    arithmetic with one rounding per written operation;
  * it agrees with the tolerance references the suite already trusts (_masked_ref.masked_ref, _large_offsets_ref.apply_ref) within
    their own published bounds;
  * the inputs of tests/test_contract_gpu.py can tell the contract from five deliberately wrong recipes: the shares of differing
    outputs are printed and each must reach 1 %.  The patterns here are the from_weights pattern of the GPU test itself, the saved
    patterns of its small Stores and fixed patterns that need no Store; the GPU test repeats the same check, reference against reference,
    on the patterns of all its Stores;
  * the restatements of the transpose, the rotation and the Grid -> Grid wind chain equal independent numpy statements of the same
    sentences (a loop of cr.fma_vec over a stable sort by source; plain float64 numpy, which neither fuses nor reorders), the transpose
    lies within _transpose_ref.transpose_ref's bound of the long-double sum, its inputs tell a reversed segment and a separate multiply
    and add from the contract, and the special grid values and mass winds reach every field while 90 % of the outputs stay finite."""
import math
from fractions import Fraction as F

import numpy as np
import pytest

import _contract_ref as cr

MIN_SHARE = 0.01


def rf(q):
    """a rational rounded to float64, to nearest even, overflow to infinity"""
    try:
        return float(q)
    except OverflowError:
        return math.inf if q > 0 else -math.inf


def exact_fma(a, b, c):
    """fma(a, b, c) for finite arguments from rational arithmetic, with IEEE 754's rule for the sign of an exact zero"""
    p = F(a) * F(b)
    s = p + F(c)
    if s != 0:
        return rf(s)
    if p == 0 and c == 0:                                  # (+-0) + (+-0): the common sign, +0 when they differ
        neg_p = (math.copysign(1.0, a) < 0) != (math.copysign(1.0, b) < 0)
        return -0.0 if neg_p and math.copysign(1.0, c) < 0 else 0.0
    return 0.0                                              # x + (-x) rounds to nearest: +0


def same_float(x, y):
    return (math.isnan(x) and math.isnan(y)) or (x == y and math.copysign(1.0, x) == math.copysign(1.0, y))


def test_the_reference_fma_is_exact_here():
    rng = np.random.default_rng(11)
    triples = []
    for _ in range(1500):
        a, b = (float(rng.normal() * 2.0 ** rng.integers(-40, 40)) for _ in range(2))
        triples.append((a, b, float(rng.normal() * 2.0 ** rng.integers(-80, 80))))
        c = -(a * b)                                        # cancellation: the rounded product and its neighbours
        triples += [(a, b, c), (a, b, float(np.nextafter(c, math.inf))), (a, b, float(np.nextafter(c, -math.inf)))]
    for _ in range(300):                                    # subnormal results
        a, b = float(rng.normal() * 2.0 ** rng.integers(-540, -500)), float(rng.normal() * 2.0 ** rng.integers(-540, -520))
        triples += [(a, b, 0.0), (a, b, float(rng.normal() * 5e-324 * 2.0 ** rng.integers(0, 30))), (a, b, -(a * b))]
    for _ in range(200):                                    # overflow, and a finite result of an overflowing product
        a, b = float(rng.normal() * 2.0 ** rng.integers(500, 520)), float(rng.normal() * 2.0 ** rng.integers(500, 520))
        triples += [(a, b, 1.0), (a, b, -math.copysign(1.7e308, a * b)), (1.7e308, 1.0, 1.7e308), (-1.7e308, 1.0, -1.7e308)]
    for za in (0.0, -0.0):
        for zb in (0.0, -0.0):
            for c in (0.0, -0.0, 3.5, -3.5):
                triples += [(za, zb, c), (za, 7.0, c), (7.0, zb, c)]
    triples += [(1.5, 2.0, -3.0), (-1.5, 2.0, 3.0), (5e-324, 0.5, 0.0), (5e-324, 0.5, 5e-324), (5e-324, -0.5, 0.0)]
    assert len(triples) > 5000
    got = cr.fma_vec(*[np.array(x) for x in zip(*triples)])
    bad = [(t, g, exact_fma(*t)) for t, g in zip(triples, got) if not same_float(float(g), exact_fma(*t))]
    assert not bad, "the host fma is not exact here: %d of %d triples, first %r" % (len(bad), len(triples), bad[0])
    assert all(same_float(cr.fma(*t), float(g)) for t, g in list(zip(triples, got))[:50])
    assert math.isnan(cr.fma(math.inf, 0.0, 1.0)) and math.isnan(cr.fma(1.0, math.inf, -math.inf)) and cr.fma(2.0, math.inf, 1.0) == math.inf


# ---- hand-made rows: fma(w, x, acc) differs from w * x + acc -----------------------------------------------------------------------
E = 2.0 ** -30
ROW_W = [-1.0, 1.0 + E, 2.0 ** -70, 2.0 ** -40, 0.5]
ROW_X = [1.0, 1.0 + E, 3.0, 1.0 + E, 2.0 ** -50]     # (1 + E)^2 = 1 + 2^-29 + 2^-60: the product needs 61 bits


def _chain_exact(ws, xs):
    acc = 0.0
    for w, x in zip(ws, xs):
        acc = exact_fma(w, x, acc)
    return acc


def _chain_muladd(ws, xs):
    acc = 0.0
    for w, x in zip(ws, xs):
        acc = w * x + acc
    return acc


def test_hand_made_rows_follow_the_header():
    src = np.array(ROW_X + [9.0])
    # three slots: fma(w2, e, fma(w1, b, w0 * a)) -- the first product rounded on its own
    w3, x3 = ROW_W[:3], ROW_X[:3]
    p3 = cr.Pattern(6, 2, 3, idx=[[0, 1, 2], [-1, -1, -1]], w=[w3, [0.0] * 3])
    want3 = exact_fma(w3[2], x3[2], exact_fma(w3[1], x3[1], rf(F(w3[0]) * F(x3[0]))))
    assert want3 == 2.0 ** -29 + 2.0 ** -60 + 3 * 2.0 ** -70 and want3 != (w3[0] * x3[0] + w3[1] * x3[1]) + w3[2] * x3[2]
    got = cr.apply(p3, src, epilogue=False)
    assert same_float(float(got[0, 0, 0]), want3) and same_float(float(got[0, 0, 1]), 0.0), got
    assert not same_float(float(cr.apply(p3, src, epilogue=False, variant=cr.MULADD)[0, 0, 0]), want3)
    assert not same_float(float(cr.apply(p3, src, epilogue=False, variant=cr.REVERSED)[0, 0, 0]), want3)
    # four slots: the chain from 0.0
    w4, x4 = ROW_W[:4], ROW_X[:4]
    p4 = cr.Pattern(6, 1, 4, idx=[[0, 1, 2, 3]], w=[w4])
    want4 = _chain_exact(w4, x4)
    assert want4 != _chain_muladd(w4, x4)
    assert same_float(float(cr.apply(p4, src, epilogue=False)[0, 0, 0]), want4)
    # CSR: stored order, here neither ascending nor descending, a repeated column and a stored zero among the entries
    order = [0, 4, 1, 2, 3, 1, 5]
    ws = [ROW_W[0], ROW_W[4], ROW_W[1], ROW_W[2], ROW_W[3], 2.0 ** -45, 0.0]
    pc = cr.Pattern(6, 4, 0, rowptr=[0, 0, len(order), len(order), len(order) + 3], col=order + [1, 0, 2], val=ws + [ROW_W[1], ROW_W[0], ROW_W[2]])
    wantc = _chain_exact(ws, [float(src[c]) for c in order])
    assert wantc != _chain_muladd(ws, [float(src[c]) for c in order])
    got = cr.apply(pc, src, epilogue=False)
    assert same_float(float(got[0, 0, 1]), wantc) and same_float(float(got[0, 0, 0]), 0.0) and same_float(float(got[0, 0, 2]), 0.0)
    # a row stored as columns 1, 0, 2: in stored order the product (1 + E)^2 is rounded before -1 arrives, in ascending order after
    assert same_float(float(got[0, 0, 3]), 2.0 ** -29 + 3 * 2.0 ** -70)
    assert same_float(float(cr.apply(pc, src, epilogue=False, variant=cr.COLSORT)[0, 0, 3]), want3)
    # the epilogue is one fma and one cast, on unmapped points and empty rows too, per-field offsets, both destination types and orders
    src2 = np.concatenate([src, 2.0 * src])
    for pat, acc in ((p3, want3), (p4, want4)):
        for dt in (np.float64, np.float32):
            for lev_fast in (False, True):
                got = cr.apply(pat, src2, 1, 2, dst_dtype=dt, dst_lev_fast=lev_fast, scale=9.81, offset=[-300.0, 7.0])
                assert got.dtype == dt and same_float(float(got[0, 0, 0]), float(dt(exact_fma(acc, 9.81, -300.0))))
                assert same_float(float(got[1, 0, 0]), float(dt(exact_fma(2.0 * acc, 9.81, 7.0))))
    assert same_float(float(cr.apply(p3, src, scale=9.81, offset=-300.0)[0, 0, 1]), -300.0)
    assert same_float(float(cr.apply(pc, src, scale=9.81, offset=-300.0)[0, 0, 0]), -300.0)
    # layouts: [src][lev] sources and [point][lev] results hold the same bits
    s = cr.ordinary(6, 5, 2)
    a = cr.apply(pc, s, 5, 2)
    b = cr.apply(pc, s.transpose(0, 2, 1).copy(), 5, 2, src_lev_fast=True, dst_lev_fast=True)
    assert cr.same(a, b.transpose(0, 2, 1))
    assert cr.same(cr.apply(pc, s.astype(np.float32), 5, 2), cr.apply(pc, s.astype(np.float32).astype(np.float64), 5, 2))


def test_a_minus_zero_sum_with_and_without_epilogue():
    p3 = cr.Pattern(3, 2, 3, idx=[[0, 1, 2], [-1, -1, -1]], w=[[0.2, 0.3, 0.5], [0.0] * 3])
    p1 = cr.Pattern(3, 2, 1, idx=[[1], [-1]], w=[[1.0], [0.0]])
    p4 = cr.Pattern(4, 1, 4, idx=[[0, 1, 2, 3]], w=[[0.25] * 4])
    z = np.full(4, -0.0)
    for pat in (p3, p1):
        raw = cr.apply(pat, z[:3], epilogue=False)
        assert same_float(float(raw[0, 0, 0]), -0.0) and same_float(float(raw[0, 0, 1]), 0.0), "mpg_regrid_dev: -0.0 survives, unmapped is +0.0"
        epi = cr.apply(pat, z[:3], epilogue=True)
        assert same_float(float(epi[0, 0, 0]), 0.0) and same_float(float(epi[0, 0, 1]), 0.0), "fma(-0.0, 1, 0) is +0.0"
    assert same_float(float(cr.apply(p4, z, epilogue=False)[0, 0, 0]), 0.0), "a chain from +0.0 never gives -0.0"
    for mode, c, s in (("mesh", None, None), ("mesh", [1.0, 1.0], [0.0, 0.0]), ("edges", [0.0, 0.0], [1.0, 1.0])):
        for o in cr.wind_pair(mode, p1, p3, z[:3], z[:3], c, s, 1):
            assert same_float(float(o[0, 0]), 0.0) and same_float(float(o[0, 1]), 0.0)


def test_wind_formulas():
    p4 = cr.synthetic_fixed(4, 50, 40)
    p1 = cr.synthetic_fixed(1, 60, 40, seed=9)
    u, v = cr.ordinary(50, 3, 1)[0] - 280.0, cr.ordinary(60, 3, 1, seed=1)[0] - 280.0
    rng = np.random.default_rng(3)
    phi = rng.uniform(0, 2 * np.pi, 40)
    c, s = np.cos(phi), np.sin(phi)
    a, b = cr.apply(p4, u, 3)[0], cr.apply(p1, v, 3)[0]
    un = p4.unmapped | p1.unmapped
    for dt in (np.float64, np.float32):
        ue, ve = cr.wind_pair("mesh", p4, p1, u, v, c, s, 3, dt)
        en, et = cr.wind_pair("edges", p4, p1, u, v, c, s, 3, dt)
        pa, pb = cr.wind_pair("mesh", p4, p1, u, v, None, None, 3, dt)
        only, = cr.wind_pair("edges", p4, p1, u, v, c, s, 3, dt, tangential=False)
        for got, want in ((ue, a * c - b * s), (ve, a * s + b * c), (en, a * c + b * s), (et, b * c - a * s), (pa, a), (pb, b), (only, a * c + b * s)):
            assert cr.same(got, np.where(un, 0.0, want).astype(dt))
        lf = cr.wind_pair("mesh", p4, p1, u, v, c, s, 3, dt, dst_lev_fast=True)
        assert cr.same(lf[0].T, ue) and cr.same(lf[1].T, ve)


def test_masked_identity_and_recipe():
    """With nothing missing Wt / Wv == 1.0 and a mapped point has the bits of the unmasked Regrid with epilogue (1, 0); an unmapped point
    and an empty row are the fill.  A hand-made row checks Wt, Wv, N and the quotient one rounding at a time."""
    (_, _, _), fw = cr.from_weights_case()
    for pat in (cr.synthetic_fixed(3), cr.synthetic_fixed(4), cr.synthetic_fixed(1), fw):
        src = cr.ordinary(pat.n_src, 3, 2)
        for dt in (np.float64, np.float32):
            plain = cr.apply(pat, src, 3, 2, dst_dtype=dt)
            # a row whose stored weights are all zero has Wv = 0: undefined by the Wv > 0 rule
            dead = pat.unmapped if pat.nnz else pat.unmapped | (np.add.reduceat(np.abs(pat.val), np.minimum(pat.rowptr[:-1], pat.val.size - 1)) == 0)
            for frac in (0.0, 0.5, 1.0):
                m = cr.apply_masked(pat, src, 3, 2, dst_dtype=dt, min_valid_frac=frac, fill_value=-9999.0)
                assert cr.same(m[:, :, ~dead], plain[:, :, ~dead]) and (m[:, :, pat.unmapped] == -9999.0).all()
    w = [0.3, 0.1, 0.6]
    x = [281.0, float("nan"), 1.0 / 3.0]
    pat = cr.Pattern(3, 1, 3, idx=[[0, 1, 2]], w=[w])
    Wt, Wv = (w[0] + w[1]) + w[2], (w[0] + 0.0) + w[2]
    N = exact_fma(w[2], x[2], exact_fma(0.0, 0.0, w[0] * x[0]))
    want = exact_fma(N * (Wt / Wv), 9.81, -300.0)
    got = cr.apply_masked(pat, np.array(x), min_valid_frac=0.5, scale=9.81, offset=-300.0)
    assert same_float(float(got[0, 0, 0]), want)
    assert same_float(float(cr.apply_masked(pat, np.array(x), min_valid_frac=0.95, fill_value=5.0, scale=9.81, offset=-300.0)[0, 0, 0]), 5.0)
    got = cr.apply_masked(pat, np.array([281.0, 7.0, 1.0 / 3.0]), flags=2, missing_value=7.0, scale=9.81, offset=-300.0)
    assert same_float(float(got[0, 0, 0]), want)
    got = cr.apply_masked(pat, np.array([281.0, 7.0, 1.0 / 3.0]), flags=0, src_mask=[0, 1, 0], scale=9.81, offset=-300.0)
    assert same_float(float(got[0, 0, 0]), want)
    assert math.isinf(float(cr.apply_masked(pat, np.array([281.0, math.inf, 1.0]), flags=0)[0, 0, 0])), "Inf is not missing"


# ---- the references already trusted -------------------------------------------------------------------------------------------------
def _small_patterns():
    (_, _, _), fw = cr.from_weights_case()
    return [("3 slots", cr.synthetic_fixed(3, 301, 200)), ("4 slots", cr.synthetic_fixed(4, 301, 200)), ("1 slot", cr.synthetic_fixed(1, 301, 200)),
            ("from_weights", fw)]


@pytest.mark.parametrize("what,pat", _small_patterns(), ids=lambda v: v if isinstance(v, str) else "")
def test_agrees_with_the_masked_reference(what, pat):
    from _masked_ref import masked_ref, check_masked
    nlev = 3
    src = cr.ordinary(pat.n_src, nlev, 1)[0]
    rng = np.random.default_rng(8)
    src[rng.random(src.shape) < 0.15] = np.nan
    src[rng.random(src.shape) < 0.05] = -9999.0
    mask = rng.random(pat.n_src) < 0.1
    for frac in (0.0, 0.5, 1.0):
        for sdt in (np.float64, np.float32):
            s = src.astype(sdt)
            ref = masked_ref(pat, s, nan=True, missing_value=-9999.0, src_mask=mask, min_valid_frac=frac)
            for ddt in (np.float64, np.float32):
                for scale, offset in ((1.0, 0.0), cr.EPI):
                    got = cr.apply_masked(pat, s, nlev, 1, dst_dtype=ddt, flags=3, missing_value=-9999.0, src_mask=mask, min_valid_frac=frac,
                                          fill_value=float("nan"), scale=scale, offset=offset)
                    check_masked(got[0], ref, float("nan"), (what, frac, sdt, ddt, scale), scale=scale, offset=offset)
                    # "defined" is an exact restatement on both sides: no output may be left to the edge set
                    assert np.array_equal(np.isnan(got[0]), ~ref.defined), (what, frac)


@pytest.mark.parametrize("what,pat", _small_patterns(), ids=lambda v: v if isinstance(v, str) else "")
def test_agrees_with_the_large_offsets_reference(what, pat):
    import torch
    import _large_offsets_ref as lo
    nlev = 5
    W = lo.Weights(torch, pat.n_src, pat.n_dst, idx=pat.idx if pat.nnz else None, w=pat.w if pat.nnz else None,
                   rowptr=None if pat.nnz else pat.rowptr, col=None if pat.nnz else pat.col, val=None if pat.nnz else pat.val)
    src = cr.ordinary(pat.n_src, nlev, 1)[0]
    xmax = float(np.abs(src).max())
    for sdt in (np.float64, np.float32):
        cf = np.ascontiguousarray(src.astype(sdt))
        for lev_fast, s in ((False, cf), (True, np.ascontiguousarray(cf.T))):
            for dst_rows in (False, True):
                for ddt in (np.float64, np.float32):
                    for scale, offset in ((1.0, 0.0), cr.EPI):
                        got = cr.apply(pat, s, nlev, 1, src_lev_fast=lev_fast, dst_dtype=ddt, dst_lev_fast=dst_rows, scale=scale, offset=offset)
                        worst = lo.compare(W, torch.from_numpy(got.reshape(-1)), torch.from_numpy(s.reshape(-1)), nlev, lev_fast, dst_rows=dst_rows,
                                           scale=scale, offset=offset, xmax=xmax, what=str((what, sdt, lev_fast, dst_rows, ddt, scale)))
                        assert worst <= 1.0


# ---- the inputs can tell the contract from its neighbours ----------------------------------------------------------------------------
def _report(what, shares):
    for name, share in shares.items():
        print("%-28s %-62s %6.2f %%" % (what, name, 100.0 * share))
    low = {k: v for k, v in shares.items() if not k.endswith("[info]") and v < MIN_SHARE}
    assert not low, "%s: these inputs cannot tell the contract from %r" % (what, low)


def test_the_inputs_can_tell_the_difference():
    """On the source arrays test_contract_gpu.py uses (cr.ordinary with the pattern's n_src, two fields, 17 levels, float64) and the
    patterns that need no Store: the from_weights pattern of the GPU test, whose rows are stored in shuffled and descending column order,
    and fixed patterns of 3, 4 and 1 slots.  The all -0.0 input of the skipped-epilogue recipe must differ on EVERY qualifying point."""
    (_, _, _), fw = cr.from_weights_case()
    lens = np.diff(fw.rowptr)
    assert fw.n_dst == 210 and fw.n_dst % 64 and {0, 1, 1024, 1025, 2049} <= set(lens.tolist())
    assert lens[64] == 1024 and lens[128] == 1025 and lens[192] == 2049 and lens[0] == 0 and lens[1] == 1
    assert len(set(fw.col[fw.rowptr[2]:fw.rowptr[3]].tolist())) == 1 and lens[2] > 1, "a row that repeats one column"
    assert (fw.val == 0.0).sum() == 1 and (np.diff(fw.col[fw.rowptr[4]:fw.rowptr[5]]) < 0).all()
    saved = [("saved Store pattern: " + k, v) for k, v in cr.golden_patterns().items()]
    for what, pat in [("from_weights CSR", fw), ("fixed, 3 slots", cr.synthetic_fixed(3)), ("fixed, 4 slots", cr.synthetic_fixed(4)),
                      ("fixed, 1 slot", cr.synthetic_fixed(1))] + saved:
        shares = cr.recipe_shares(pat, cr.ordinary(pat.n_src, 17, 2), 17, 2)
        _report(what, shares)
        if "epilogue skipped at (1, 0)" in shares:
            assert shares["epilogue skipped at (1, 0)"] == 1.0
    assert set(cr.recipe_shares(fw, cr.ordinary(fw.n_src, 2, 2), 2, 2)) >= {"slots reversed", "separate multiply and add", "CSR row in ascending-column order"}


def test_the_special_sources_stay_informative():
    (_, _, _), fw = cr.from_weights_case()
    pats = [fw, cr.synthetic_fixed(3), cr.synthetic_fixed(4), cr.synthetic_fixed(1)] + list(cr.golden_patterns().values())
    for pat in pats:
        for nlev in (1, 2, 17, 65):
            for seed in (0, 1):
                x, where = cr.special(pat, nlev, 2, seed)
                assert sum(int(m.sum()) for m in where.values()) / x.size <= 0.03 or x.size < 2000
                assert any(m[0, 0, 0] for m in where.values()) and any(m[0, 0, -1] for m in where.values())
                for name, v in cr.SPECIALS:
                    assert where[name].any() and all(same_float(float(e), v) for e in x[where[name]][:3])
                for s in (x, cr.to_f32(x)):
                    cr.special_is_informative(pat, s, where, nlev, 2)
            y, wy = cr.special(pat, nlev, 2, with_nan=False)
            assert not np.isnan(y).any()
            cr.special_is_informative(pat, y, wy, nlev, 2, [k for k, _ in cr.SPECIALS if k != "nan"])


def test_pole_cap_rows_with_one_huge_value_are_held():
    """only a row whose sum of absolute values overflows is exempt from the cap bound"""
    pat = cr.golden_patterns()["pole 4"]
    pat.pole = (np.array([5, 2600], np.int32), np.array([0, pat.n_src - 72], np.int32), np.array([0.25, 0.5]), 72)
    x = cr.ordinary(pat.n_src, 2, 1)
    x[0, 0, 3] = 1.7e308
    x[0, 1, pat.n_src - 2], x[0, 1, pat.n_src - 9] = 1.7e308, -1.7e308
    pts, want, bound, must_nan, free = cr.pole_caps(pat, x, 2, 1, False, np.float64, True, 1.0, 0.0)
    assert free.tolist() == [[[False, False], [False, True]]] and not must_nan.any()
    assert np.isfinite(bound[0, 0, 0]) and 1e305 < want[0, 0, 0] < 1e306 and np.isfinite(bound[0, 1, 0])


# ---- the transpose, the rotation and the Grid -> Grid wind chain ---------------------------------------------------------------------
def _transpose_patterns():
    (_, _, _), fw = cr.from_weights_case()
    (_, _, _), syn = cr.synthetic_transpose_case()
    return [("saved Store pattern: " + k, v) for k, v in cr.golden_patterns().items()] + [("from_weights CSR", fw), ("synthetic segments", syn)]


class _AsHandle:
    """what _transpose_ref.transpose_ref reads of a RouteHandle, from a Pattern (no pole caps: the saved patterns carry none)"""

    def __init__(self, pat):
        self.pat, self.n_src, self.n_dst, self.nnz_per_row = pat, pat.n_src, pat.n_dst, pat.nnz

    def weights(self):
        return self.pat.weights()

    def csr(self):
        return self.pat.csr()

    def pole(self):
        return np.empty(0, np.int32), np.empty(0, np.int32), np.empty(0), 0

    def to_esmf_weights(self):
        pt = cr.transposed(self.pat)
        col = np.repeat(np.arange(pt.n_dst), np.diff(pt.rowptr))
        return pt.col + 1, col + 1, pt.val


def _transpose_by_numpy(pat, g, nlev, nfields):
    """acc[c] = fma(w_j, g[row_j], acc[c]) entry by entry with cr.fma_vec, the segments taken from a stable sort by source"""
    pt = cr.transposed(pat)
    lens = np.diff(pt.rowptr)
    acc = np.zeros((nfields, nlev, pat.n_src))
    g = np.asarray(g, np.float64).reshape(nfields, nlev, pat.n_dst)
    for j in range(int(lens.max())):
        sel = np.nonzero(lens > j)[0]
        e = pt.rowptr[sel] + j
        acc[:, :, sel] = cr.fma_vec(pt.val[e][None, None, :], g[:, :, pt.col[e]], acc[:, :, sel])
    return acc


def test_the_synthetic_handle_holds_the_listed_segments():
    (row, col, S), pat = cr.synthetic_transpose_case()
    lens = cr.segment_lengths(pat)
    assert set(cr.SYN_LENGTHS) <= set(lens.tolist()) and lens.max() == 300 and (0, 16, 17, 64, 65) == tuple(n for n in (0, 16, 17, 64, 65) if n in lens)
    assert pat.n_src == 41 and pat.n_src % 64 and 380 <= pat.n_dst <= 420 and pat.nnz == 0
    pairs = np.stack([row, col], axis=1)
    uniq, count = np.unique(pairs, axis=0, return_counts=True)
    assert count.max() >= 3 and (count > 1).sum() > 10, "duplicate (row, col) pairs"
    assert pat.rowptr[1] - pat.rowptr[0] == 1, "destination point 0 holds one entry"
    inside = np.setdiff1d(np.arange(pat.col.size - 1), pat.rowptr[1:-1] - 1)
    assert (np.diff(pat.col)[inside] < 0).any() and (np.diff(pat.col)[inside] > 0).any(), "rows are stored in no particular column order"


@pytest.mark.parametrize("what,pat", _transpose_patterns(), ids=lambda v: v if isinstance(v, str) else "")
def test_transpose_restatement(what, pat):
    from _transpose_ref import assert_f32_close, assert_f64_close, transpose_ref
    nlev, nf = 3, 2
    g = cr.ordinary(pat.n_dst, nlev, nf) - 250.0                 # both signs: cancellation inside a segment
    by_numpy = _transpose_by_numpy(pat, g, nlev, nf)
    got, cap = cr.transpose(pat, g, nlev, nf)
    assert cr.same(got, by_numpy) and not cap.any()
    assert cr.same(got, cr.apply(cr.transposed(pat), g, nlev, nf, epilogue=False)), "the CSR chain over the transposed pattern"
    assert (got[:, :, cr.segment_lengths(pat) == 0] == 0.0).all() and not np.signbit(got[:, :, cr.segment_lengths(pat) == 0]).any()
    assert cr.same(cr.transpose(pat, g, nlev, nf, dst_dtype=np.float32)[0], by_numpy.astype(np.float32))
    assert cr.same(cr.transpose(pat, g, nlev, nf, dst_lev_fast=True)[0], by_numpy.transpose(0, 2, 1))
    g32 = cr.to_f32(g)
    assert cr.same(cr.transpose(pat, g32, nlev, nf)[0], _transpose_by_numpy(pat, g32, nlev, nf))
    ld = pat.n_dst + 5                                            # pitched planes, NaN in the pad
    buf = np.full((nf * nlev, ld), np.nan)
    buf[:, :pat.n_dst] = g.reshape(nf * nlev, pat.n_dst)
    assert cr.same(cr.transpose(pat, buf, nlev, nf, g_level_stride=ld)[0], by_numpy)
    rh = _AsHandle(pat)
    for f in range(nf):
        want, bound = transpose_ref(rh, g[f])
        assert_f64_close(got[f], want, bound, what)
        assert_f32_close(cr.transpose(pat, g, nlev, nf, dst_dtype=np.float32)[0][f], want, bound, what)
    if cr.segment_lengths(pat).max() >= 3:
        assert not cr.same(cr.transpose(pat, g, nlev, nf, variant=cr.REVERSED)[0], got)


def test_transpose_cap_rows_and_nearest_weights():
    pat = cr.golden_patterns()["pole 4"]
    pat.pole = (np.array([5, 9, 2600], np.int32), np.array([0, 0, pat.n_src - 72], np.int32), np.array([0.25, 0.0, 0.5]), 72)
    _, cap = cr.transpose(pat, cr.ordinary(pat.n_dst, 1, 1))
    assert cap.sum() == 144 and cap[:72].all() and cap[-72:].all()
    pat.pole = (np.array([9], np.int32), np.array([0], np.int32), np.array([0.0]), 72)
    assert not cr.transpose(pat, cr.ordinary(pat.n_dst, 1, 1))[1].any(), "a cap of weight zero adds nothing"
    # a nearest handle's weight is 1.0 whatever its stored weight array holds
    p1 = cr.Pattern(3, 4, 1, idx=[[2], [0], [-1], [2]], w=[[0.5], [0.5], [0.0], [0.5]])
    got, _ = cr.transpose(p1, np.array([1.0, 2.0, 4.0, 8.0]))
    assert got.reshape(-1).tolist() == [2.0, 0.0, 9.0]


def test_transpose_inputs_can_tell_the_difference():
    """on the grid values test_contract_adjoint_gpu.py uses (cr.ordinary over the handle's n_dst, two fields, 17 levels): each wrong
    recipe that can change a source of the pattern changes at least 1 % of the outputs it can change"""
    listed = 0
    for what, pat in _transpose_patterns():
        shares = cr.transpose_shares(pat, cr.ordinary(pat.n_dst, 17, 2), 17, 2)
        _report(what + " (transpose)", shares)
        listed += len(shares)
    (_, _, _), syn = cr.synthetic_transpose_case()
    assert set(cr.transpose_shares(syn, cr.ordinary(syn.n_dst, 17, 2), 17, 2)) == {"segment reversed", "separate multiply and add"} and listed >= 8


def test_transpose_special_grid_values_stay_informative():
    for what, pat in _transpose_patterns():
        for nlev in (1, 2, 17, 65):
            x, where, pt = cr.special_g(pat, nlev, 2)
            assert np.isnan(x[:, :, 0]).all(), "a NaN at destination point 0 of every plane"
            for s in (x, cr.to_f32(x)):
                fin = cr.special_is_informative(pt, s, where, nlev, 2)
                reach = {name: int(np.isin(np.nonzero(m.reshape(-1, pt.n_src).any(axis=0))[0], pt.used).sum()) for name, m in where.items()}
                print("%-34s %2d levels %-8s finite %6.2f %%  points read per kind: %s" % (what, nlev, s.dtype, 100.0 * fin, sorted(reach.values())))


def test_rotation_is_plain_float64():
    rng = np.random.default_rng(6)
    for npts, nlev in ((1, 1), (257, 3), (1000, 65)):
        phi = rng.uniform(0.0, 2.0 * np.pi, npts)
        ca, sa = np.cos(phi), np.sin(phi)
        ca[::97], ca[5::101] = 0.0, -0.0
        u, v, where = cr.mass_winds(npts, 1, nlev, "special")
        gu, gv = cr.rotate(ca, sa, u, v)
        with np.errstate(all="ignore"):
            tana = sa / ca
            den = ca + sa * tana
            un = (u + v * tana) / den
            vn = (v - un * sa) / ca
        assert cr.same(gu, un) and cr.same(gv, vn) and (npts == 1 or len(where) == len(cr.SPECIALS))
        assert npts == 1 or (np.isfinite(gu).mean() > 0.9 and not np.isfinite(gu[:, ca == 0.0]).all())


def test_wind_chain_restatement():
    """cr_wind_destagger is cr_rotate, then the 4-slot chain, then the store of each result type -- on 4-slot patterns that need no Store"""
    nx, ny, nlev = 19, 11, 3
    n = nx * ny
    p1, p2 = cr.synthetic_fixed(4, n, (nx + 1) * ny), cr.synthetic_fixed(4, n, nx * (ny + 1), seed=9)
    rng = np.random.default_rng(12)
    phi = rng.uniform(-0.6, 0.6, n)
    ca, sa = np.cos(phi), np.sin(phi)
    ca[7], ca[100] = 0.0, -0.0
    for kind in ("ordinary", "special"):
        um, vm, where = cr.mass_winds(nx, ny, nlev, kind)
        for rot in (True, False):
            ru, rv = cr.rotate(ca, sa, um, vm) if rot else (um, vm)
            for dst_type in (0, 1, 2, 3):
                U, V, ku, kv = cr.wind_destagger(p1, p2, ca if rot else None, sa if rot else None, um, vm, nlev, dst_type, keep_mass=True)
                dt = np.float32 if dst_type & 1 else np.float64
                for got, pat, src in ((U, p1, ru), (V, p2, rv)):
                    want = cr.apply(pat, src, nlev, 1, dst_dtype=dt, epilogue=dst_type != 0)[0]
                    assert cr.same(cr.swap(got) if dst_type & 2 else got, want), (kind, rot, dst_type)
                    assert (cr.bits(got[:, pat.unmapped]) == 0).all(), "an unmapped point is +0.0, in either byte order"
                assert (ku is None) == (not rot) and (not rot or (cr.same(ku, ru) and cr.same(kv, rv)))
            if kind == "special":
                U, V, _, _ = cr.wind_destagger(p1, p2, ca if rot else None, sa if rot else None, um, vm, nlev)
                print("special mass winds, %s: finite %.2f %%" % ("rotated" if rot else "unrotated", 100.0 * cr.winds_are_informative(p1, p2, rot, where, U, V)))
    um, vm, _ = cr.mass_winds(nx, ny, nlev, "ordinary")
    U, V, _, _ = cr.wind_destagger(p1, None, None, None, um, None, nlev, 1)
    assert V is None and cr.same(U, cr.apply(p1, um, nlev, 1, dst_dtype=np.float32)[0])
    U, V, _, _ = cr.wind_destagger(None, p2, None, None, None, vm, nlev, 0, dst_level_stride=p2.n_dst + 7)
    assert U is None and cr.same(V[:, :p2.n_dst], cr.apply(p2, vm, nlev, 1, epilogue=False)[0]) and np.isnan(V[:, p2.n_dst:]).all()
    # the float64 entry keeps a -0.0 sum, a typed result stores fma(-0.0, 1, 0) = +0.0
    one = cr.Pattern(4, 1, 4, idx=[[0, 1, 2, 3]], w=[[-1.0, 0.0, 0.0, 0.0]])
    z = np.zeros((1, 4))
    assert np.signbit(cr.wind_destagger(one, None, None, None, z, None, 1, 0)[0][0, 0]) == np.signbit(cr.apply(one, z, epilogue=False)[0, 0, 0])
