"""The reference of the masked Regrid's adjoint (tests/_masked_transpose_ref.py) checked without a GPU: it is the adjoint by
construction -- the transposed dense Jacobian of the forward's own reference applied to a gradient -- and the test inputs tell the
contract from four wrong recipes on at least 1 % of the outputs, the bar of tests/test_contract_ref.py."""
import numpy as np
import pytest

import _contract_ref as cr
from _masked_ref import masked_ref
from _masked_transpose_ref import CASE_NLEV as NLEV, MUTANTS, gappy_case, jacobian_product, masked_transpose_ref

MIN_SHARE = 0.01


def test_defined_is_the_forward_references_decision():
    pat, src, mask, _, defined = gappy_case()
    ref = masked_ref(pat, src, src_mask=mask, min_valid_frac=0.5)
    assert np.array_equal(defined, ref.defined)
    undef_mapped = (~defined & ~pat.unmapped[None, :]).mean()      # (about a third of the 401 points hold no entry at all)
    assert 0.05 < undef_mapped and defined.mean() > 0.2 and pat.unmapped.any(), "the case needs defined, undefined and unmapped outputs"
    fwd = cr.apply_masked(pat, src, NLEV, 1, src_mask=mask, min_valid_frac=0.5)[0]
    assert np.array_equal(~np.isnan(fwd), defined), "the exact restatement of the forward fills other outputs"


@pytest.mark.parametrize("frac,scale", [(0.5, 1.0), (0.0, -2.5), (1.0, 1.0)])
def test_adjoint_by_construction(frac, scale):
    pat, src, mask, g, defined = gappy_case(frac=frac)
    got, h, d2 = masked_transpose_ref(pat, g, src[None], NLEV, 1, src_mask=mask, min_valid_frac=frac, scale=scale)
    assert np.array_equal(d2[0], defined)
    want, bound, ok = jacobian_product(pat, g, src, NLEV, src_mask=mask, min_valid_frac=frac, scale=scale)
    got = got[0]
    assert not np.isnan(got).any(), "a NaN of g at an undefined output reached a source"
    assert not np.isnan(h).any() and (cr.bits(h[0][~defined]) == 0).all(), "h is +0.0 at every undefined output"
    assert (cr.bits(got[~ok]) == 0).all(), "an invalid source is exactly +0.0"
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    bad = ~(err <= bound)
    assert not bad.any(), "%d outputs outside the bound, first %s: got %r want %r bound %r" % (
        int(bad.sum()), np.argwhere(bad)[0], got[bad][0], float(want[bad][0]), bound[bad][0])
    assert (np.abs(want[ok]) > 0).mean() > 0.5, "most valid sources must carry a gradient"


def test_no_gaps_is_the_unmasked_transpose():
    _, pat = cr.synthetic_transpose_case()
    g, _, _ = cr.special_g(pat, NLEV, 2, seed=1)
    src = cr.ordinary(pat.n_src, NLEV, 2, 3)
    for dt, lf in ((np.float64, False), (np.float32, True)):
        got, h, _ = masked_transpose_ref(pat, g, src, NLEV, 2, dst_dtype=dt, dst_lev_fast=lf)
        want, _ = cr.transpose(pat, g, NLEV, 2, dt, lf)
        mapped = ~pat.unmapped
        assert cr.same(h[:, :, mapped], g[:, :, mapped]), "Wt / Wv == 1.0: h is g"
        # the synthetic pattern has unmapped points, whose g the masked adjoint drops; no entry references them, so nothing else changes
        assert cr.same(got, want)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_inputs_tell_the_contract_from_a_wrong_recipe(mutant):
    pat, src, mask, g, defined = gappy_case()
    assert np.isnan(g[~defined]).all() and (~defined).any()
    want, _, _ = masked_transpose_ref(pat, g, src[None], NLEV, 1, src_mask=mask)
    got, _, _ = masked_transpose_ref(pat, g, src[None], NLEV, 1, src_mask=mask, variant=mutant)
    share = float(cr.differs(got, want).mean())
    print("%s: differs on %.1f %% of the outputs" % (mutant, 100.0 * share))
    assert share >= MIN_SHARE, "%s differs on %.2f %% of the outputs only" % (mutant, 100.0 * share)
