"""Reference for the adjoint of the masked Regrid (mpg_regrid_masked_transpose_dev), restated from the header's text on a handle's own
exported pattern (_contract_ref.Pattern); nothing here touches a GPU.

    valid(q), Wt, Wv, defined   sequential float64 in stored order with numpy, the loop of _masked_ref.masked_ref (which keeps Wt and Wv
                                to itself; test_masked_transpose_cpu.py holds `defined` here to masked_ref's)
    h[k][p]    = defined ? ((double)g * scale) * (Wt / Wv) : +0.0     numpy's correctly rounded * and /, np.where
    acc        = _contract_ref.transpose(pattern, h): the exact C restatement of acc = fma(w_j, h[row_j], acc), with the cast to dst's type
    dst[c][k]  = src_mask[c] == 0 and src(c, k) not missing ? acc : +0.0

`variant` selects a deliberately wrong recipe (MUTANTS); None is the contract.  Results are compared on integer views
(_contract_ref.bits / differs / same): nothing excluded, no tolerance."""
import numpy as np

import _contract_ref as cr

EPS = np.finfo(np.float64).eps
# wrong recipes a test's inputs must tell from the contract:
#   "no select"     the chain's value is stored at invalid sources too
#   "no ratio"      h = g * scale at defined points: the renormalisation Wt / Wv left out
#   "ratio after"   the ratio enters after the gradient has entered the chain's product instead of before: folded into the weight,
#                   acc = fma(w_j * (Wt / Wv), g * scale, acc), in place of h -- the same real number, other roundings
#   "times zero"    h = (g * scale) * (Wt / Wv) * (defined ? 1 : 0) in place of the select: a NaN of g at an undefined point spreads
MUTANTS = ("no select", "no ratio", "ratio after", "times zero")


def _missing(x, nan, missing_value):
    miss = np.zeros(x.shape, bool)
    if nan:
        miss |= np.isnan(x)
    if missing_value is not None:
        miss |= x == missing_value
    return miss


def weight_sums(pat, src, nan=True, missing_value=None, src_mask=None, min_valid_frac=0.5):
    """src [nlev][n_src] float64 -> (Wt [n_dst], Wv [nlev][n_dst], defined [nlev][n_dst]), the forward's decision bit for bit."""
    src = np.asarray(src, np.float64).reshape(-1, pat.n_src)
    nlev, P = src.shape[0], pat.n_dst
    mask = np.zeros(pat.n_src, bool) if src_mask is None else np.asarray(src_mask).astype(bool)
    Wt, Wv = np.zeros(P), np.zeros((nlev, P))
    if pat.nnz == 0:
        lens = np.diff(pat.rowptr)
        for t in range(int(lens.max()) if P else 0):           # entry t of every row that has one: sequential per row, stored order
            rows = np.flatnonzero(lens > t)
            e = pat.rowptr[rows] + t
            c, wq = pat.col[e].astype(np.int64), pat.val[e]
            ok = ((c >= 0) & ~mask[np.maximum(c, 0)])[None, :] & ~_missing(src[:, np.maximum(c, 0)], nan, missing_value)
            Wt[rows] = Wt[rows] + wq
            Wv[:, rows] = Wv[:, rows] + np.where(ok, wq[None, :], 0.0)
    else:
        w = np.ones_like(pat.w) if pat.nnz == 1 else pat.w      # nearest neighbour: weight 1
        for q in range(pat.nnz):                                # the slots, left to right
            c, wq = pat.idx[:, q].astype(np.int64), w[:, q]
            ok = ((c >= 0) & ~mask[np.maximum(c, 0)])[None, :] & ~_missing(src[:, np.maximum(c, 0)], nan, missing_value)
            wk = np.where(ok, wq[None, :], 0.0)
            Wt = wq.copy() if q == 0 else Wt + wq
            Wv = wk.copy() if q == 0 else Wv + wk
    defined = (Wv > 0.0) & (Wv >= (min_valid_frac * Wt)[None, :])
    return Wt, Wv, defined


def source_ok(pat, src, nan=True, missing_value=None, src_mask=None):
    """[nlev][n_src] bool: the source element entered the forward wherever an entry references it"""
    src = np.asarray(src, np.float64).reshape(-1, pat.n_src)
    mask = np.zeros(pat.n_src, bool) if src_mask is None else np.asarray(src_mask).astype(bool)
    return ~mask[None, :] & ~_missing(src, nan, missing_value)


def masked_transpose_ref(pat, g, src, nlev=1, nfields=1, nan=True, missing_value=None, src_mask=None, min_valid_frac=0.5, scale=1.0,
                         dst_dtype=np.float64, dst_lev_fast=False, g_level_stride=0, variant=None):
    """g: float32 / float64, nfields * nlev planes of n_dst, g_level_stride elements apart (0: dense); src: (nfields, nlev, n_src), the
    VALUES the forward read (a float32 field: widened; a level-fast field: put back to [lev][cell] by the caller).
    -> (dst (nfields, nlev, n_src) or, dst_lev_fast, (nfields, n_src, nlev) of dst_dtype; h (nfields, nlev, n_dst) float64;
        defined (nfields, nlev, n_dst) bool)."""
    assert variant is None or variant in MUTANTS
    P, ld = pat.n_dst, g_level_stride or pat.n_dst
    g = np.ascontiguousarray(g).reshape(-1)
    gd = np.stack([g[i * ld:i * ld + P] for i in range(nfields * nlev)]).astype(np.float64).reshape(nfields, nlev, P)
    src = np.asarray(src, np.float64).reshape(nfields, nlev, pat.n_src)
    h = np.empty((nfields, nlev, P))
    defined = np.empty((nfields, nlev, P), bool)
    ratio = np.empty((nfields, nlev, P))
    with np.errstate(all="ignore"):
        for f in range(nfields):
            Wt, Wv, defined[f] = weight_sums(pat, src[f], nan, missing_value, src_mask, min_valid_frac)
            ratio[f] = Wt[None, :] / Wv
            gs = gd[f] * scale
            if variant == "no ratio" or variant == "ratio after":
                h[f] = np.where(defined[f], gs, 0.0)
            elif variant == "times zero":
                h[f] = (gs * ratio[f]) * defined[f].astype(np.float64)
            else:
                h[f] = np.where(defined[f], gs * ratio[f], 0.0)
    if variant == "ratio after":
        assert pat.nnz == 0, "the folded-weight mutant is written for CSR patterns"
        rowof = np.repeat(np.arange(P), np.diff(pat.rowptr))
        acc = np.empty((nfields, nlev, pat.n_src), dst_dtype)
        for f in range(nfields):
            for k in range(nlev):
                with np.errstate(all="ignore"):
                    val = pat.val * np.where(defined[f, k], ratio[f, k], 0.0)[rowof]
                pk = cr.Pattern(pat.n_src, P, 0, rowptr=pat.rowptr, col=pat.col, val=val)
                acc[f, k] = cr.transpose(pk, h[f, k], 1, 1, dst_dtype)[0][0, 0]
        if dst_lev_fast:
            acc = np.ascontiguousarray(acc.transpose(0, 2, 1))
    else:
        acc, _ = cr.transpose(pat, h, nlev, nfields, dst_dtype, dst_lev_fast)
    ok = np.stack([source_ok(pat, src[f], nan, missing_value, src_mask) for f in range(nfields)])
    if dst_lev_fast:
        ok = ok.transpose(0, 2, 1)
    dst = acc if variant == "no select" else np.where(ok, acc, acc.dtype.type(0.0))
    return np.ascontiguousarray(dst), h, defined


CASE_NLEV = 2


def gappy_case(nlev=CASE_NLEV, seed=5, frac=0.5):
    """The inputs the CPU tests and the dense-Jacobian GPU test share: the synthetic transpose pattern (41 sources, 401 points), one field
    with NaN on 30 % of its elements, a static mask on three sources, and a finite gradient with a NaN planted at every undefined and
    unmapped output.  -> (pattern, src [nlev][n_src], mask uint8 [n_src], g [nlev][n_dst], defined [nlev][n_dst])."""
    _, pat = cr.synthetic_transpose_case()
    rng = np.random.default_rng(seed)
    src = cr.ordinary(pat.n_src, nlev, 1, seed)[0]
    src[rng.uniform(size=src.shape) < 0.3] = np.nan
    mask = np.zeros(pat.n_src, np.uint8)
    mask[rng.permutation(pat.n_src)[:3]] = 1
    g = rng.normal(0.0, 3.0, (nlev, pat.n_dst))
    _, _, defined = weight_sums(pat, src, src_mask=mask, min_valid_frac=frac)
    g[~defined] = np.nan
    return pat, src, mask, g, defined


def jacobian_product(pat, g, src, nlev, nan=True, missing_value=None, src_mask=None, min_valid_frac=0.5, scale=1.0):
    """The adjoint by construction, one field: the dense Jacobian of _contract_ref.apply_masked column by column -- one valid element 1,
    the other valid ones 0, missing ones left missing -- and J^T g in np.longdouble.  g [nlev][n_dst] float64 (entries where J is zero
    are not read: a NaN there is as good as any number), src [nlev][n_src] float64.
    -> (want [nlev][n_src] longdouble, bound [nlev][n_src]): |dst - want| <= bound = 8 eps sum_j (Wt / Wv)_j |w_j g_j scale|, times n / 8 for
    a segment of n > 8 entries -- the form of _masked_ref.py and of the transpose's bound."""
    src = np.asarray(src, np.float64).reshape(nlev, pat.n_src)
    g = np.asarray(g, np.float64).reshape(nlev, pat.n_dst)
    flags = (1 if nan else 0) | (2 if missing_value is not None else 0)
    ok = source_ok(pat, src, nan, missing_value, src_mask)
    base = np.where(ok, 0.0, src)                       # statically masked elements keep their value: the mask hides them
    want = np.zeros((nlev, pat.n_src), np.longdouble)
    bound = np.zeros((nlev, pat.n_src))
    for k in range(nlev):
        for c in np.flatnonzero(ok[k]):
            x = base.copy()
            x[k, c] = 1.0
            col = cr.apply_masked(pat, x, nlev, 1, flags=flags, missing_value=missing_value or 0.0, src_mask=src_mask,
                                  min_valid_frac=min_valid_frac, fill_value=0.0, scale=scale)[0]
            assert not col[np.arange(nlev) != k].any(), "levels are independent"
            nz = np.flatnonzero(col[k])
            want[k, c] = (col[k, nz].astype(np.longdouble) * g[k, nz].astype(np.longdouble)).sum()
    # the bound from the pattern itself
    Wt, Wv, defined = weight_sums(pat, src, nan, missing_value, src_mask, min_valid_frac)
    pt = cr.transposed(pat)
    seg = np.repeat(np.arange(pat.n_src), np.diff(pt.rowptr))
    n = np.maximum(np.diff(pt.rowptr), 8) / 8.0
    with np.errstate(all="ignore"):
        for k in range(nlev):
            term = np.where(defined[k], (Wt / Wv[k]) * np.abs(g[k] * scale), 0.0)[pt.col] * np.abs(pt.val)
            bound[k] = 8 * EPS * n * np.bincount(seg, weights=term, minlength=pat.n_src)
    return want, bound, ok
