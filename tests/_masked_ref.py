"""Reference for the masked Regrid (mpg_regrid_masked_dev), in numpy, from the handle's own exported weights (RouteHandle.weights /
RouteHandle.csr).  The validity decision and the two weight sums Wt, Wv are computed exactly as the contract specifies them --
float64, sequentially, in stored order -- so that defined / undefined can be compared exactly; the weighted value N is summed in
np.longdouble and comes with the per-output bound 8 eps (Wt / Wv) sum |w s| over the valid entries (times n / 8 for a CSR row of
n > 8 entries, as the transpose reference scales its bound)."""
import numpy as np

EPS = np.finfo(np.float64).eps


class MaskedRef:
    """defined [nlev][n_dst] bool; value [nlev][n_dst] float64 = N * Wt / Wv (meaningless where undefined); bound [nlev][n_dst] (callers
    check |delta| <= 8 eps bound); edge [nlev][n_dst] bool: Wv > 0 and |Wv - frac * Wt| <= 1e-12 * Wt, the outputs that may fall either way;
    stored [n_dst] bool: the point has at least one stored entry with idx >= 0."""

    def __init__(self, defined, value, bound, edge, stored):
        self.defined, self.value, self.bound, self.edge, self.stored = defined, value, bound, edge, stored


def _missing(x, nan, missing_value):
    miss = np.zeros(x.shape, bool)
    if nan:
        miss |= np.isnan(x)
    if missing_value is not None:
        miss |= x == missing_value
    return miss


def masked_ref(rh, src, nan=True, missing_value=None, src_mask=None, min_valid_frac=0.5):
    """src: [nlev][n_src] float64 (a float32 field: its values widened).  -> MaskedRef."""
    src = np.asarray(src, np.float64).reshape(-1, rh.n_src)
    nlev, P = src.shape[0], rh.n_dst
    mask = np.zeros(rh.n_src, bool) if src_mask is None else np.asarray(src_mask).astype(bool)
    Wt = np.zeros(P)
    Wv = np.zeros((nlev, P))
    N = np.zeros((nlev, P), np.longdouble)
    ab = np.zeros((nlev, P))
    nent = np.zeros(P, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        if rh.nnz_per_row == 0:
            rowptr, col, val = rh.csr()
            lens = np.diff(rowptr)
            for t in range(int(lens.max()) if P else 0):       # entry t of every row that has one: sequential per row, stored order
                rows = np.flatnonzero(lens > t)
                e = rowptr[rows] + t
                c, wq = col[e].astype(np.int64), val[e]
                x = src[:, np.maximum(c, 0)]
                ok = ((c >= 0) & ~mask[np.maximum(c, 0)])[None, :] & ~_missing(x, nan, missing_value)
                wk, xk = np.where(ok, wq[None, :], 0.0), np.where(ok, x, 0.0)
                Wt[rows] = Wt[rows] + wq
                Wv[:, rows] = Wv[:, rows] + wk
                N[:, rows] += wk.astype(np.longdouble) * xk.astype(np.longdouble)
                ab[:, rows] += np.abs(wk * xk)
                nent[rows] += c >= 0
            scale = np.maximum(lens, 8) / 8.0
        else:
            idx, w = rh.weights()
            if rh.nnz_per_row == 1:
                w = np.ones_like(w)                              # nearest neighbour: weight 1
            for q in range(rh.nnz_per_row):                      # explicit loop over the slots, left to right
                c, wq = idx[:, q].astype(np.int64), w[:, q]
                x = src[:, np.maximum(c, 0)]
                ok = ((c >= 0) & ~mask[np.maximum(c, 0)])[None, :] & ~_missing(x, nan, missing_value)
                wk, xk = np.where(ok, wq[None, :], 0.0), np.where(ok, x, 0.0)
                Wt = wq.copy() if q == 0 else Wt + wq
                Wv = wk.copy() if q == 0 else Wv + wk
                N += wk.astype(np.longdouble) * xk.astype(np.longdouble)
                ab += np.abs(wk * xk)
                nent += c >= 0
            scale = np.ones(P)
        thr = min_valid_frac * Wt
        defined = (nent > 0)[None, :] & (Wv > 0.0) & (Wv >= thr[None, :])
        # (Wv == 0 is undefined by the Wv > 0 rule, whatever the threshold: no rounding decides it, so it is never an edge output)
        edge = (Wv > 0.0) & (np.abs(Wv - thr[None, :]) <= 1e-12 * np.abs(Wt)[None, :])
        ratio = np.where(defined, Wt[None, :].astype(np.longdouble) / np.where(defined, Wv, 1.0).astype(np.longdouble), 1.0)
        value = (N * ratio).astype(np.float64)
        bound = scale[None, :] * ratio.astype(np.float64) * ab
    return MaskedRef(defined, value, bound, edge, nent > 0)


def check_masked(got, ref, fill, what, scale=1.0, offset=0.0):
    """got: [nlev][n_dst] float32 / float64 from the library; fill must not be a value a defined point can take (NaN is fine).
    Defined and undefined must agree exactly outside ref.edge; defined values within the bound (float32: 1 ulp of the rounded reference
    more); undefined values exactly fill in got's type.  -> number of edge outputs."""
    got = np.asarray(got)
    f32 = got.dtype == np.float32
    got = got.reshape(ref.value.shape)
    fill_t = got.dtype.type(fill)
    is_fill = np.isnan(got) if np.isnan(fill_t) else got == fill_t
    sure = ~ref.edge
    wrong = sure & (is_fill == ref.defined)
    assert not wrong.any(), "%s: %d outputs defined / undefined against the reference, first at %s (reference defined: %s)" % (
        what, int(wrong.sum()), np.argwhere(wrong)[0], bool(ref.defined[tuple(np.argwhere(wrong)[0])]))
    d = ~is_fill & ref.defined
    want = ref.value * scale + offset
    bound = 8 * EPS * ref.bound * abs(scale)
    if (scale, offset) != (1.0, 0.0):
        bound = bound + EPS * np.abs(want)            # the epilogue's own rounding
    g = got.astype(np.float64)
    if f32:
        w32 = want.astype(np.float32)
        err = np.abs(g - w32.astype(np.float64))
        tol = np.spacing(np.abs(w32)).astype(np.float64) + bound
    else:
        err = np.abs(g - want)
        tol = bound
    bad = d & ~(err <= tol)
    assert not bad.any(), "%s: %d defined outputs outside the bound, first at %s: got %r want %r (tol %r)" % (
        what, int(bad.sum()), np.argwhere(bad)[0], g[bad][0], want[bad][0], tol[bad][0])
    return int(ref.edge.sum())
