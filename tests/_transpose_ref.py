"""Reference for the transpose Regrid: A^T g from the handle's own ESMF weight list (RouteHandle.to_esmf_weights, pole terms
included), in numpy, with the per-output error bound |delta| <= 8 eps sum_j |w_j g_j|."""
import numpy as np

EPS = np.finfo(np.float64).eps


def transpose_ref(rh, g):
    """g: [nlev][n_dst] float64 (numpy).  -> (A^T g [nlev][n_src], bound [nlev][n_src]).
    The reference sums every source's products in extended precision (np.longdouble), so it is all but exact.  The bound is what the
    library's float64 arithmetic may lose, scaled so that callers check |delta| <= 8 eps bound: sum_j |w_j g_j| for a source with at
    most 8 stored entries; n_c / 8 times that for a longer sequential sum of n_c entries; plus, on the two CENTER rows of a pole cap,
    (ceil(n_q / 256) + 10) / 8 times the cap's sum_q |w_pole g| / row_len (the cap's fixed-order reduction of n_q terms: per-thread
    partial sums, an 8-level tree, the division and the final add)."""
    row, col, S = rh.to_esmf_weights()
    r, c = row.astype(np.int64) - 1, col.astype(np.int64) - 1
    g = np.asarray(g, np.float64).reshape(-1, rh.n_dst)
    order = np.argsort(c, kind="stable")
    cs, rs, Ss = c[order], r[order], S[order].astype(np.longdouble)
    starts = np.flatnonzero(np.r_[True, cs[1:] != cs[:-1]]) if cs.size else np.zeros(0, np.int64)
    if rh.nnz_per_row == 0:
        stored = rh.csr()[1]
    else:
        idx = rh.weights()[0]
        stored = idx[idx >= 0]
    n_c = np.bincount(stored.astype(np.int64), minlength=rh.n_src)[:rh.n_src]
    scale = np.maximum(n_c, 8) / 8.0
    dst, src0, wp, row_len = rh.pole()
    out = np.zeros((g.shape[0], rh.n_src))
    bound = np.empty_like(out)
    for k in range(g.shape[0]):
        if cs.size:
            out[k, cs[starts]] = np.add.reduceat(Ss * g[k, rs], starts).astype(np.float64)
        bound[k] = scale * np.bincount(c, weights=np.abs(S * g[k, r]), minlength=rh.n_src)
        for first in np.unique(src0):
            q = (src0 == first) & (wp != 0.0)
            if q.any():
                cap = np.abs(wp[q] * g[k, dst[q]]).sum() / row_len
                bound[k, first:first + row_len] += (-(-int(q.sum()) // 256) + 10) / 8.0 * cap
    return out, bound


def assert_f64_close(got, want, bound, what):
    got = np.asarray(got, np.float64).reshape(want.shape)
    err = np.abs(got - want)
    bad = ~(err <= 8 * EPS * bound)
    assert not bad.any(), "%s: %d outputs outside 8 eps sum|w g|, first at %s: got %r want %r (bound %r)" % (
        what, int(bad.sum()), np.argwhere(bad)[0], got[bad][0], want[bad][0], bound[bad][0])


def assert_f32_close(got, want, bound, what):
    """float32 results within 1 ulp of the rounded float64 reference, widened by the reference's own float64 bound (which only
    matters under cancellation)."""
    got = np.asarray(got, np.float32).reshape(want.shape).astype(np.float64)
    w32 = want.astype(np.float32)
    ulp = np.spacing(np.abs(w32)).astype(np.float64)
    err = np.abs(got - w32.astype(np.float64))
    bad = ~(err <= ulp + 8 * EPS * bound)
    assert not bad.any(), "%s: %d float32 outputs beyond 1 ulp, first at %s: got %r want %r" % (
        what, int(bad.sum()), np.argwhere(bad)[0], got[bad][0], w32[bad][0])
