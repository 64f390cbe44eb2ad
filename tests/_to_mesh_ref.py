"""float64 numpy restatement of the Grid -> Mesh bilinear Store rule (include/mpassit_amd.h, mpg_regrid_store_to_mesh).

Not a copy of the kernel: no pyramid, no index boxes, no per-quad AABB.  Source cells are the quads of four neighbouring stagger
points A = (b, a), B = (b, a+1), C = (b+1, a+1), D = (b+1, a); a point belongs to the quad with the LOWEST id b * (snx - 1) + a for
which the Newton solve of X(xi, eta) = t * P (the iteration of the oracle's quad_solve: start (0.5, 0.5, 1), Cramer steps, stop after
a step below 1e-9, at most 50) ends with t > 0 and xi, eta in [-tol, 1 + tol].

Candidates: every quad of the grid (small grids) or, given an estimate of each point's stagger index, the quads within `reach` of
it (large grids).  Either list is thinned by one geometric fact only: a point that passes lies in the hull of the quad's corners
pushed out to the sphere, hence within the quad's circumscribing radius of its centroid -- quads more than twice that radius (plus
1e-6) away are not solved.
"""
import numpy as np


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def quad_solve(P, A, B, C, D):
    """Vectorised over rows of [n][3] arrays -> (xi, eta, ok)."""
    n = P.shape[0]
    s, t, lam = np.full(n, 0.5), np.full(n, 0.5), np.ones(n)
    ok = np.ones(n, bool)
    act = np.arange(n)
    e1, e2, e3 = B - A, D - A, (A - B) + (C - D)
    for _ in range(50):
        if act.size == 0:
            break
        a, p = A[act], P[act]
        f1, f2, f3 = e1[act], e2[act], e3[act]
        sa, ta, la = s[act], t[act], lam[act]
        X = (a + f1 * sa[:, None]) + (f2 * ta[:, None] + f3 * (sa * ta)[:, None])
        F = X - p * la[:, None]
        Js, Jt, Jl = f1 + f3 * ta[:, None], f2 + f3 * sa[:, None], -p
        det = _dot(Js, _cross(Jt, Jl))
        bad = det == 0.0
        det = np.where(bad, 1.0, det)
        mF = -F
        ds, dt, dl = _dot(mF, _cross(Jt, Jl)) / det, _dot(Js, _cross(mF, Jl)) / det, _dot(Js, _cross(Jt, mF)) / det
        ds, dt, dl = np.where(bad, 0.0, ds), np.where(bad, 0.0, dt), np.where(bad, 0.0, dl)
        s[act], t[act], lam[act] = sa + ds, ta + dt, la + dl
        ok[act[bad]] = False
        done = bad | ((np.abs(ds) < 1e-9) & (np.abs(dt) < 1e-9))
        act = act[~done]
    return s, t, ok & (lam > 0.0)


def to_mesh_bilinear(src_xyz, pts, tol=1e-10, cand=None, reach=2, chunk=4096):
    """src_xyz [sny][snx][3] unit vectors of the stagger points, pts [n][3] -> (idx [n][4] int32, -1 = unmapped; w [n][4];
    edge [n] = min(xi, 1 - xi, eta, 1 - eta) of the chosen quad, NaN where unmapped).
    cand: None = every quad of the grid; else (i, j) float arrays [n]: an estimate of each point's position in the stagger's own
    0-based index space -- the quads with a in floor(i) - reach .. + reach, b likewise, are the candidates."""
    src_xyz, pts = np.asarray(src_xyz, np.float64), np.asarray(pts, np.float64)
    sny, snx, _ = src_xyz.shape
    qnx, qny = snx - 1, sny - 1
    A, B = src_xyz[:-1, :-1].reshape(-1, 3), src_xyz[:-1, 1:].reshape(-1, 3)
    C, D = src_xyz[1:, 1:].reshape(-1, 3), src_xyz[1:, :-1].reshape(-1, 3)
    ctr = 0.25 * (A + B + C + D)
    rad = np.max([np.linalg.norm(X - ctr, axis=1) for X in (A, B, C, D)], axis=0)
    n = pts.shape[0]
    pi_l, qi_l = [], []
    if cand is None:
        chunk = max(1, min(chunk, 20_000_000 // max(ctr.shape[0], 1)))
        c2 = (ctr * ctr).sum(axis=1)
        for p0 in range(0, n, chunk):
            pc = pts[p0:p0 + chunk]
            d2 = np.maximum((pc * pc).sum(axis=1)[:, None] + c2[None, :] - 2.0 * (pc @ ctr.T), 0.0)
            pp, qq = np.nonzero(np.sqrt(d2) <= 2.0 * rad[None, :] + 1e-6)
            pi_l.append(pp + p0)
            qi_l.append(qq)
    else:
        ci, cj = np.floor(np.asarray(cand[0], np.float64)), np.floor(np.asarray(cand[1], np.float64))
        okc = np.isfinite(ci) & np.isfinite(cj)
        ci, cj = np.where(okc, ci, -10**6).astype(np.int64), np.where(okc, cj, -10**6).astype(np.int64)
        allp = np.arange(n)
        for db in range(-reach, reach + 1):
            for da in range(-reach, reach + 1):
                a, b = ci + da, cj + db
                keep = (a >= 0) & (a < qnx) & (b >= 0) & (b < qny)
                pp, qq = allp[keep], (b * qnx + a)[keep]
                near = np.linalg.norm(pts[pp] - ctr[qq], axis=1) <= 2.0 * rad[qq] + 1e-6
                pi_l.append(pp[near])
                qi_l.append(qq[near])
    pi, qi = np.concatenate(pi_l), np.concatenate(qi_l)
    xi, eta, ok = quad_solve(pts[pi], A[qi], B[qi], C[qi], D[qi])
    ok &= (xi >= -tol) & (xi <= 1.0 + tol) & (eta >= -tol) & (eta <= 1.0 + tol)
    best = np.full(n, np.iinfo(np.int64).max)
    np.minimum.at(best, pi[ok], qi[ok])
    sel = ok & (qi == best[pi])
    idx, w, edge = np.full((n, 4), -1, np.int32), np.zeros((n, 4)), np.full(n, np.nan)
    p, q, x, e = pi[sel], qi[sel], xi[sel], eta[sel]
    b, a = q // qnx, q % qnx
    iA = b * snx + a
    idx[p] = np.stack([iA, iA + 1, iA + 1 + snx, iA + snx], axis=1).astype(np.int32)
    w[p] = np.stack([(1 - x) * (1 - e), x * (1 - e), x * e, (1 - x) * e], axis=1)
    edge[p] = np.minimum(np.minimum(x, 1 - x), np.minimum(e, 1 - e))
    return idx, w, edge


def edge_share(edge, eps=1e-9):
    """Share of the mapped points that sit within eps (parametric units) of an edge of their quad: the points on which two correct
    implementations may pick different quads."""
    m = np.isfinite(edge)
    return float((edge[m] < eps).sum()) / max(int(m.sum()), 1)
