"""float64 numpy restatement of the periodic Grid -> Mesh bilinear Store rule (include/mpassit_amd.h, mpg_regrid_store_periodic_to_mesh).

Not a copy of the kernel: no pyramid, no index boxes, no candidate list, no sorting network.
  quads  _to_mesh_ref.to_mesh_bilinear on the CENTER points padded with column 0 as column nx: its quad (b, a) of the padded grid IS
         quad (b, a) of the periodic one (id b * nx + a, lowest id first), and its columns map back by a + 1 -> (a + 1) mod nx.
  caps   the oracle's bilinear_weights (planar barycentric weights seen from the sphere's centre, the lowest passing triangle id) on the
         points of the two end rows plus one pole point per end, (0, 0, sign of that end row's mean z): (A, B, N) at the north pole,
         (B, A, S) at the south pole; triangle ids 0 .. nx - 1 on row 0, nx .. 2 nx - 1 on row ny - 1, whichever way the rows are numbered.
         Only points no quad took are asked.
  rows   quad rows: 4 entries, zeros included; cap rows: nx entries, wr = t_pole / nx everywhere, t_A + wr and t_B + wr on A and B;
         columns ascending.
`mutate` builds deliberately wrong variants for the reference's own tests: "seam_swap_bc" (B and C exchanged in the seam quads),
"cap_no_division" (wr = t_pole), "caps_first" (a cap is tried before the quads), "caps_by_row_index" (row 0 always takes the pole (0, 0, -1)
and row ny - 1 (0, 0, 1): Arctic points of a grid numbered north to south then get rows of the Antarctic end row).
"""
import numpy as np

import _to_mesh_ref as ref

NO_SOUTH, NO_NORTH = 2, 4   # MPG_GRID_NO_SOUTH_POLE, MPG_GRID_NO_NORTH_POLE
POLE_NONE, POLE_ALLAVG = 0, 1
KIND_NONE, KIND_QUAD, KIND_CAP = 0, 1, 2


def _caps(oracle, cen, pts, flags, by_row_index=False):
    """-> (cap id [n], -1 = none; t_A, t_B, t_pole [n]; smallest barycentric coordinate [n]).
    The pole of an end is (0, 0, sign of that end row's mean z); by_row_index: the rule before that one, (0, 0, -1) for row 0 and
    (0, 0, 1) for row ny - 1 whatever the rows' latitudes."""
    ny, nx, _ = cen.shape
    pole = [-1.0, 1.0] if by_row_index else [-1.0 if cen[j, :, 2].mean() < 0.0 else 1.0 for j in (0, ny - 1)]
    if not by_row_index and not flags & (NO_SOUTH | NO_NORTH) and pole[0] == pole[1]:
        raise ValueError("both end rows lie in one hemisphere: at most one closes on a pole (MPG_GRID_NO_SOUTH_POLE / MPG_GRID_NO_NORTH_POLE)")
    cells = np.concatenate([cen[0], cen[ny - 1], [[0.0, 0.0, pole[0]]], [[0.0, 0.0, pole[1]]]])
    a = np.arange(nx)
    a1 = (a + 1) % nx
    # counter-clockwise seen from outside: (A, B, N) at the north pole, (B, A, S) at the south pole
    ends = [np.stack([e * nx + a, e * nx + a1, np.full(nx, 2 * nx + e)], axis=1) if pole[e] > 0 else
            np.stack([e * nx + a1, e * nx + a, np.full(nx, 2 * nx + e)], axis=1) for e in (0, 1)]
    if flags & NO_SOUTH:
        ends[0][:] = -1
    if flags & NO_NORTH:
        ends[1][:] = -1
    idx, w = oracle.bilinear_weights(cells, np.concatenate(ends).astype(np.int32), pts)
    n = pts.shape[0]
    cap, tA, tB, tP = np.full(n, -1, np.int64), np.zeros(n), np.zeros(n), np.zeros(n)
    hit = idx[:, 0] >= 0
    for e in (0, 1):
        at = hit & (idx[:, 2] == 2 * nx + e)
        ia, ib = (0, 1) if pole[e] > 0 else (1, 0)
        cap[at] = idx[at, ia]            # e * nx + a already
        tA[at], tB[at] = w[at, ia], w[at, ib]
    tP[hit] = w[hit, 2]
    return cap, tA, tB, tP, np.where(hit, w.min(axis=1), np.nan)


def periodic_to_mesh(oracle, cen_xyz, pts, pole_method=POLE_ALLAVG, flags=0, tol=1e-10, mutate=None):
    """oracle: the built oracle module (the `oracle` fixture); cen_xyz [ny][nx][3] unit vectors of the CENTER points, pts [n][3] -> dict(rowptr, col, val, kind [n], quad [n] (quad id or -1),
    cap [n] (cap id or -1), edge [n]: min(xi, 1 - xi, eta, 1 - eta) of a quad row, the smallest barycentric coordinate of a cap row,
    NaN where unmapped)."""
    cen, pts = np.asarray(cen_xyz, np.float64), np.asarray(pts, np.float64)
    ny, nx, _ = cen.shape
    n = pts.shape[0]
    idx, w, edge = ref.to_mesh_bilinear(np.concatenate([cen, cen[:, :1]], axis=1), pts, tol=tol)
    inq = idx[:, 0] >= 0
    b, a = idx[:, 0] // (nx + 1), idx[:, 0] % (nx + 1)
    a1 = (a + 1) % nx
    qcol = np.stack([b * nx + a, b * nx + a1, (b + 1) * nx + a1, (b + 1) * nx + a], axis=1)
    quad = np.where(inq, b * nx + a, -1)
    if mutate == "seam_swap_bc":
        seam = inq & (a == nx - 1)
        w = w.copy()
        w[seam, 1], w[seam, 2] = w[seam, 2].copy(), w[seam, 1].copy()
    kind = np.where(inq, KIND_QUAD, KIND_NONE)
    cap = np.full(n, -1, np.int64)
    tA = tB = tP = np.zeros(n)
    if pole_method == POLE_ALLAVG:
        ask = np.arange(n) if mutate == "caps_first" else np.nonzero(~inq)[0]
        if ask.size:
            c, ta, tb, tp, bary = _caps(oracle, cen, pts[ask], flags, by_row_index=mutate == "caps_by_row_index")
            hit = c >= 0
            cap[ask[hit]] = c[hit]
            tA, tB, tP = np.zeros(n), np.zeros(n), np.zeros(n)
            tA[ask], tB[ask], tP[ask] = ta, tb, tp
            kind[ask[hit]] = KIND_CAP
            quad[ask[hit]] = -1
            edge = edge.copy()
            edge[ask[hit]] = bary[hit]
    length = np.where(kind == KIND_QUAD, 4, np.where(kind == KIND_CAP, nx, 0))
    rowptr = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    col, val = np.empty(rowptr[-1], np.int32), np.empty(rowptr[-1])
    q = np.nonzero(kind == KIND_QUAD)[0]
    if q.size:
        order = np.argsort(qcol[q], axis=1, kind="stable")
        at = rowptr[q][:, None] + np.arange(4)[None, :]
        col[at] = np.take_along_axis(qcol[q], order, axis=1)
        val[at] = np.take_along_axis(w[q], order, axis=1)
    for p in np.nonzero(kind == KIND_CAP)[0]:
        north = cap[p] >= nx
        ca = cap[p] - nx if north else cap[p]
        row0 = (ny - 1) * nx if north else 0
        wr = tP[p] if mutate == "cap_no_division" else tP[p] / float(nx)
        v = np.full(nx, wr)
        v[ca] = tA[p] + wr
        v[(ca + 1) % nx] = tB[p] + wr
        col[rowptr[p]:rowptr[p + 1]] = row0 + np.arange(nx)
        val[rowptr[p]:rowptr[p + 1]] = v
    return dict(rowptr=rowptr, col=col, val=val, kind=kind, quad=quad, cap=cap, edge=edge, nx=nx, ny=ny)


def edge_share(r, eps=1e-9):
    """Share of the mapped points within eps (parametric or barycentric) of an edge of their quad / cap triangle."""
    m = r["kind"] != KIND_NONE
    return float((r["edge"][m] < eps).sum()) / max(int(m.sum()), 1)


def seam_rows(r):
    return np.nonzero((r["kind"] == KIND_QUAD) & (r["quad"] % r["nx"] == r["nx"] - 1))[0]
