"""float64 numpy reference of the conservative Grid -> Mesh Store (include/mpassit_amd.h, mpg_regrid_store_conserve_to_mesh).

With A[g][c] = I(c, g) / area(g) any Mesh -> Grid conservative matrix, the matrix wanted is B[c][g] = I(c, g) / area(c) =
A[g][c] * area(g) / area(c) (MPG_NORM_DSTAREA) or I / sum_g I (MPG_NORM_FRACAREA), the dst fraction sum_g I / area(c).  Areas are
spherical polygon areas as a fan of Van Oosterom-Strackee triangles."""
import numpy as np

NORM_DSTAREA, NORM_FRACAREA = 0, 1
SLIVER_RULE = 1e-14          # an entry is dropped when I <= 1e-14 * area(c)
SLIVER = 1e-12               # weights below this may legitimately exist on one side only (tests/_parity_helpers.py)
SLIVER_CAP = 1e-4            # at most 1 entry in 10 000 of a reference may be that small


def tri_area(a, b, c):
    """Signed area of the spherical triangles a, b, c ([..., 3] unit vectors): tan(E / 2) = a . (b x c) / (1 + a.b + b.c + c.a).  The
    triple product in difference form, a . ((b - a) x (c - a)): the direct form cancels to ~1e-16 absolute, 1e-9 of a 3-km cell."""
    num = np.einsum("...i,...i->...", a, np.cross(b - a, c - a))
    den = 1.0 + np.einsum("...i,...i->...", a, b) + np.einsum("...i,...i->...", b, c) + np.einsum("...i,...i->...", c, a)
    return 2.0 * np.arctan2(num, den)


def poly_area(v):
    """|area| of one spherical polygon, vertices [n][3] in order: the fan from its first vertex."""
    v = np.asarray(v, np.float64)
    return abs(sum(tri_area(v[0], v[i], v[i + 1]) for i in range(1, v.shape[0] - 1)))


def grid_cell_areas(corner_xyz, nx, ny):
    """[ny * nx] areas of the grid's cells: the four CORNER points around centre (i, j), index j * nx + i."""
    c = np.asarray(corner_xyz, np.float64).reshape(ny + 1, nx + 1, 3)
    q0, q1, q2, q3 = c[:-1, :-1], c[:-1, 1:], c[1:, 1:], c[1:, :-1]
    return np.abs(tri_area(q0, q1, q2) + tri_area(q0, q2, q3)).reshape(-1)


def mesh_cell_areas(voc, vert_xyz):
    """[nCells] areas of the Voronoi cells from verticesOnCell ([nCells][maxEdges], 1-based, 0-padded)."""
    voc = np.asarray(voc)
    n_cells = voc.shape[0]
    first, prev = np.zeros((n_cells, 3)), np.zeros((n_cells, 3))
    cnt, area = np.zeros(n_cells, np.int64), np.zeros(n_cells)
    for j in range(voc.shape[1]):
        ok = voc[:, j] > 0
        x = vert_xyz[np.maximum(voc[:, j], 1) - 1]
        fan = ok & (cnt >= 2)
        area[fan] += tri_area(first[fan], prev[fan], x[fan])
        first[ok & (cnt == 0)] = x[ok & (cnt == 0)]
        prev[ok] = x[ok]
        cnt += ok
    return np.abs(area)


def tol_both(corner_xyz, nx, ny, voc, vert_xyz):
    """The project's conservative bar -- 64 eps / min(h), floored at 1e-11, h the thin dimension (area / longest diagonal) of a cell
    (tests/_parity_helpers.py conserve_tol) -- with h taken over BOTH cell sets: the mesh cell's area is the divisor here."""
    c = np.asarray(corner_xyz, np.float64).reshape(ny + 1, nx + 1, 3)
    d1, d2 = c[1:, 1:] - c[:-1, :-1], c[1:, :-1] - c[:-1, 1:]
    ga = grid_cell_areas(corner_xyz, nx, ny).reshape(ny, nx)
    diag = np.maximum(np.linalg.norm(d1, axis=-1), np.linalg.norm(d2, axis=-1))
    hg = (ga / np.maximum(diag, 1e-300))[ga > 0]
    voc = np.asarray(voc)
    ma = mesh_cell_areas(voc, vert_xyz)
    v = vert_xyz[np.maximum(voc, 1) - 1]                                   # [nCells][maxEdges][3]
    v = np.where((voc > 0)[..., None], v, v[:, :1])                        # pads repeat the first vertex
    diam = np.linalg.norm(v[:, :, None, :] - v[:, None, :, :], axis=-1).max(axis=(1, 2))
    hm = (ma / np.maximum(diam, 1e-300))[ma > 0]
    return max(1e-11, 64 * np.finfo(np.float64).eps / min(hg.min(), hm.min()))


def b_ref(entries_g, entries_c, entries_a, area_g, area_c, norm=NORM_DSTAREA):
    """B and frac from the entries (g, c, A[g][c]) of a Mesh -> Grid conservative matrix.  Returns rowptr [nCells + 1], col (grid
    index, ascending within a row), val, frac [nCells]."""
    g, c, a = np.asarray(entries_g, np.int64), np.asarray(entries_c, np.int64), np.asarray(entries_a, np.float64)
    n_cells = area_c.size
    inter = a * area_g[g]
    keep = inter > SLIVER_RULE * area_c[c]
    g, c, inter = g[keep], c[keep], inter[keep]
    order = np.lexsort((g, c))
    g, c, inter = g[order], c[order], inter[order]
    cover = np.bincount(c, weights=inter, minlength=n_cells)
    frac = np.where(area_c > 0, cover / np.maximum(area_c, 1e-300), 0.0)
    div = area_c[c] if norm == NORM_DSTAREA else cover[c]
    rowptr = np.zeros(n_cells + 1, np.int64)
    np.cumsum(np.bincount(c, minlength=n_cells), out=rowptr[1:])
    return rowptr, g.astype(np.int32), inter / div, frac


def b_ref_from_csr(rowptr, col, val, area_g, area_c, norm=NORM_DSTAREA):
    """... from A in CSR form (rows = grid cells), as oracle.conserve and RouteHandle.csr() give it."""
    rows = np.repeat(np.arange(rowptr.size - 1, dtype=np.int64), np.diff(rowptr))
    return b_ref(rows, col, val, area_g, area_c, norm)


def sliver_share(val):
    return float((np.asarray(val) < SLIVER).sum()) / max(len(val), 1)
