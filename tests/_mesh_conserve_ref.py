"""float64 numpy reference of the conservative Mesh -> Mesh Store (include/mpassit_amd.h, mpg_regrid_store_conserve_mesh).

I(d, s), the area of source polygon s inside destination polygon d, exactly as the header states it: the source polygon is the subject,
made counter-clockwise by the sign of its own fan area (its listed order reversed when that is negative); it is clipped by the
destination polygon's sides in listed order, that polygon made counter-clockwise the same way; clip-plane normals in difference form
a x (b - a); Sutherland-Hodgman with the 1e-15 * |n| inside rule; a side with |b - a|^2 < 1e-24 bounds nothing; the area is the triangle
fan from slot 0, clamped at 0.  Candidates by brute force: every pair whose bounding caps overlap.  The clip runs over the whole pair
list at once (one numpy step per clip side and polygon slot), so a few thousand cells take well under a second.

Polygons are (xyz [n][M][3], count [n]): the first count[i] slots of row i are polygon i's vertices in listed order.  Mesh cells come
from verticesOnCell (polygons_of_mesh), grid cells from the four CORNER points around a centre (polygons_of_grid) -- the second form
lets the same code be held against oracle.conserve.  One answer per mesh pair is cached (answer()), never modified."""
import numpy as np

import _mesh_to_mesh_cases as MC
from _conserve_to_mesh_ref import NORM_DSTAREA, NORM_FRACAREA, SLIVER, SLIVER_CAP, SLIVER_RULE, mesh_cell_areas, tri_area

__all__ = ["NORM_DSTAREA", "NORM_FRACAREA", "SLIVER", "SLIVER_CAP", "polygons_of_mesh", "polygons_of_grid", "fan_areas", "cap_pairs",
           "clip_areas", "intersections", "rows", "thin", "tol_meshes", "answer", "PAIRS"]

PAIRS = ("geo10_to_vor1500", "vor2500_to_hex", "hex_to_geo10", "varres3000_to_geo8")   # the cell pairs of tests/_mesh_to_mesh_cases.py


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def polygons_of_mesh(voc, vert_xyz):
    """The Voronoi cells: valid entries of every verticesOnCell row (1-based, <= 0 pads anywhere) compacted to the front."""
    voc = np.asarray(voc)
    n, M = voc.shape
    ok = voc > 0
    cnt = ok.sum(axis=1)
    order = np.argsort(~ok, axis=1, kind="stable")                      # valid entries first, in listed order
    ids = np.take_along_axis(voc, order, axis=1)
    xyz = np.asarray(vert_xyz, np.float64)[np.maximum(ids, 1) - 1]
    xyz[np.arange(M)[None, :] >= cnt[:, None]] = 0.0
    return xyz, cnt


def polygons_of_grid(corner_xyz, nx, ny):
    """The grid's cells, index j * nx + i: corners (i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1)."""
    c = np.asarray(corner_xyz, np.float64).reshape(ny + 1, nx + 1, 3)
    xyz = np.stack([c[:-1, :-1], c[:-1, 1:], c[1:, 1:], c[1:, :-1]], axis=2).reshape(nx * ny, 4, 3)
    return xyz, np.full(nx * ny, 4, np.int64)


def fan_areas(xyz, cnt):
    """Signed fan area of every polygon from its first vertex, in listed order (0 for fewer than three vertices)."""
    area = np.zeros(xyz.shape[0])
    for k in range(1, xyz.shape[1] - 1):
        m = cnt > k + 1
        area[m] += tri_area(xyz[m, 0], xyz[m, k], xyz[m, k + 1])
    return area


def _ccw(xyz, cnt):
    """Every polygon counter-clockwise seen from outside: the listed order reversed where the fan area is negative."""
    rev = fan_areas(xyz, cnt) < 0.0
    out = xyz.copy()
    M = xyz.shape[1]
    k = np.arange(M)[None, :]
    src = np.where(k < cnt[:, None], cnt[:, None] - 1 - k, k)
    out[rev] = np.take_along_axis(xyz[rev], src[rev][:, :, None], axis=1)
    return out


def _caps(xyz, cnt):
    """(centre [n][3], angular radius [n]) of a cap that holds every polygon: the normalised vertex mean and the largest angle to a
    vertex (a cap smaller than a hemisphere is convex, so it holds the great-circle sides and the interior too)."""
    valid = (np.arange(xyz.shape[1])[None, :] < cnt[:, None])
    c = (xyz * valid[:, :, None]).sum(axis=1)
    c /= np.maximum(np.linalg.norm(c, axis=1), 1e-300)[:, None]
    chord = np.linalg.norm(xyz - c[:, None, :], axis=2) * valid
    return c, 2.0 * np.arcsin(np.minimum(0.5 * chord.max(axis=1), 1.0))


def cap_pairs(dst, src, slack=1e-9):
    """Brute-force candidates: every (d, s) whose caps overlap, polygons without an area left out.  Returns (d [Np], s [Np]), d-major."""
    (dx, dn), (sx, sn) = dst, src
    cd, rd = _caps(dx, dn)
    cs, rs = _caps(sx, sn)
    okd, oks = fan_areas(dx, dn) != 0.0, fan_areas(sx, sn) != 0.0
    out_d, out_s = [], []
    step = max(1, (1 << 22) // max(cs.shape[0], 1))
    for d0 in range(0, cd.shape[0], step):
        ang = 2.0 * np.arcsin(np.minimum(0.5 * np.linalg.norm(cd[d0:d0 + step, None, :] - cs[None, :, :], axis=2), 1.0))
        hit = (ang <= rd[d0:d0 + step, None] + rs[None, :] + slack) & okd[d0:d0 + step, None] & oks[None, :]
        d, s = np.nonzero(hit)
        out_d.append(d + d0)
        out_s.append(s)
    return np.concatenate(out_d).astype(np.int64), np.concatenate(out_s).astype(np.int64)


def clip_areas(subj_xyz, subj_n, clip_xyz, clip_n):
    """I for aligned lists of pairs: row t of the subject polygons clipped by row t of the clip polygons (both counter-clockwise)."""
    Np, Ms = subj_xyz.shape[:2]
    Mc = clip_xyz.shape[1]
    cap = Ms + Mc                                                        # a convex m-gon cut by a convex n-gon: at most m + n vertices
    poly = np.zeros((Np, cap, 3))
    poly[:, :Ms] = subj_xyz
    n = subj_n.astype(np.int64).copy()
    rows_all = np.arange(Np)
    for e in range(Mc):
        nxt = np.where(e + 1 == clip_n, 0, np.minimum(e + 1, Mc - 1))
        qa, qb = clip_xyz[:, e], clip_xyz[rows_all, nxt]
        side = qb - qa
        act = (e < clip_n) & (n >= 3) & ~(_dot(side, side) < 1e-24)
        if not act.any():
            continue
        nrm = _cross(qa, side)
        eps = 1e-15 * np.sqrt(_dot(nrm, nrm))
        out = np.zeros_like(poly)
        m = np.zeros(Np, np.int64)
        nmax = int(n[act].max())
        for i in range(nmax):
            on = act & (i < n)
            r = rows_all[on]
            X1 = poly[r, i]
            X2 = poly[r, np.where(i + 1 == n[r], 0, i + 1)]
            d1, d2 = _dot(nrm[r], X1), _dot(nrm[r], X2)
            in1, in2 = d1 >= -eps[r], d2 >= -eps[r]
            k = r[in1]
            out[k, m[k]] = X1[in1]
            m[k] += 1
            x = in1 != in2
            X = X1[x] * d2[x][:, None] - X2[x] * d1[x][:, None]
            sgn = np.where((d2[x] - d1[x]) > 0.0, 1.0, -1.0)
            nn = np.sqrt(_dot(X, X))
            good = nn > 0.0
            k = r[x][good]
            out[k, m[k]] = X[good] * (sgn[good] / nn[good])[:, None]
            m[k] += 1
        poly[act] = out[act]
        n[act] = m[act]
    assert n.max(initial=0) <= cap
    area = np.zeros(Np)
    for k in range(1, cap - 1):
        on = n > k + 1
        area[on] += tri_area(poly[on, 0], poly[on, k], poly[on, k + 1])
    return np.maximum(area, 0.0)


def intersections(dst, src, pairs=None):
    """(d, s, I) over the candidate pairs (all cap pairs unless given), d-major and s ascending within d."""
    (dx, dn), (sx, sn) = dst, src
    d, s = cap_pairs(dst, src) if pairs is None else pairs
    dc, sc = _ccw(dx, dn), _ccw(sx, sn)
    inter = np.zeros(d.size)
    for a in range(0, d.size, 1 << 16):                                  # bounded memory
        b = a + (1 << 16)
        inter[a:b] = clip_areas(sc[s[a:b]], sn[s[a:b]], dc[d[a:b]], dn[d[a:b]])
    return d, s, inter


def rows(d, s, inter, area_d, norm=NORM_DSTAREA):
    """CSR rows keyed by destination polygon from the intersections: the 1e-14 rule, columns ascending, both norms, frac."""
    n_dst = area_d.size
    keep = inter > SLIVER_RULE * area_d[d]
    d, s, inter = d[keep], s[keep], inter[keep]
    order = np.lexsort((s, d))
    d, s, inter = d[order], s[order], inter[order]
    cover = np.bincount(d, weights=inter, minlength=n_dst)
    frac = np.where(area_d > 0, cover / np.maximum(area_d, 1e-300), 0.0)
    div = area_d[d] if norm == NORM_DSTAREA else cover[d]
    rowptr = np.zeros(n_dst + 1, np.int64)
    np.cumsum(np.bincount(d, minlength=n_dst), out=rowptr[1:])
    return rowptr, s.astype(np.int32), inter / div, frac


def thin(voc, vert_xyz):
    """h = area / diameter of every cell with an area (tests/_conserve_to_mesh_ref.py tol_both, its mesh half)."""
    voc = np.asarray(voc)
    ma = mesh_cell_areas(voc, vert_xyz)
    v = vert_xyz[np.maximum(voc, 1) - 1]
    v = np.where((voc > 0)[..., None], v, v[:, :1])                      # pads repeat the first vertex
    diam = np.linalg.norm(v[:, :, None, :] - v[:, None, :, :], axis=-1).max(axis=(1, 2))
    return (ma / np.maximum(diam, 1e-300))[ma > 0]


def tol_meshes(voc_a, vxyz_a, voc_b, vxyz_b):
    """The project's conservative bar, max(1e-11, 64 eps / min h), h = area / diameter over BOTH meshes' cells."""
    return max(1e-11, 64 * np.finfo(np.float64).eps / min(thin(voc_a, vxyz_a).min(), thin(voc_b, vxyz_b).min()))


class Answer:
    """Everything the tests need of one mesh pair, computed once: polygons, areas, intersections, the bar, rows per norm."""

    def __init__(self, o, src, dst):
        self.src, self.dst = src, dst
        self.vs = o.lonlat_deg_to_xyz(*o.mesh_coords_deg(src.lonVertex, src.latVertex))
        self.vd = self.vs if dst is src else o.lonlat_deg_to_xyz(*o.mesh_coords_deg(dst.lonVertex, dst.latVertex))
        self.ps, self.pd = polygons_of_mesh(src.verticesOnCell, self.vs), polygons_of_mesh(dst.verticesOnCell, self.vd)
        self.area_s, self.area_d = mesh_cell_areas(src.verticesOnCell, self.vs), mesh_cell_areas(dst.verticesOnCell, self.vd)
        self.d, self.s, self.inter = intersections(self.pd, self.ps)
        self.tol = tol_meshes(src.verticesOnCell, self.vs, dst.verticesOnCell, self.vd)
        for a in (self.vs, self.vd, self.area_s, self.area_d, self.d, self.s, self.inter):
            a.setflags(write=False)
        self._rows = {}

    def rows(self, norm=NORM_DSTAREA):
        if norm not in self._rows:
            r = rows(self.d, self.s, self.inter, self.area_d, norm)
            for a in r:
                a.setflags(write=False)
            self._rows[norm] = r
        return self._rows[norm]


_ANSWERS = {}


def answer(o, name):
    """The cached Answer of pair `name` of tests/_mesh_to_mesh_cases.py, or of "<mesh>_self" (src == dst)."""
    if name not in _ANSWERS:
        if name.endswith("_self"):
            m = MC.mesh(name[:-5])
            _ANSWERS[name] = Answer(o, m, m)
        else:
            src, dst, loc = MC.pair(name)
            assert loc == 0
            _ANSWERS[name] = Answer(o, src, dst)
    return _ANSWERS[name]
