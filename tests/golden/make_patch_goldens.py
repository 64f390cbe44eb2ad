"""50-digit goldens of the patch rule (include/mpassit_amd.h, "patch regridding"): python tests/golden/make_patch_goldens.py writes
patch_hp.npz (inputs and expected rows) and patch_hp.json (what the cases are and which attempts they reach) next to itself.

The rule is evaluated by brute force in mpmath at 50 digits and uses nothing of the mirror (target_grid.patch_rows): the ring-1 patch
of a mesh cell comes straight from verticesOnCell -- the cells that share one of its vertices, counting only vertices listed by exactly
three cells -- ring 2 is the union of ring 1 over ring 1, a grid node takes its shifted 3 x 3 window; the frame, h, G and the pivots of
its Cholesky factor are computed in mpmath, the shape values by a dense solve of G y = phi(p).  Inputs are float64 (unit vectors from the
oracle, bilinear weights from the oracle for the meshes and from the projection's index space for the grids), the expected values are
the 50-digit results rounded once.

Cases: geodesic_mesh(6) and a 2 000-cell global_voronoi_mesh onto points spread over the sphere (the latter with every triangle that
touches a cell whose ring 1 is too small for degree 2: attempt B), a small regional hex mesh with its rim under a larger Lambert grid (B
at the rim), a 7 x 5 Lambert CENTER stagger onto that mesh's cells, and a 2 x 2 stagger onto them (four points: attempt C).  The
generator asserts that A, B and C all occur."""
import json
import os
import sys

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
mpmath.mp.dps = 50
mpf = mpmath.mpf
MAX_PNTS = 32
TOL = mpf(2) ** -26
LAMBERT = dict(ref_lat=38.5, ref_lon=-97.5, truelat1=38.5, truelat2=38.5, stand_lon=-97.5)


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def ring1_mesh(voc):
    """N1 of every cell from verticesOnCell alone"""
    cells_of = {}
    for c, row in enumerate(voc):
        for v in row:
            if v > 0:
                cells_of.setdefault(int(v), []).append(c)
    out = []
    for c, row in enumerate(voc):
        s = {c}
        for v in row:
            if v > 0 and len(cells_of[int(v)]) == 3:
                s.update(cells_of[int(v)])
        out.append(sorted(s))
    return out


def ring1_grid(snx, sny):
    out = []
    for j in range(sny):
        for i in range(snx):
            i0, j0 = min(max(i - 1, 0), max(snx - 3, 0)), min(max(j - 1, 0), max(sny - 3, 0))
            out.append(sorted(b * snx + a for b in range(j0, min(j0 + 3, sny)) for a in range(i0, min(i0 + 3, snx))))
    return out


class Fit:
    """the frame about node c, the patch's local coordinates, G and whether the attempt passes"""

    def __init__(self, X, c, patch, degree):
        self.patch, self.degree = patch, degree
        n = [mpf(float(X[k][c])) for k in range(3)]
        ax = min(range(3), key=lambda k: (abs(n[k]), k))
        a = [mpf(1) if k == ax else mpf(0) for k in range(3)]
        s = dot(a, n)
        t = [a[k] - s * n[k] for k in range(3)]
        r = mpmath.sqrt(dot(t, t))
        self.n, self.e1 = n, [t[k] / r for k in range(3)]
        e1 = self.e1
        self.e2 = [n[1] * e1[2] - n[2] * e1[1], n[2] * e1[0] - n[0] * e1[2], n[0] * e1[1] - n[1] * e1[0]]
        d = [[mpf(float(X[k][q])) - n[k] for k in range(3)] for q in patch]
        self.h = mpmath.sqrt(max(dot(x, x) for x in d))
        self.ok = self.h > 0
        if not self.ok:
            return
        self.phis = [self.phi(self.uv(x)) for x in d]
        m = len(self.phis[0])
        self.G = mpmath.matrix(m, m)
        for p in self.phis:
            for a_ in range(m):
                for b in range(m):
                    self.G[a_, b] += p[a_] * p[b]
        R = mpmath.matrix(m, m)                              # the pivots of G = R^T R
        for k in range(m):
            s = self.G[k, k] - sum(R[i, k] ** 2 for i in range(k))
            if not s > TOL * self.G[k, k]:
                self.ok = False
                return
            R[k, k] = mpmath.sqrt(s)
            for j in range(k + 1, m):
                R[k, j] = (self.G[k, j] - sum(R[i, k] * R[i, j] for i in range(k))) / R[k, k]

    def uv(self, d):
        return dot(d, self.e1) / self.h, dot(d, self.e2) / self.h

    def phi(self, uv):
        u, v = uv
        return [mpf(1), u, v] + ([u * u, u * v, v * v] if self.degree == 2 else [])

    def shape(self, P):
        d = [mpf(float(P[k])) - self.n[k] for k in range(3)]
        y = mpmath.lu_solve(self.G, mpmath.matrix(self.phi(self.uv(d))))
        return [sum(p[a] * y[a] for a in range(len(p))) for p in self.phis]


def node_fit(X, c, n1, is_mesh, cache):
    if c not in cache:
        p1 = n1[c]
        fit, att = None, "D"
        if len(p1) <= MAX_PNTS:
            if len(p1) >= 6:
                f = Fit(X, c, p1, 2)
                if f.ok:
                    fit, att = f, "A"
            if fit is None and is_mesh:
                p2 = sorted(set().union(*[n1[d] for d in p1]))
                if 6 <= len(p2) <= MAX_PNTS:
                    f = Fit(X, c, p2, 2)
                    if f.ok:
                        fit, att = f, "B"
            if fit is None and len(p1) >= 3:
                f = Fit(X, c, p1, 1)
                if f.ok:
                    fit, att = f, "C"
        cache[c] = (fit, att)
    return cache[c]


def rows(X, P, idx, w, n1, is_mesh):
    cache, counts = {}, dict(A=0, B=0, C=0, D=0)
    rowptr, col, val = [0], [], []
    for i in range(idx.shape[0]):
        acc = {}
        if idx[i, 0] >= 0:
            for s in range(idx.shape[1]):
                c = int(idx[i, s])
                if c < 0:
                    continue
                fit, att = node_fit(X, c, n1, is_mesh, cache)
                counts[att] += 1
                ids, L = ([c], [mpf(1)]) if fit is None else (fit.patch, fit.shape(P[:, i]))
                for q, l in zip(ids, L):
                    acc[q] = acc.get(q, mpf(0)) + mpf(float(w[i, s])) * l
        for q in sorted(acc):
            col.append(q)
            val.append(float(acc[q]))
        rowptr.append(len(col))
    return np.array(rowptr, np.int64), np.array(col, np.int32), np.array(val), counts


def main():
    from oracle import oracle as o
    from mpassit_amd import synth, target_grid as tg
    o.build()
    rng = np.random.default_rng(29)
    cases, arrays, meta = [], {}, {}

    def mesh_xyz(m):
        return o.lonlat_deg_to_xyz(*o.mesh_coords_deg(m.lonCell, m.latCell))

    def add_mesh(name, m, pts, what):
        x = mesh_xyz(m)
        tri, _ = o.dual_triangles(m.verticesOnCell, m.nVertices, x)
        idx, w = o.bilinear_weights(x, tri, pts)[:2]
        cases.append((name, what, x.T.copy(), pts.T.copy(), idx, w, ring1_mesh(m.verticesOnCell), True,
                      dict(voc=np.asarray(m.verticesOnCell, np.int32), tri=tri)))
        return x, tri

    def add_grid(name, g, lon_deg, lat_deg, pts, what):
        """CENTER stagger of g onto the points (lon_deg, lat_deg) = pts: bilinear weights in the projection's index space, the slots in the
        order (b, a), (b, a + 1), (b + 1, a + 1), (b + 1, a); a point outside the stagger is unmapped"""
        c = o.lonlat_deg_to_xyz(g.lon, g.lat)
        i0, j0 = g.proj.latlon_to_ij(g.lat[0, 0], g.lon[0, 0])
        fi, fj = g.proj.latlon_to_ij(lat_deg, lon_deg)
        fi, fj = fi - i0, fj - j0
        inside = (fi >= 0) & (fi <= g.nx - 1) & (fj >= 0) & (fj <= g.ny - 1)
        a, b = np.clip(np.floor(fi).astype(np.int64), 0, g.nx - 2), np.clip(np.floor(fj).astype(np.int64), 0, g.ny - 2)
        s, t_ = fi - a, fj - b
        idx = np.stack([b * g.nx + a, b * g.nx + a + 1, (b + 1) * g.nx + a + 1, (b + 1) * g.nx + a], axis=1)
        w = np.stack([(1 - s) * (1 - t_), s * (1 - t_), s * t_, (1 - s) * t_], axis=1)
        idx[~inside], w[~inside] = -1, 0.0
        cases.append((name, what, c.T.copy(), pts.T.copy(), idx, w, ring1_grid(g.nx, g.ny), False, dict(shape=np.array([g.nx, g.ny], np.int32))))

    def sphere_points(n):
        v = rng.normal(size=(n, 3))
        return v / np.sqrt((v * v).sum(axis=1))[:, None]

    add_mesh("geodesic6", synth.geodesic_mesh(6), sphere_points(90), "geodesic_mesh(6) onto 90 points spread over the sphere")
    m = synth.global_voronoi_mesh(2000)
    x = mesh_xyz(m)
    tri, _ = o.dual_triangles(m.verticesOnCell, m.nVertices, x)
    n1 = ring1_mesh(m.verticesOnCell)
    small = [c for c in range(m.nCells) if len(n1[c]) < 6]
    near = [t.mean(axis=0) for t in x[tri[(tri >= 0).all(axis=1) & np.isin(tri, small).any(axis=1)]]]     # centroids of their triangles
    pts = np.concatenate([sphere_points(70)] + ([np.array(near) / np.linalg.norm(near, axis=1)[:, None]] if near else []))
    add_mesh("voronoi2000", m, pts, "global_voronoi_mesh(2000) onto 70 points spread over the sphere and the centroids of every dual triangle "
             "with a cell of fewer than six ring-1 points (%d cells)" % len(small))
    gs = tg.define_target_grid_params("lambert", 10, 8, dx=30000.0, dy=30000.0, **LAMBERT)
    hexm = synth.regional_mesh_for_lambert(gs.proj, 10, 8, 130, margin=0.0, seed=7)
    gl = tg.define_target_grid_params("lambert", 13, 11, dx=30000.0, dy=30000.0, **LAMBERT)
    hlon, hlat = o.mesh_coords_deg(hexm.lonCell, hexm.latCell)
    hx, _ = add_mesh("regional hex", hexm, o.lonlat_deg_to_xyz(gl.lon, gl.lat), "regional_mesh_for_lambert(9 x 7 at 30 km, 130 cells) with its rim under "
                     "a 12 x 10 Lambert grid")
    add_grid("grid7x5 to cells", tg.define_target_grid_params("lambert", 8, 6, dx=30000.0, dy=30000.0, **LAMBERT), hlon, hlat, hx,
             "a 7 x 5 Lambert CENTER stagger (30 km) onto that mesh's cells")
    add_grid("grid2x2 to cells", tg.define_target_grid_params("lambert", 3, 3, dx=30000.0, dy=30000.0, **LAMBERT), hlon, hlat, hx,
             "a 2 x 2 Lambert CENTER stagger (30 km) onto that mesh's cells: four points, degree 1")
    total = dict(A=0, B=0, C=0, D=0)
    for k, (name, what, X, P, idx, w, n1, is_mesh, extra) in enumerate(cases):
        rowptr, col, val, counts = rows(X, P, idx, w, n1, is_mesh)
        mapped = int((idx[:, 0] >= 0).sum())
        print("%s: %d sources, %d rows (%d mapped), %d entries, attempts %s" % (name, X.shape[1], P.shape[1], mapped, col.size, counts))
        assert mapped > 0 and np.array_equal(np.diff(rowptr) > 0, idx[:, 0] >= 0)
        for a in total:
            total[a] += counts[a]
        pre = "c%d_" % k
        arrays.update({pre + "src_xyz": X, pre + "dst_xyz": P, pre + "idx": idx.astype(np.int32), pre + "w": w, pre + "rowptr": rowptr,
                       pre + "col": col, pre + "val": val})
        arrays.update({pre + key: v for key, v in extra.items()})
        meta[name] = dict(index=k, what=what, mesh=bool(is_mesh), n_src=int(X.shape[1]), n_dst=int(P.shape[1]), mapped=mapped, nnz=int(col.size),
                          attempts=counts)
    assert total["A"] > 0 and total["B"] > 0 and total["C"] > 0, total      # every attempt the rule reaches on these cases
    meta["_total"] = total
    np.savez_compressed(os.path.join(HERE, "patch_hp.npz"), **arrays)
    with open(os.path.join(HERE, "patch_hp.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print("attempts over all cases:", total)


if __name__ == "__main__":
    main()
