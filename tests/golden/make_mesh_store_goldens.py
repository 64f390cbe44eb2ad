#!/usr/bin/env python3
"""Generator of tests/golden/mesh_store_hp.{json,npz} and tests/golden/mesh_store_global_hp.{json,npz} -- the Grid -> Mesh, periodic
Grid -> Mesh and Mesh -> Mesh Stores and the mesh rotation angles by brute force at 50 digits (mpmath), the sibling of
make_store_goldens.py (whose helpers it imports and whose fixture it does not touch).  A directory as the first argument receives the
files instead of tests/golden.

Every expectation is built from the STATEMENT of the rule in include/mpassit_amd.h, by a route that shares nothing with the kernels, the
oracle or the float64 restatements under tests/_*_ref.py: every point against every figure a generous float64 distance pre-filter keeps
(the only float64 step), unit vectors formed at 50 digits from the float64 latitudes / longitudes the tests hand to the library, no
search structure.

* Grid -> Mesh bilinear (mpg_regrid_store_to_mesh): for every mesh point P and every quad A = (b, a), B = (b, a+1), C = (b+1, a+1),
  D = (b+1, a) of the stagger, X(xi, eta) = A + xi (B - A) + eta (D - A) + xi eta (A - B + C - D) = t P by mpmath.findroot at 40 digits
  from (0.5, 0.5, 1); the winner is the lowest quad id b * (snx - 1) + a with t > 0 and xi, eta in [-1e-10, 1 + 1e-10].
* Grid -> Mesh nearest, Mesh -> Mesh nearest: argmin of the chord distance over ALL source points.
* periodic Grid -> Mesh (mpg_regrid_store_periodic_to_mesh): the same solve on the quads b in [0, ny - 2], a in [0, nx - 1] with the
  column wrapped mod nx, id b * nx + a; where no quad passed, the 2 nx cap triangles (A, B, N) / (B, A, S) onto the pole node
  (0, 0, sign of the mean z of the end row), planar barycentric weights seen from the centre (3 x 3 solve), tolerance 1e-10, ids
  0 .. nx - 1 on the row-0 end and nx .. 2 nx - 1 on the other, the lowest passing id.
* Mesh -> Mesh bilinear (mpg_regrid_store_mesh): the dual triangles of the source mesh (the vertices touched by exactly three cells,
  triangle id = vertex id), the lowest id for which the 3 x 3 solve passes with tolerance 1e-10; line type 0: A + u (B - A) + v (C - A)
  = t P, t > 0; line type 1: P dropped along the triangle's normal, triangles whose outward normal faces away from P left out.
* conservative Mesh -> Mesh (mpg_regrid_store_conserve_mesh): Voronoi cell against Voronoi cell by the 50-digit Sutherland-Hodgman
  clip, areas by GIRARD's theorem -- the true spherical area, which the header's triangle fan approximates.
* angles (mpg_mesh_rotang_dev, mpg_mesh_edge_rotang_dev): the forward Lambert conformal map (llij_lc) differentiated at 50
  digits with mpmath.diff; the earth vector whose image is the grid's +j axis has east / north components (e, n), alpha =
  atan2(-e, n) (get_rotang's sign).  The closed form alpha = -cone * dlon is NOT used.

Format.  mesh_store_hp holds the two Lambert cases (Grid -> Mesh bilinear and nearest from CENTER, EDGE1, EDGE2 onto cells, vertices and
edges; the angles), mesh_store_global_hp the periodic cases and the mesh pairs.  Each is a pair of files: <stem>.json, the document
{"note", "arrays", "meshes": {name: latCell, lonCell, latVertex, lonVertex, verticesOnCell and, where a case uses the edges, latEdge,
lonEdge, angleEdge} (radians, each mesh once), "cases": [...]} with every LIST replaced by {"@": its path in the document}, and <stem>.npz,
which holds those lists under their paths as float64 / int32 arrays (uncompressed, members in sorted order with a fixed time stamp, so a
rerun gives the same bytes).  A regional case holds its grid's coordinates (degrees), a periodic one its 1-D longitudes [nx] and
latitudes [ny] (degrees).  A list of per-point entries (the points of one mesh location: "cell", "vertex", "edge") is the two arrays
"<path>/k" (int32: the kind, then the entry's integers) and "<path>/f" (float64: its real numbers), one row per point, zeros where an
entry has no such number:
  kind 0          null: in no quad / no quad and no cap / in no triangle
  kind 5 quad     k = (5, quad id), f = (xi, eta): the columns A, B, C, D follow from the id and the weights are (1-xi)(1-eta), xi (1-eta),
                  xi eta, (1-xi) eta (the float64 products of the rounded xi, eta are within 3e-16 of the rounded 50-digit weights); in a
                  periodic case a seam row where id mod nx = nx - 1.  kind 6: the same, within 1e-9 (in xi or eta) of the border of two
                  quads -- either neighbour is right.  kind 1 "hull": within 1e-9 (held) or 1e-6 (not held) of the hull -- mapped or not
                  is a tolerance's business.
  kind 4 cap      k = (4, cap id), f = (t_A, t_B, t_pole): the row has nx entries, wr = t_pole / nx everywhere, t_A + wr on A, t_B + wr on
                  B.  kind 2 "tie": within 1e-9 of a quad's or a cap triangle's border, skipped.  The entries are those of
                  MPG_POLEMETHOD_ALLAVG; under MPG_POLEMETHOD_NONE the cap entries are null and nothing else changes (caps are tried only
                  where no quad passed).  "on_edge": eight more points, the midpoints of chords of the two end rows (lon, lat in
                  radians): a quad passes there within the tolerance, so the header's row is that quad's (kind 7), weights good to 3e-9
                  -- what a cap tried before the quads gets wrong.
  kind 8 triangle k = (8, the three cells ascending), f = their weights; kind 2 "tie": within 1e-9 of a triangle's border, skipped; kind 3
                  "corner": k = (3, c), the point IS cell centre c (src == dst: weight 1 on c).
  nearest         int32 per point: the source index, or -1 where the runner-up is within 1e-9 relative (a tie); src == dst has none on
                  the vertices (a Voronoi vertex is equidistant from three centres).
  conservative    "conserve": rows of (row, column, I / area(row)), float64 (MPG_NORM_DSTAREA; entries below 1e-30 are the 50-digit clip's zeros and
                  are left out), "frac": sum_s I / area(d) per destination cell.  MPG_NORM_FRACAREA is w / frac.
  angles          "cosa" / "sina" per location; edges also "cn" / "sn" = cos / sin of angleEdge - alpha.
Conditions checked here (the run fails otherwise): at most 2 % of a list's points marked tie / hull (corner points of src == dst apart),
at least 50 comparable points per list, at least 100 conservative entries, seam rows and cap rows at both poles in every periodic case.

    python tests/golden/make_mesh_store_goldens.py        # rewrites the four files (deterministic; about 3 minutes)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import mpmath as mp  # noqa: E402
from make_store_goldens import ccw, f3, xyz_from_deg, xyz_from_rad  # noqa: E402
from make_weight_goldens import clip, cross, dedupe, dot, girard_area, sub, tri_weights, tri_weights_normal  # noqa: E402

mp.mp.dps = 50
E9, E10, E6 = mp.mpf(10) ** -9, mp.mpf(10) ** -10, mp.mpf(10) ** -6
LOCS = ("cell", "vertex", "edge")


def mesh_points(m, loc):
    lon, lat = {"cell": (m.lonCell, m.latCell), "vertex": (m.lonVertex, m.latVertex), "edge": (m.lonEdge, m.latEdge)}[loc]
    return [xyz_from_rad(lon[i], lat[i]) for i in range(lon.size)]


def farr(P):
    return np.array([f3(p) for p in P])


# ---- quads ----------------------------------------------------------------------------------------------------------------------------
def quad_solve(A, B, C, D, P):
    f = lambda s_, t_, l_: [A[k] + s_ * (B[k] - A[k]) + t_ * (D[k] - A[k]) + s_ * t_ * (A[k] - B[k] + C[k] - D[k]) - l_ * P[k] for k in range(3)]  # noqa: E731
    try:
        sol = mp.findroot(f, (mp.mpf("0.5"), mp.mpf("0.5"), mp.mpf(1)), tol=mp.mpf(10) ** -40, maxsteps=60)
    except (ValueError, ZeroDivisionError):
        return None
    return sol[0], sol[1], sol[2]


def quads_of(S, periodic):
    """S [sny][snx] of 50-digit unit vectors -> (ids, corner index pairs, float64 centres, float64 radii)"""
    sny, snx = len(S), len(S[0])
    qnx = snx if periodic else snx - 1
    Sf = np.array([[f3(S[j][i]) for i in range(snx)] for j in range(sny)])
    ids, corners, ctr, rad = [], [], [], []
    for b in range(sny - 1):
        for a in range(qnx):
            a1 = (a + 1) % snx
            cs = ((b, a), (b, a1), (b + 1, a1), (b + 1, a))
            pts = np.array([Sf[j, i] for j, i in cs])
            c = pts.mean(axis=0)
            ids.append(b * qnx + a)
            corners.append(cs)
            ctr.append(c)
            rad.append(np.linalg.norm(pts - c, axis=1).max())
    return ids, corners, np.array(ctr), np.array(rad)


def quad_search(S, P, periodic=False, literal=False):
    """One entry per point of P: the quad rule of the header.  literal: a point within 1e-9 of a border gets the header's own winner (the
    lowest passing id), marked "on_edge", instead of a tie / hull mark."""
    ids, corners, ctr, rad = quads_of(S, periodic)
    Pf = farr(P)
    out = []
    for p in range(len(P)):
        cand = np.nonzero(np.linalg.norm(ctr - Pf[p], axis=1) <= 1.6 * rad + 1e-9)[0]      # a held point lies within the quad's radius (+ sagitta)
        passing, strict, border, near_out = [], [], [], False
        for k in cand:
            (ja, ia), (jb, ib), (jc, ic), (jd, id_) = corners[k]
            sol = quad_solve(S[ja][ia], S[jb][ib], S[jc][ic], S[jd][id_], P[p])
            if sol is None or sol[2] <= 0:
                continue
            xi, eta = sol[0], sol[1]
            out_by = max(-xi, xi - 1, -eta, eta - 1)                                        # > 0: that far outside this quad
            if out_by <= E10:
                passing.append((ids[k], xi, eta))
            if abs(out_by) <= E9:
                border.append(ids[k])
            elif out_by < 0:
                strict.append(ids[k])
            elif out_by < E6:
                near_out = True
        if not passing and not border:
            out.append({"hull": 1} if near_out else None)
        elif border and literal and passing:
            q, xi, eta = min(passing)
            out.append({"q": int(q), "xi": float(xi), "eta": float(eta), "on_edge": 1})
        elif border:
            if passing and (strict or len(border) >= 2):
                q, xi, eta = min(passing)
                out.append({"q": int(q), "xi": float(xi), "eta": float(eta), "tie": 1})
            else:
                out.append({"hull": 1})
        else:
            assert len(strict) == 1 and len(passing) == 1, (p, strict, passing)
            q, xi, eta = passing[0]
            out.append({"q": int(q), "xi": float(xi), "eta": float(eta)})
    return out


def nearest_search(Sflat, P):
    Sf, Pf = farr(Sflat), farr(P)
    out = []
    for p in range(len(P)):
        d = np.linalg.norm(Sf - Pf[p], axis=1)
        cand = np.nonzero(d <= d.min() * (1 + 1e-6) + 1e-12)[0]
        dd = sorted((mp.sqrt(dot(sub(Sflat[c], P[p]), sub(Sflat[c], P[p]))), int(c)) for c in cand)
        tie = len(dd) > 1 and (dd[1][0] - dd[0][0]) <= E9 * dd[0][0]
        out.append(-1 if tie else dd[0][1])
    return out


# ---- periodic: quads with the seam column, then the caps ------------------------------------------------------------------------------
def periodic_search(S, P, literal=False):
    ny, nx = len(S), len(S[0])
    out = quad_search(S, P, periodic=True, literal=literal)
    zmean = [sum(float(S[j][i][2]) for i in range(nx)) / nx for j in (0, ny - 1)]
    assert min(abs(z) for z in zmean) > 0.1
    pole = [[mp.mpf(0), mp.mpf(0), mp.mpf(1 if z > 0 else -1)] for z in zmean]
    for p, e in enumerate(out):
        if e is not None and "hull" in e:            # on the border between the last row of quads and a cap
            out[p] = {"tie": 1}
            continue
        if e is not None:
            e["kind"] = "seam" if e["q"] % nx == nx - 1 else "quad"
            continue
        passing, border = [], False
        for end, row in enumerate((0, ny - 1)):
            north = pole[end][2] > 0
            for a in range(nx):
                A, B = S[row][a], S[row][(a + 1) % nx]
                if north:
                    (tA, tB, tP), t = tri_weights(A, B, pole[end], P[p])
                else:
                    (tB, tA, tP), t = tri_weights(B, A, pole[end], P[p])
                if t <= 0:
                    continue
                lo = min(tA, tB, tP)
                if abs(lo) <= E9:
                    border = True
                if lo >= -E10:
                    passing.append((end * nx + a, tA, tB, tP))
        if border:
            out[p] = {"tie": 1}
        elif passing:
            assert len(passing) == 1, (p, passing)
            c, tA, tB, tP = passing[0]
            out[p] = {"kind": "cap", "cap": int(c), "t": [float(tA), float(tB), float(tP)]}
    return out


# ---- Mesh -> Mesh ---------------------------------------------------------------------------------------------------------------------
def dual_triangles(m):
    cov = [[] for _ in range(m.nVertices)]
    for c in range(m.nCells):
        for v in m.verticesOnCell[c]:
            if v > 0:
                cov[v - 1].append(c)
    return [(v, tuple(cs)) for v, cs in enumerate(cov) if len(cs) == 3]


def tri_search(C, tris, P, linetype):
    Cf, Pf = farr(C), farr(P)
    tri_r = np.array([max(np.linalg.norm(Cf[a] - Cf[b]), np.linalg.norm(Cf[b] - Cf[c]), np.linalg.norm(Cf[a] - Cf[c])) for _, (a, b, c) in tris])
    tri_c = np.array([Cf[a] for _, (a, _, _) in tris])
    out = []
    for p in range(len(P)):
        near = np.nonzero(np.linalg.norm(tri_c - Pf[p], axis=1) <= 1.5 * tri_r + 1e-9)[0]
        passing, border = [], False
        for k in near:
            tid, (a, b, c) = tris[k]
            if linetype == 0:
                w, t = tri_weights(C[a], C[b], C[c], P[p])
                if t <= 0:
                    continue
            else:
                n = cross(sub(C[b], C[a]), sub(C[c], C[a]))
                if dot(n, [C[a][i] + C[b][i] + C[c][i] for i in range(3)]) < 0:
                    n = [-x for x in n]
                if dot(n, P[p]) <= 0:                # the triangle faces away from the point
                    continue
                w = tri_weights_normal(C[a], C[b], C[c], P[p])
            lo = min(w)
            if abs(lo) <= E9:
                border = True
            if lo >= -E10:
                passing.append((tid, (a, b, c), w))
        if border:
            e = {"tie": 1}
            d = np.linalg.norm(Cf - Pf[p], axis=1)
            if d.min() < 1e-12:
                e["corner"] = int(d.argmin())
            out.append(e)
        elif not passing:
            out.append(None)
        else:
            _, ids, w = min(passing, key=lambda h: h[0])
            order = sorted(range(3), key=lambda k: ids[k])
            out.append({"col": [int(ids[k]) for k in order], "w": [float(w[k]) for k in order]})
    return out


def cell_polys(m, V):
    polys = [ccw([V[v - 1] for v in m.verticesOnCell[c] if v > 0]) for c in range(m.nCells)]
    ctr = np.array([np.mean([f3(q) for q in poly], axis=0) for poly in polys])
    rad = np.array([max(np.linalg.norm(f3(q) - ctr[c]) for q in poly) for c, poly in enumerate(polys)])
    return polys, ctr, rad


def conserve_mesh(src, dst):
    Vs = [xyz_from_rad(src.lonVertex[i], src.latVertex[i]) for i in range(src.nVertices)]
    ps, cs, rs = cell_polys(src, Vs)
    if dst is src:
        pd, cd, rd = ps, cs, rs
    else:
        Vd = [xyz_from_rad(dst.lonVertex[i], dst.latVertex[i]) for i in range(dst.nVertices)]
        pd, cd, rd = cell_polys(dst, Vd)
    trip, frac = [], []
    for d in range(dst.nCells):
        area = girard_area(pd[d])
        cover = mp.mpf(0)
        for s in np.nonzero(np.linalg.norm(cs - cd[d], axis=1) <= (rs + rd[d]) * 1.05 + 1e-9)[0]:
            poly = list(ps[s])
            for e in range(len(pd[d])):
                poly = clip(poly, pd[d][e], pd[d][(e + 1) % len(pd[d])])
                if len(poly) < 3:
                    break
            poly = dedupe(poly)
            if len(poly) < 3:
                continue
            a = girard_area(poly)
            if a / area > mp.mpf(10) ** -30:
                trip.append([d, int(s), float(a / area)])
                cover += a
        frac.append(float(cover / area))
    return trip, frac


# ---- angles ---------------------------------------------------------------------------------------------------------------------------
def lambert_forward(proj):
    """(lon, lat in radians) -> (x, y) in grid units with the pole at the origin: r = rebydx cos(tl1) / cone * (tan((90 hemi - lat) / 2) /
    tan((90 hemi - tl1) / 2)) ^ cone, x = hemi r sin(cone dlon), y = -hemi r cos(cone dlon) (llij_lc up to the pole's offset)."""
    rad = mp.pi / 180
    hemi = -1 if proj.truelat1 < 0 else 1
    tl1, tl2, std = mp.mpf(proj.truelat1), mp.mpf(proj.truelat2), mp.mpf(proj.stdlon) * rad
    if abs(tl1 - tl2) > mp.mpf("0.1"):
        cone = (mp.log(mp.cos(tl1 * rad)) - mp.log(mp.cos(tl2 * rad))) / (mp.log(mp.tan((45 - abs(tl1) / 2) * rad)) - mp.log(mp.tan((45 - abs(tl2) / 2) * rad)))
    else:
        cone = mp.sin(abs(tl1) * rad)
    k = mp.cos(tl1 * rad) / cone / mp.tan((90 * hemi - tl1) * rad / 2) ** cone

    def fwd(lon, lat):
        r = k * mp.tan((mp.pi / 2 * hemi - lat) / 2) ** cone
        d = lon - std
        d = d - 2 * mp.pi * mp.floor((d + mp.pi) / (2 * mp.pi))
        return hemi * r * mp.sin(cone * d), -hemi * r * mp.cos(cone * d)
    return fwd


def angles(proj, lon, lat, angle_edge=None):
    fwd = lambert_forward(proj)
    cosa, sina, cn, sn = [], [], [], []
    for i in range(lon.size):
        lo, la = mp.mpf(float(lon[i])), mp.mpf(float(lat[i]))
        # images of the unit east and north vectors
        ex, ey = (mp.diff(lambda t: fwd(t, la)[k], lo) / mp.cos(la) for k in (0, 1))
        nx_, ny_ = (mp.diff(lambda t: fwd(lo, t)[k], la) for k in (0, 1))
        # a e + b n -> (0, 1): the grid's +j axis as an earth vector
        det = ex * ny_ - nx_ * ey
        a, b = -nx_ / det, ex / det
        alpha = mp.atan2(-a, b)
        cosa.append(float(mp.cos(alpha)))
        sina.append(float(mp.sin(alpha)))
        if angle_edge is not None:
            phi = mp.mpf(float(angle_edge[i])) - alpha
            cn.append(float(mp.cos(phi)))
            sn.append(float(mp.sin(phi)))
    out = {"cosa": cosa, "sina": sina}
    if angle_edge is not None:
        out.update(cn=cn, sn=sn)
    return out


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
PROBLEMS = []


def qualify(label, entries, skipped, corner_ok=False, floor=50):
    n = len(entries)
    marked = sum(1 for e in entries if skipped(e) and not (corner_ok and isinstance(e, dict) and "corner" in e))
    compared = sum(1 for e in entries if e is not None and not skipped(e)) + (sum(1 for e in entries if isinstance(e, dict) and "corner" in e) if corner_ok else 0)
    ok = marked <= 0.02 * n and compared >= floor
    print("    %-44s %4d points, %4d compared, %3d null, %2d tie / hull%s" % (label, n, compared, sum(e is None for e in entries), marked, "" if ok else "   <-- FAILS"), flush=True)
    if not ok:
        PROBLEMS.append(label)


def skip_dict(e):
    return isinstance(e, dict) and ("tie" in e or "hull" in e)


def mesh_json(m, edges):
    keys = ("latCell", "lonCell", "latVertex", "lonVertex", "verticesOnCell") + (("latEdge", "lonEdge", "angleEdge") if edges else ())
    return {k: getattr(m, k).tolist() for k in keys}


# kinds of a point's entry in the "<key>/k" array (see the docstring's Format)
K_NULL, K_HULL, K_TIE, K_CORNER, K_CAP, K_QUAD, K_QUAD_TIE, K_QUAD_ON_EDGE, K_TRI = range(9)


def encode_entries(entries):
    """One list of per-point entries -> (k int32 [n][1 + ints], f float64 [n][floats]), rows of zeros where an entry has no such number."""
    rows = []
    for e in entries:
        if e is None:
            rows.append((K_NULL, [], []))
        elif "q" in e:
            rows.append((K_QUAD_TIE if "tie" in e else K_QUAD_ON_EDGE if "on_edge" in e else K_QUAD, [e["q"]], [e["xi"], e["eta"]]))
        elif "cap" in e:
            rows.append((K_CAP, [e["cap"]], e["t"]))
        elif "col" in e:
            rows.append((K_TRI, e["col"], e["w"]))
        elif "corner" in e:
            rows.append((K_CORNER, [e["corner"]], []))
        else:
            rows.append((K_HULL if "hull" in e else K_TIE, [], []))
    ni, nf = max(len(r[1]) for r in rows), max(len(r[2]) for r in rows)
    k, f = np.zeros((len(rows), 1 + ni), np.int32), np.zeros((len(rows), nf), np.float64)
    for p, (kind, ints, floats) in enumerate(rows):
        k[p, 0] = kind
        k[p, 1:1 + len(ints)] = ints
        f[p, :len(floats)] = floats
    return k, f


def externalize(x, arrays, key):
    """The document with every list moved into `arrays` (by its path in the document) and replaced by {"@": path}."""
    if isinstance(x, dict):
        return {k: externalize(v, arrays, key + "/" + k if key else k) for k, v in x.items()}
    if not isinstance(x, list):
        return x
    if x and all(v is None or isinstance(v, dict) for v in x):
        if all(v is None or set(v) & {"q", "cap", "col", "corner", "hull", "tie"} for v in x):
            arrays[key + "/k"], arrays[key + "/f"] = encode_entries(x)
            return {"@": key}
        return [externalize(v, arrays, "%s/%d" % (key, i)) for i, v in enumerate(x)]      # the list of cases
    a = np.array(x)
    arrays[key] = a.astype(np.int32) if a.dtype.kind in "iu" else a.astype(np.float64)
    return {"@": key}


def write_npz(path, arrays):
    """An uncompressed .npz with nothing in it that changes from run to run (np.savez stamps the time of day on every member)."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), version=(1, 0))
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def regional_case(name, mesh_name, m, g):
    print("case %s: grid %d x %d, mesh %s (%d cells, %d vertices, %d edges)" % (name, g.nx, g.ny, mesh_name, m.nCells, m.nVertices, m.nEdges), flush=True)
    stag = {"center": (g.lon, g.lat), "edge1": (g.lon_u, g.lat_u), "edge2": (g.lon_v, g.lat_v)}
    exp = {"bilinear": {}, "nearest": {}, "angles": {}}
    pts = {loc: mesh_points(m, loc) for loc in LOCS}
    for sk, (lon, lat) in stag.items():
        S = [[xyz_from_deg(lon[j, i], lat[j, i]) for i in range(lon.shape[1])] for j in range(lon.shape[0])]
        flat = [v for row in S for v in row]
        exp["bilinear"][sk], exp["nearest"][sk] = {}, {}
        for loc in LOCS:
            exp["bilinear"][sk][loc] = quad_search(S, pts[loc])
            exp["nearest"][sk][loc] = nearest_search(flat, pts[loc])
            qualify("bilinear %s -> %s" % (sk, loc), exp["bilinear"][sk][loc], skip_dict)
            qualify("nearest  %s -> %s" % (sk, loc), exp["nearest"][sk][loc], lambda e: e == -1)
    exp["angles"]["cell"] = angles(g.proj, m.lonCell, m.latCell)
    exp["angles"]["vertex"] = angles(g.proj, m.lonVertex, m.latVertex)
    exp["angles"]["edge"] = angles(g.proj, m.lonEdge, m.latEdge, m.angleEdge)
    return {"name": name, "mesh": mesh_name, "nx": int(g.nx), "ny": int(g.ny),
            "lon": g.lon.ravel().tolist(), "lat": g.lat.ravel().tolist(), "lon_u": g.lon_u.ravel().tolist(), "lat_u": g.lat_u.ravel().tolist(),
            "lon_v": g.lon_v.ravel().tolist(), "lat_v": g.lat_v.ravel().tolist(), "expect": exp}


def periodic_case(name, layout, mesh_name, m, locs):
    import _periodic_layouts as PL
    lon, lat = PL.coords(layout)
    ny, nx = lat.shape
    print("case %s: layout %s %d x %d, mesh %s" % (name, layout, nx, ny, mesh_name), flush=True)
    S = [[xyz_from_deg(lon[j, i], lat[j, i]) for i in range(nx)] for j in range(ny)]
    exp = {}
    for loc in locs:
        exp[loc] = periodic_search(S, mesh_points(m, loc))
        qualify("periodic -> %s" % loc, exp[loc], skip_dict)
        kinds = [e.get("kind") for e in exp[loc] if e]
        caps = [e["cap"] // nx for e in exp[loc] if e and e.get("kind") == "cap"]
        print("      seam rows %d, cap rows %d at the row-0 end, %d at the other" % (kinds.count("seam"), caps.count(0), caps.count(1)), flush=True)
        if not (kinds.count("seam") and caps.count(0) and caps.count(1)):
            PROBLEMS.append("%s %s: no seam rows or no cap rows at one pole" % (name, loc))
    # the midpoints of four chords of each end row (the seam's included), as float64 longitudes / latitudes: ON the border between the
    # last quads and the cap.  A quad passes there (within the 1e-10 tolerance), so by the header the row is that quad's.
    Sf = np.array([[f3(S[j][i]) for i in range(nx)] for j in range(ny)])
    a = np.array([0, 1, nx // 2, nx - 1])
    mid = np.concatenate([Sf[ny - 1, a] + Sf[ny - 1, (a + 1) % nx], Sf[0, a] + Sf[0, (a + 1) % nx]])
    mid /= np.linalg.norm(mid, axis=1, keepdims=True)
    elat, elon = np.arcsin(mid[:, 2]), np.arctan2(mid[:, 1], mid[:, 0])
    on_edge = periodic_search(S, [xyz_from_rad(elon[i], elat[i]) for i in range(8)], literal=True)
    if not all(e and "on_edge" in e for e in on_edge):
        PROBLEMS.append("%s: a chord midpoint is not within 1e-9 of its quad's border" % name)
    return {"name": name, "layout": layout, "mesh": mesh_name, "nx": nx, "ny": ny, "lon": lon[0].tolist(), "lat": lat[:, 0].tolist(), "expect": exp,
            "on_edge": {"lon": elon.tolist(), "lat": elat.tolist(), "expect": on_edge}}


def mesh_pair_case(name, sname, src, dname, dst):
    print("case %s: %s (%d cells) -> %s (%d cells, %d vertices)" % (name, sname, src.nCells, dname, dst.nCells, dst.nVertices), flush=True)
    C = mesh_points(src, "cell")
    tris = dual_triangles(src)
    exp = {"bilinear0": {}, "bilinear1": {}, "nearest": {}}
    for loc in ("cell", "vertex"):
        P = C if (dst is src and loc == "cell") else mesh_points(dst, loc)
        for lt in (0, 1):
            exp["bilinear%d" % lt][loc] = tri_search(C, tris, P, lt)
            qualify("bilinear line type %d -> %s" % (lt, loc), exp["bilinear%d" % lt][loc], skip_dict, corner_ok=True)
        if dst is src and loc == "vertex":          # a Voronoi vertex is equidistant from its three cell centres: every point a tie
            continue
        exp["nearest"][loc] = nearest_search(C, P)
        qualify("nearest -> %s" % loc, exp["nearest"][loc], lambda e: e == -1)
    exp["conserve"], exp["frac"] = conserve_mesh(src, dst)
    full, empty = sum(abs(f - 1) < 1e-9 for f in exp["frac"]), sum(f == 0 for f in exp["frac"])
    print("    conservative: %d entries, %d cells wholly covered, %d empty rows" % (len(exp["conserve"]), full, empty), flush=True)
    if len(exp["conserve"]) < 100:
        PROBLEMS.append("%s: fewer than 100 conservative entries" % name)
    return {"name": name, "src": sname, "dst": dname, "expect": exp}


def write(stem, note, meshes, cases):
    """<stem>.json: names, sizes and where each list is; <stem>.npz: the lists themselves, float64 / int32."""
    out = sys.argv[1] if len(sys.argv) > 1 else HERE
    arrays = {}
    doc = externalize({"meshes": {k: mesh_json(m, edges) for k, (m, edges) in meshes.items()}, "cases": cases}, arrays, "")
    write_npz(os.path.join(out, stem + ".npz"), arrays)
    with open(os.path.join(out, stem + ".json"), "w") as f:
        json.dump(dict({"note": note, "arrays": stem + ".npz"}, **doc), f, indent=1)
        f.write("\n")
    for ext in (".json", ".npz"):
        size = os.path.getsize(os.path.join(out, stem + ext))
        print("wrote %s (%d bytes)" % (os.path.join(out, stem + ext), size))
        if size >= 500000:
            PROBLEMS.append("%s is %d bytes" % (stem + ext, size))


def build_meshes():
    """The meshes and grids of the cases, by name (tests/test_mesh_store_goldens.py rebuilds nothing: it reads the fixture)."""
    from mpassit_amd import synth, target_grid as tg
    lam = dict(ref_lat=38.5, ref_lon=-97.5, truelat1=38.5, truelat2=38.5, stand_lon=-97.5)
    g120 = tg.define_target_grid_params("lambert", 18, 14, dx=120000.0, dy=120000.0, **lam)
    g3 = tg.define_target_grid_params("lambert", 18, 14, dx=3000.0, dy=3000.0, **lam)
    # regional hexagon meshes LARGER than the grid (margin 0.08 of its width on every side): points outside it are null rows
    hex120 = synth.mesh_edges(synth.regional_mesh_for_lambert(g120.proj, 18, 14, 96, margin=0.08))
    hex3 = synth.mesh_edges(synth.regional_mesh_for_lambert(g3.proj, 18, 14, 96, margin=0.08))
    vor260 = synth.mesh_edges(synth.global_voronoi_mesh(260))
    # Mesh -> Mesh: a regional mesh wide enough (600-km cells) to hold some fifty points of a second global mesh
    g600 = tg.define_target_grid_params("lambert", 18, 14, dx=600000.0, dy=600000.0, **lam)
    hex600 = synth.mesh_edges(synth.regional_mesh_for_lambert(g600.proj, 18, 14, 120, margin=0.0))
    vor400 = synth.mesh_edges(synth.global_voronoi_mesh(400, seed=synth.SEED + 1))
    return g120, g3, hex120, hex3, vor260, hex600, vor400


def main():
    g120, g3, hex120, hex3, vor260, hex600, vor400 = build_meshes()
    note = "generated by tests/golden/make_mesh_store_goldens.py (mpmath, 50 digits, brute force); see its docstring"
    cases = [regional_case("lambert_120km", "hex120", hex120, g120), regional_case("lambert_3km", "hex3", hex3, g3)]
    write("mesh_store_hp", note, {"hex120": (hex120, True), "hex3": (hex3, True)}, cases)
    cases = [periodic_case("periodic_s2n", "s2n", "vor260", vor260, LOCS),
             periodic_case("periodic_n2s", "n2s", "vor260", vor260, ("cell", "vertex")),
             periodic_case("periodic_gauss_n2s", "gauss_n2s", "vor260", vor260, ("vertex", "edge")),
             mesh_pair_case("global_to_regional", "vor260", vor260, "hex600", hex600),
             mesh_pair_case("regional_to_global", "hex600", hex600, "vor400", vor400),
             mesh_pair_case("regional_self", "hex600", hex600, "hex600", hex600)]
    write("mesh_store_global_hp", note, {"vor260": (vor260, True), "hex600": (hex600, False), "vor400": (vor400, False)}, cases)
    if PROBLEMS:
        raise SystemExit("conditions broken: %s" % PROBLEMS)
    print("every case is inside the tie and count conditions")


if __name__ == "__main__":
    main()
