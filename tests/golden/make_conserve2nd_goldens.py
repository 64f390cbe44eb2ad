#!/usr/bin/env python3
"""50-digit goldens of the second-order conservative rule (include/mpassit_amd.h, "second-order conservative regridding", steps 1 to 6):
python tests/golden/make_conserve2nd_goldens.py writes conserve2nd_hp.npz (inputs, expected rows and intermediates, mutants) and
conserve2nd_hp.json (the cases, their branches, the margins, the measured figures) next to itself; a directory as the first argument
receives the files instead.  About ten seconds; a rerun gives the same bytes (compressed members in sorted order with a fixed time stamp; an
array whose bytes another array already has is stored once, "aliases" in the json).

The rule is evaluated by brute force in mpmath at 50 digits, straight from the header's text, and uses nothing of the mirror
(target_grid's _c2_*, conserve2nd_* and patch_* functions) nor of csrc: the triangle area is the exact 2 atan2(num, den) of the header's two
numbers -- NOT the half-angle steps and the series, so the golden judges that approximation too; N1 of a mesh cell comes from
verticesOnCell alone (the cells that share a vertex listed by exactly three cells), N1 of a grid cell is the shifted 3 x 3 window of the
CENTER stagger; the frame is the patch rule's about n = G_i; the clip is Sutherland-Hodgman by the destination polygon's sides in listed
counter-clockwise order, closing side last, normals a x (b - a), the 1e-15 |n| inside rule and the |b - a|^2 < 1e-24 rule applied at 50
digits as written.  Summation orders are not copied: they do not matter at 50 digits.  Inputs are float64 and stored: the polygons' unit
vectors and the cell centres (per side, each side once), verticesOnCell or the grid shape, the first-order pattern from the CPU references
(an input of the rule: tests/_conserve2nd_golden_cases.py first_order_pattern), the norm, the source mask.  Expected values are the
50-digit results rounded once: rowptr, col, val; per stored entry A_q and m_q; per source A_i, G_i, the pass flag; per stencil entry b
(sptr, scol, sb); per destination area(d).

Margins, asserted here and recorded in the json ("_margins"; conditions, not measurements).  No inside decision has |distance| / |n|
within a factor 1000 of 1e-15 on either side; no side length squared is within a factor 1000 of 1e-24; no stencil's det / (M00 M11) is
within a factor 4 of 2^-26; no A_q that the clamp or the > 0 tests decide lies in (0, 1e-20).  With them the golden's discrete decisions
are float64's too, so the tests demand equal patterns and equal pass flags.  The 1 x 5 grid's stencils are collinear up to the curvature
of a Lambert grid line: their det / (M00 M11) falls BELOW 2^-26 by the factor the json records, so every one of them fails (first order).

Cases (case_list below; each asserts the branch it is there for).  geodesic_mesh(6) onto a global Voronoi mesh, plain and with every 17th
source masked; a regional hex mesh to and from geodesic_mesh(6) under both norms; that mesh onto a 9 x 7 Lambert grid that overhangs it;
Lambert grids of 7 x 5, 2 x 2 and 1 x 5 cells onto that mesh; and the hex pair with the listed vertex order of every third cell reversed on
both sides (the rule turns it back, so the expectation is the unreversed pair's up to the last bits of area(d), whose fan starts at the
other end of the listing: the orientation rule seen alone).  The Voronoi
mesh has 120 cells and the hex mesh 204, not more: with geodesic_mesh(6)'s 362 stencils per source side the fixture is 430 KB as it is,
and no committed golden is larger than 492 KB.

Mutants, evaluated at the same 50 digits on the case where each bites (arrays m<k>/...): 1 the stencil (and its frame) about the stored cell
centre instead of G_i; 2 delta_q about G_i instead of M_i / A_i; 3 b_i = 0; 4 masked cells left in the stencils; 5 planar triangle areas
and moments instead of spherical ones.

Measured ("_measured", per case): the worst |mirror - golden| of val with the mirror (target_grid._conserve2nd_rows) run on the stored
inputs, and the worst change of the mirror's val when every stored unit vector is moved by a random last-bit change and renormalised.
The mirror is imported for these two figures only, after every expectation has been computed."""
import io
import json
import os
import sys
import zipfile

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
mpmath.mp.dps = 50
mpf = mpmath.mpf
ZERO = mpf(0)
MAX_PNTS = 32
DET_TOL = mpf(2) ** -26
INSIDE = mpf(10) ** -15
SHORT = mpf(10) ** -24
TINY_AREA = mpf(10) ** -20
NORM_DSTAREA, NORM_FRACAREA = 0, 1
MUTANTS = {1: "the stencil about the stored cell centre instead of G_i", 2: "delta_q about G_i instead of M_i / A_i", 3: "b_i = 0",
           4: "masked cells left in the stencils", 5: "planar triangle areas and moments"}
RECHECK = ("grid7x5 to hex", 20)        # tests/test_conserve2nd_goldens.py re-evaluates that many rows of this case


def vec(x):
    return [mpf(float(x[0])), mpf(float(x[1])), mpf(float(x[2]))]


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def tri_sphere(a, b, c):
    """the signed area of the spherical triangle: 2 atan2 of the header's two numbers"""
    num = dot(a, cross(sub(b, a), sub(c, a)))
    den = 1 + dot(a, b) + dot(b, c) + dot(c, a)
    assert den > 0                                       # (the header's den <= 0 branch: a triangle of half the sphere; no case has one)
    return 2 * mpmath.atan2(num, den)


def tri_plane(a, b, c):
    """mutant 5: the area of the flat triangle, signed as seen from outside"""
    n = cross(sub(b, a), sub(c, a))
    s = mpmath.sqrt(dot(n, n)) / 2
    return s if dot(n, a) >= 0 else -s


def fan(poly, tri=tri_sphere):
    """(signed area, moment) of the fan from slot 0"""
    area, m = ZERO, [ZERO, ZERO, ZERO]
    for t in range(1, len(poly) - 1):
        a = tri(poly[0], poly[t], poly[t + 1])
        area += a
        for k in range(3):
            m[k] += a * (poly[0][k] + poly[t][k] + poly[t + 1][k]) / 3
    return area, m


class Margins:
    """how close the discrete decisions of a case come to their thresholds"""

    def __init__(self):
        self.inside_above, self.inside_below = mpmath.inf, ZERO        # smallest |d| / |n| above 1e-15, largest at or below it
        self.side_min = mpmath.inf
        self.det_above, self.det_below = mpmath.inf, ZERO               # det / (M00 M11) of the stencils with two members or more
        self.area_small = mpmath.inf                                    # smallest positive piece area
        self.sides_dropped = 0

    def inside(self, r):
        if r > INSIDE:
            self.inside_above = min(self.inside_above, r)
        else:
            self.inside_below = max(self.inside_below, r)

    def check(self, name):
        assert self.inside_above > 1000 * INSIDE and self.inside_below < INSIDE / 1000, (name, "inside", self.inside_above, self.inside_below)
        assert self.side_min > 1000 * SHORT, (name, "side", self.side_min)
        assert self.det_above > 4 * DET_TOL and self.det_below < DET_TOL / 4, (name, "det", self.det_above, self.det_below)
        assert not self.area_small < TINY_AREA, (name, "area", self.area_small)

    def record(self):
        f = lambda x: None if x == mpmath.inf else float(x)  # noqa: E731
        return {"inside_smallest_above_1e-15": f(self.inside_above), "inside_largest_at_or_below_1e-15": f(self.inside_below),
                "side_squared_smallest": f(self.side_min), "det_ratio_smallest_passing": f(self.det_above),
                "det_ratio_largest_failing": f(self.det_below), "piece_area_smallest_positive": f(self.area_small)}


def clip(subject, clipper, mg):
    """the subject polygon cut by the sides of the clip polygon in order (both counter-clockwise), the closing side last"""
    poly = subject
    for e in range(len(clipper)):
        if len(poly) < 3:
            break
        a, b = clipper[e], clipper[(e + 1) % len(clipper)]
        side = sub(b, a)
        s2 = dot(side, side)
        mg.side_min = min(mg.side_min, s2)
        if s2 < SHORT:
            mg.sides_dropped += 1
            continue
        n = cross(a, side)
        ln = mpmath.sqrt(dot(n, n))
        d = [dot(n, x) for x in poly]
        for x in d:
            mg.inside(abs(x) / ln)
        ins = [x >= -INSIDE * ln for x in d]
        out = []
        for i in range(len(poly)):
            j = (i + 1) % len(poly)
            if ins[i]:
                out.append(poly[i])
            if ins[i] != ins[j]:                         # where the side from i to j meets the plane, on the side's own arc
                x = [poly[i][k] * d[j] - poly[j][k] * d[i] for k in range(3)]
                r = mpmath.sqrt(dot(x, x))
                if d[j] - d[i] < 0:
                    r = -r
                out.append([v / r for v in x])
        poly = out
    return poly


def frame(n):
    """the patch rule's frame about the unit vector n"""
    ax = min(range(3), key=lambda k: (abs(n[k]), k))
    a = [mpf(1) if k == ax else ZERO for k in range(3)]
    s = dot(a, n)
    t = [a[k] - s * n[k] for k in range(3)]
    r = mpmath.sqrt(dot(t, t))
    e1 = [v / r for v in t]
    return e1, cross(n, e1)


def ring1_mesh(voc):
    """N1 of every cell from verticesOnCell alone: the cell and the cells that share one of its vertices, counting only vertices listed by
    exactly three cells"""
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


class Side:
    """one side's cells at 50 digits: the polygons in listed order and counter-clockwise, the centres, N1"""

    def __init__(self, arrays):
        self.centre = [vec(x) for x in arrays["cell_xyz"]]
        if "voc" in arrays:
            v = [vec(x) for x in arrays["vert_xyz"]]
            self.listed = [[v[int(k) - 1] for k in row if k > 0] for row in arrays["voc"]]
            self.n1 = ring1_mesh(arrays["voc"])
        else:
            nx, ny = (int(k) for k in arrays["shape"])
            c = [vec(x) for x in arrays["corner_xyz"]]
            at = lambda i, j: c[j * (nx + 1) + i]  # noqa: E731
            self.listed = [[at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)] for j in range(ny) for i in range(nx)]
            self.n1 = ring1_grid(nx, ny)
        self._fan, self._ccw, self._G = {}, {}, {}

    def fan_listed(self, c):
        if c not in self._fan:
            self._fan[c] = fan(self.listed[c])[0]
        return self._fan[c]

    def reversed(self, c):
        return self.fan_listed(c) < 0

    def ccw(self, c):
        return self.listed[c][::-1] if self.reversed(c) else self.listed[c]

    def G(self, c):
        """the geometric centroid: the unit vector of the counter-clockwise polygon's own fan moment"""
        if c not in self._G:
            g = self.centre[c]
            if len(self.listed[c]) >= 3:
                m = fan(self.ccw(c))[1]
                r = mpmath.sqrt(dot(m, m))
                if r > 0:
                    g = [v / r for v in m]
            self._G[c] = g
        return self._G[c]


class Geometry:
    """the clipped polygons of a pair of sides, shared by every case (norm, mask, mutant) on that pair"""

    def __init__(self, src, dst):
        self.src, self.dst, self.mg = src, dst, Margins()
        self._poly, self._piece = {}, {}

    def poly(self, j, i):
        if (j, i) not in self._poly:
            self._poly[(j, i)] = clip(self.src.ccw(i), self.dst.ccw(j), self.mg)
        return self._poly[(j, i)]

    def piece(self, j, i, planar=False):
        """(A_q, m_q)"""
        key = (j, i, planar)
        if key not in self._piece:
            p = self.poly(j, i)
            if len(p) < 3:
                self._piece[key] = (ZERO, [ZERO, ZERO, ZERO])
            else:
                a, m = fan(p, tri_plane if planar else tri_sphere)
                if a > 0 and not planar:
                    self.mg.area_small = min(self.mg.area_small, a)
                self._piece[key] = (a if a > 0 else ZERO, m)
        return self._piece[key]


class Rule:
    """steps 2 to 6 on one first-order pattern; everything on demand, so a few rows can be evaluated alone"""

    def __init__(self, geo, rowptr, col, norm, mask=None, mutant=0):
        self.geo, self.src, self.dst = geo, geo.src, geo.dst
        self.rowptr, self.col, self.norm, self.mutant = [int(v) for v in rowptr], [int(v) for v in col], norm, mutant
        self.nS, self.nD = len(self.src.listed), len(self.rowptr) - 1
        self.mask = [False] * self.nS if mask is None else [bool(v) for v in mask]
        self.by_src = {}
        for j in range(self.nD):
            for q in range(self.rowptr[j], self.rowptr[j + 1]):
                self.by_src.setdefault(self.col[q], []).append(j)
        self._cell, self._stencil = {}, {}

    def origin(self, i):
        """the point the stencil of cell i is built about"""
        return self.src.centre[i] if self.mutant == 1 else self.src.G(i)

    def piece(self, j, i):
        return self.geo.piece(j, i, planar=self.mutant == 5)

    def cell(self, i):
        """(A_i, M_i, e1, e2)"""
        if i not in self._cell:
            A, M = ZERO, [ZERO, ZERO, ZERO]
            for j in self.by_src.get(i, []):
                a, m = self.piece(j, i)
                A += a
                M = [M[k] + m[k] for k in range(3)]
            self._cell[i] = (A, M) + frame(self.origin(i))
        return self._cell[i]

    def stencil(self, i):
        """(passes, [(id, bx, by)] ascending, det / (M00 M11) or None)"""
        if i not in self._stencil:
            n1 = self.src.n1[i]
            S = [k for k in n1 if k != i and (self.mutant == 4 or not self.mask[k])]
            ok, ratio, ent = len(S) >= 2 and len(n1) <= MAX_PNTS and not self.mask[i], None, [(i, ZERO, ZERO)]
            if ok:
                _, _, e1, e2 = self.cell(i)
                o = self.origin(i)
                d = [(dot(sub(self.origin(k), o), e1), dot(sub(self.origin(k), o), e2)) for k in S]
                m00, m01, m11 = sum(x * x for x, _ in d), sum(x * y for x, y in d), sum(y * y for _, y in d)
                det = m00 * m11 - m01 * m01
                ratio = det / (m00 * m11)
                if not self.mutant:
                    mg = self.geo.mg
                    if ratio > DET_TOL:
                        mg.det_above = min(mg.det_above, ratio)
                    else:
                        mg.det_below = max(mg.det_below, ratio)
                ok = det > DET_TOL * (m00 * m11)
                if ok:
                    b = [((m11 * x - m01 * y) / det, (m00 * y - m01 * x) / det) for x, y in d]
                    own = (ZERO, ZERO) if self.mutant == 3 else (-sum(x for x, _ in b), -sum(y for _, y in b))
                    ent = sorted([(k, bx, by) for k, (bx, by) in zip(S, b)] + [(i,) + own])
            self._stencil[i] = (ok, ent, ratio)
        return self._stencil[i]

    def area_d(self, j):
        return abs(self.dst.fan_listed(j)) if len(self.dst.listed[j]) >= 3 else ZERO

    def row(self, j):
        """[(column, value)] ascending"""
        ent = [(self.col[q], self.piece(j, self.col[q])) for q in range(self.rowptr[j], self.rowptr[j + 1])]
        div = self.area_d(j) if self.norm == NORM_DSTAREA else sum(a for _, (a, _) in ent)
        acc = {}
        for i, (a, m) in ent:
            w = a / div if div > 0 else ZERO
            Ai, Mi, e1, e2 = self.cell(i)
            dx = dy = ZERO
            if a > 0 and Ai > 0:
                about = self.src.G(i) if self.mutant == 2 else [Mi[k] / Ai for k in range(3)]
                dq = [m[k] / a - about[k] for k in range(3)]
                dx, dy = dot(dq, e1), dot(dq, e2)
            for e, bx, by in self.stencil(i)[1]:
                g = dx * bx + dy * by
                acc[e] = acc.get(e, ZERO) + w * ((1 + g) if e == i else g)
        return sorted(acc.items())

    def rows(self, which=None):
        rowptr, col, val = [0], [], []
        for j in (range(self.nD) if which is None else which):
            for e, v in self.row(j):
                col.append(e)
                val.append(float(v))
            rowptr.append(len(col))
        return np.array(rowptr, np.int64), np.array(col, np.int32), np.array(val, np.float64)

    def intermediates(self):
        """every stored intermediate, rounded once"""
        f3 = lambda v: [float(x) for x in v]  # noqa: E731
        Aq, mq = [], []
        for j in range(self.nD):
            for q in range(self.rowptr[j], self.rowptr[j + 1]):
                a, m = self.piece(j, self.col[q])
                Aq.append(float(a))
                mq.append(f3(m))
        sptr, scol, sb, ok = [0], [], [], []
        for i in range(self.nS):
            p, ent, _ = self.stencil(i)
            ok.append(p)
            for k, bx, by in ent:
                scol.append(k)
                sb.append([float(bx), float(by)])
            sptr.append(len(scol))
        return {"Aq": np.array(Aq, np.float64), "mq": np.array(mq, np.float64).reshape(-1, 3),
                "Ai": np.array([float(self.cell(i)[0]) for i in range(self.nS)]), "G": np.array([f3(self.src.G(i)) for i in range(self.nS)]),
                "pass": np.array(ok, np.uint8), "sptr": np.array(sptr, np.int32), "scol": np.array(scol, np.int32),
                "sb": np.array(sb, np.float64).reshape(-1, 2), "area_d": np.array([float(self.area_d(j)) for j in range(self.nD)])}


def write_npz(path, arrays):
    """a compressed .npz with nothing in it that changes from run to run (np.savez stamps the time of day on every member)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), version=(1, 0))
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def case_list():
    import _conserve2nd_golden_cases as GC
    D, F = NORM_DSTAREA, NORM_FRACAREA
    g = GC.grid_spec
    return [  # name, source, destination, norm, masked, what it reaches
        ("geo6 to vor", GC.GEO6, GC.VOR, D, False, "geodesic_mesh(6) -> a global Voronoi mesh: pentagons, every source fully covered"),
        ("geo6 to vor masked", GC.GEO6, GC.VOR, D, True, "the same pair, every 17th source masked, the ENTRY rule's pattern: masked neighbours "
         "leave stencils, a masked cell keeps one entry"),
        ("hex to geo6 dstarea", GC.HEX, GC.GEO6, D, False, "a regional hex mesh -> geodesic_mesh(6): empty rows, long rows"),
        ("hex to geo6 fracarea", GC.HEX, GC.GEO6, F, False, "the same under FRACAREA: partly covered destination cells"),
        ("geo6 to hex dstarea", GC.GEO6, GC.HEX, D, False, "geodesic_mesh(6) -> the hex mesh: partly covered source cells"),
        ("geo6 to hex fracarea", GC.GEO6, GC.HEX, F, False, "the same under FRACAREA"),
        ("hex to grid9x7", GC.HEX, g(9, 7), D, False, "Mesh -> Grid: the hex mesh -> the 9 x 7 cells of a Lambert grid that overhangs it: rim rows"),
        ("grid7x5 to hex", g(7, 5), GC.HEX, D, False, "Grid -> Mesh: corner polygons, shifted windows at the border"),
        ("grid2x2 to hex", g(2, 2), GC.HEX, F, False, "Grid -> Mesh from four cells: |S| = 3"),
        ("grid1x5 to hex", g(1, 5), GC.HEX, D, False, "Grid -> Mesh from a 1 x 5 grid: collinear stencils"),
        ("reversed hex to geo6", GC.HEX_REV, GC.GEO6_REV, D, False, "the listed vertex order of every third cell reversed, on both sides: the "
         "orientation rule"),
    ]


MUTANT_CASE = {1: "hex to geo6 dstarea", 2: "geo6 to hex dstarea", 3: "hex to geo6 dstarea", 4: "geo6 to vor masked", 5: "hex to geo6 dstarea"}


class Problem:
    """the sides, geometries and rules of the cases, built on demand: main() evaluates everything, the test a few rows"""

    def __init__(self, o):
        import _conserve2nd_golden_cases as GC
        self.o, self.GC = o, GC
        self.cases = {c[0]: c for c in case_list()}
        self._arrays, self._side, self._geo, self._pattern = {}, {}, {}, {}

    @staticmethod
    def side_name(spec):
        if "grid" in spec:
            return "grid%dx%d" % tuple(spec["grid"])
        return {"geodesic": "geo6", "voronoi": "vor", "hex": "hex"}[spec["mesh"]] + ("_reversed" if spec.get("reverse_every") else "")

    def arrays(self, spec):
        k = self.side_name(spec)
        if k not in self._arrays:
            self._arrays[k] = self.GC.side_arrays(self.o, spec)
        return self._arrays[k]

    def side(self, spec):
        k = self.side_name(spec)
        if k not in self._side:
            self._side[k] = Side(self.arrays(spec))
        return self._side[k]

    def geometry(self, s, d):
        k = (self.side_name(s), self.side_name(d))
        if k not in self._geo:
            self._geo[k] = Geometry(self.side(s), self.side(d))
        return self._geo[k]

    def inputs(self, name):
        """(rowptr, col, mask or None) of a case: the reference's pattern, after the ENTRY rule where the case is masked"""
        if name not in self._pattern:
            _, s, d, norm, masked, _ = self.cases[name]
            rp, col = self.GC.first_order_pattern(self.o, s, d, norm)
            sm = None
            if masked:
                sm = self.GC.source_mask(self.arrays(s)["cell_xyz"].shape[0])
                rp, col = self.GC.entry_rule(rp, col, sm)
            self._pattern[name] = (np.asarray(rp, np.int64), np.asarray(col, np.int32), sm)
        return self._pattern[name]

    def rule(self, name, mutant=0):
        _, s, d, norm, _, _ = self.cases[name]
        rp, col, sm = self.inputs(name)
        return Rule(self.geometry(s, d), rp, col, norm, sm, mutant)


def recheck_rows(in_rowptr, n):
    """n rows spread evenly over the rows that hold an entry"""
    full = np.flatnonzero(np.diff(in_rowptr) > 0)
    return [int(j) for j in full[np.linspace(0, full.size - 1, n).astype(np.int64)]]


def main():
    import _conserve2nd_golden_cases as GC
    from oracle import oracle as o
    o.build()
    out_dir = sys.argv[1] if len(sys.argv) > 1 else HERE
    problem = Problem(o)
    arrays, doc = {}, {"note": "generated by tests/golden/make_conserve2nd_goldens.py (mpmath, 50 digits, brute force); see its docstring",
                       "arrays": "conserve2nd_hp.npz", "sides": {}, "cases": {}, "_measured": {}, "_mutants": {}, "_margins": {},
                       "recheck": {"case": RECHECK[0], "rows": RECHECK[1]}}
    expected, reached = {}, {}
    for index, (name, s, d, norm, masked, what) in enumerate(case_list()):
        for spec in (s, d):
            k = problem.side_name(spec)
            if k not in doc["sides"]:
                doc["sides"][k] = spec
                arrays.update({k + "/" + key: v for key, v in problem.arrays(spec).items()})
        r = problem.rule(name)
        rp, col, sm = problem.inputs(name)
        rowptr, ocol, val = r.rows()
        mid = r.intermediates()
        expected[name] = (rowptr, ocol, val)
        src, dst = r.src, r.dst
        n_pass = int(mid["pass"].sum())
        stats = [int(col.size), n_pass, r.nS - n_pass, int(mid["scol"].size), int(np.diff(rowptr).max())]
        area_s = np.array([float(abs(src.fan_listed(i))) for i in range(r.nS)])
        covered = np.abs(mid["Ai"] - area_s) <= 1e-9 * area_s
        reached[name] = br = {
            "source_polygon_sizes": sorted(set(len(p) for p in src.listed)), "sources_fully_covered": int(covered.sum()),
            "sources_partly_covered": int(((mid["Ai"] > 0) & ~covered).sum()), "sources_without_a_piece": int((mid["Ai"] == 0).sum()),
            "empty_rows": int((np.diff(rp) == 0).sum()), "stencil_sizes": sorted(set(int(v) - 1 for v in np.diff(mid["sptr"]))),
            "reversed_sources": sum(src.reversed(i) for i in range(r.nS)), "reversed_destinations": sum(dst.reversed(j) for j in range(r.nD)),
            "sides_dropped": r.geo.mg.sides_dropped, "negative_weights": int((val < 0).sum())}
        if masked:
            br["masked_sources"] = int(sm.sum())
            br["stencils_that_lost_a_masked_neighbour"] = sum(1 for i in range(r.nS) if not sm[i] and any(sm[k] for k in src.n1[i]))
            assert all(mid["sptr"][i + 1] - mid["sptr"][i] == 1 and not mid["pass"][i] for i in np.flatnonzero(sm)), "a masked cell keeps one entry"
        if "grid" in s:
            nx, ny = s["grid"]
            br["shifted_windows"] = sum(1 for i in range(r.nS) if i % nx in (0, nx - 1) or i // nx in (0, ny - 1))
        pre = "c%d/" % index
        arrays.update({pre + "in_rowptr": rp.astype(np.int32), pre + "in_col": col, pre + "rowptr": rowptr.astype(np.int32), pre + "col": ocol,
                       pre + "val": val})
        arrays.update({pre + k: v for k, v in mid.items()})
        if masked:
            arrays[pre + "src_mask"] = sm
        doc["cases"][name] = {"index": index, "what": what, "src_side": problem.side_name(s), "dst_side": problem.side_name(d), "norm": norm,
                              "masked": masked, "n_src": r.nS, "n_dst": r.nD, "nnz_in": int(col.size), "nnz": int(ocol.size), "stats": stats,
                              "largest_cell_area": float(max(area_s.max(), mid["area_d"].max())), "reached": br}
        assert np.abs(val).max() < 10.0, "the weights are O(1)"
        print("%-22s %4d -> %4d cells, %5d pieces, %6d entries, stats %s\n    %s" % (name, r.nS, r.nD, col.size, ocol.size, stats, br), flush=True)
    # margins: per pair of sides, asserted
    for (ks, kd), geo in problem._geo.items():
        geo.mg.check(ks + " -> " + kd)
        doc["_margins"]["%s -> %s" % (ks, kd)] = geo.mg.record()
        print("margins %-28s %s" % (ks + " -> " + kd, geo.mg.record()), flush=True)
    # every branch occurs
    R = reached
    assert 5 in R["geo6 to vor"]["source_polygon_sizes"] and R["geo6 to vor"]["sources_fully_covered"] == doc["cases"]["geo6 to vor"]["n_src"]
    assert R["geo6 to vor masked"]["stencils_that_lost_a_masked_neighbour"] > 0 and R["geo6 to vor masked"]["masked_sources"] > 0
    for n in ("geo6 to hex dstarea", "geo6 to hex fracarea"):
        assert R[n]["sources_partly_covered"] > 0 and R[n]["sources_without_a_piece"] > 0
    assert R["hex to geo6 dstarea"]["empty_rows"] > 0
    a, b = expected["hex to geo6 dstarea"], expected["hex to geo6 fracarea"]          # partly covered destination cells: the divisors differ
    assert np.array_equal(a[1], b[1]) and np.abs(a[2] - b[2]).max() > 1e-3, "FRACAREA differs from DSTAREA"
    a, b = expected["geo6 to hex dstarea"], expected["geo6 to hex fracarea"]          # every destination cell wholly covered: they agree
    assert np.array_equal(a[1], b[1]) and np.abs(a[2] - b[2]).max() < 1e-12
    rim = arrays["c%d/Aq" % doc["cases"]["hex to grid9x7"]["index"]]
    in_rp = arrays["c%d/in_rowptr" % doc["cases"]["hex to grid9x7"]["index"]]
    cover = np.add.reduceat(np.append(rim, 0.0), in_rp[:-1])[:in_rp.size - 1] * (np.diff(in_rp) > 0)
    partly = int(((cover > 0) & (cover < 0.999 * arrays["c%d/area_d" % doc["cases"]["hex to grid9x7"]["index"]])).sum())
    R["hex to grid9x7"]["rim_rows"] = partly
    assert partly > 0, "rim rows"
    assert R["grid7x5 to hex"]["shifted_windows"] > 0 and R["grid7x5 to hex"]["stencil_sizes"] == [8]
    assert R["grid2x2 to hex"]["stencil_sizes"] == [3] and doc["cases"]["grid2x2 to hex"]["stats"][1] == 4
    assert doc["cases"]["grid1x5 to hex"]["stats"][1] == 0 and R["grid1x5 to hex"]["stencil_sizes"] == [0], "the collinear stencils all fail"
    assert R["reversed hex to geo6"]["reversed_sources"] > 0 and R["reversed hex to geo6"]["reversed_destinations"] > 0
    assert not any(R[n]["reversed_sources"] or R[n]["reversed_destinations"] for n in R if not n.startswith("reversed"))
    # the mutants, each on the case where it bites
    for k in sorted(MUTANTS):
        name = MUTANT_CASE[k]
        rowptr, col, val = problem.rule(name, mutant=k).rows()
        miss = GC.union_difference((rowptr, col, val), expected[name])[0]
        arrays.update({"m%d/rowptr" % k: rowptr.astype(np.int32), "m%d/col" % k: col, "m%d/val" % k: val})
        doc["_mutants"][str(k)] = {"what": MUTANTS[k], "case": name, "worst_difference_from_the_golden": miss}
        print("mutant %d (%s) on %s: worst difference %.3e" % (k, MUTANTS[k], name, miss), flush=True)
    # the measured figures, with the mirror: after everything above
    from mpassit_amd import target_grid as tg
    for name, m in doc["cases"].items():
        _, sspec, dspec, _, _, _ = problem.cases[name]
        c = {k[len("c%d/" % m["index"]):]: v for k, v in arrays.items() if k.startswith("c%d/" % m["index"])}
        c.update(meta=m, src=problem.arrays(sspec), dst=problem.arrays(dspec))
        doc["_measured"][name] = GC.measure(o, tg, c)
        print("measured %-22s %s" % (name, doc["_measured"][name]), flush=True)
    # an array with the bytes of one already stored (the FRACAREA twin's intermediates, a reversed side's vectors, the stencils of a source
    # side that several cases share) is stored once: "aliases" names the copy it stands for
    seen, doc["aliases"] = {}, {}
    for k in sorted(arrays):
        a = np.ascontiguousarray(arrays[k])
        h = (a.dtype.str, a.shape, a.tobytes())
        if h in seen:
            doc["aliases"][k] = seen[h]
            del arrays[k]
        else:
            seen[h] = k
    write_npz(os.path.join(out_dir, "conserve2nd_hp.npz"), arrays)
    with open(os.path.join(out_dir, "conserve2nd_hp.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    for ext in (".npz", ".json"):
        size = os.path.getsize(os.path.join(out_dir, "conserve2nd_hp" + ext))
        print("wrote conserve2nd_hp%s (%d bytes)" % (ext, size))
        assert size <= 492 * 1024, "larger than the largest golden already committed"


if __name__ == "__main__":
    main()
