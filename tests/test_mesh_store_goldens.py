"""The float64 references of the Grid -> Mesh, periodic Grid -> Mesh and Mesh -> Mesh Stores and of the mesh rotation angles against
tests/golden/mesh_store_hp and mesh_store_global_hp (.json + .npz) -- the same Stores solved by brute force at 50 digits from the header's
statement of each rule (tests/golden/make_mesh_store_goldens.py: every point against every quad / cap triangle / dual triangle, every
cell pair clipped, Girard areas, the forward Lambert map differentiated; no search structure, no float64 geometry, none of the
restatements under tests/_*_ref.py).  tests/_to_mesh_ref.py, tests/_periodic_to_mesh_ref.py, tests/_mesh_conserve_ref.py, the oracle's
triangle search and target_grid.rotang_at were each other's only check; here each is held to an answer that shares no code with it, and
the mutants of the periodic reference are shown to fail it.  tests/test_mesh_store_goldens_gpu.py sends the same checkers to the library
through the C-ABI."""
import json
import os

import numpy as np
import pytest

from conftest import mesh_xyz
from test_store_goldens import SLIVER

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _decode(k, f):
    """The per-point entries of a "<key>/k", "<key>/f" pair of arrays (tests/golden/make_mesh_store_goldens.py: encode_entries) as dicts."""
    out = []
    for row, val in zip(k.tolist(), f.tolist()):
        kind = row[0]
        if kind == 0:
            out.append(None)
        elif kind in (1, 2):
            out.append({"hull": 1} if kind == 1 else {"tie": 1})
        elif kind == 3:
            out.append({"tie": 1, "corner": row[1]})
        elif kind == 4:
            out.append({"kind": "cap", "cap": row[1], "t": val[:3]})
        elif kind in (5, 6, 7):
            out.append(dict({"q": row[1], "xi": val[0], "eta": val[1]}, **({6: {"tie": 1}, 7: {"on_edge": 1}}.get(kind, {}))))
        else:
            assert kind == 8, kind
            out.append({"col": row[1:4], "w": val[:3]})
    return out


def _internalize(x, arrays):
    if isinstance(x, dict):
        if set(x) == {"@"}:
            key = x["@"]
            return _decode(arrays[key + "/k"], arrays[key + "/f"]) if key + "/k" in arrays else arrays[key].tolist()
        return {k: _internalize(v, arrays) for k, v in x.items()}
    return [_internalize(v, arrays) for v in x] if isinstance(x, list) else x


def _load(name):
    """A fixture: <name>.json says where each list is, <name>.npz holds them (float64 / int32)."""
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        doc = json.load(f)
    with np.load(os.path.join(GOLDEN, doc["arrays"])) as arrays:
        return _internalize(doc, arrays)


def _with_kind(entries, nx):
    for e in entries:
        if e and "q" in e:
            e["kind"] = "seam" if e["q"] % nx == nx - 1 else "quad"
    return entries


REGIONAL, GLOBAL = _load("mesh_store_hp"), _load("mesh_store_global_hp")
LOCS = ("cell", "vertex", "edge")          # MPG_MESHLOC_ELEMENT, _NODE, _EDGE = 0, 1, 2
STAGGERS = ("center", "edge1", "edge2")    # MPG_STAGGERLOC_CENTER, _EDGE1, _EDGE2 = 0, 1, 2
TIE_TOL = 3e-9                             # tests/test_store_goldens.py check_grid_to_grid: a point within 1e-9 of a border, either neighbour
ANGLE_TOL = 1e-14                          # cos / sin of the closed form in float64.  Measured: numpy mirror 6.1e-16, library 6.1e-16


# The bar of tests/test_store_goldens.py: the float64 latitude / longitude -> unit vector step limits agreement with the 50-digit answer
# to a few 1e-16 / h, h the smaller spacing of the two sides (radians; a mesh's: the median distance between neighbouring centres).
# Measured worst differences, float64 reference / library, each against the 50-digit answer (bar in brackets):
#   Grid -> Mesh bilinear    _to_mesh_ref 4.5e-14 / library 4.5e-14 at 120 km (2.1e-13); 1.7e-12 / 1.6e-12 at 3 km (8.5e-12)
#   periodic Grid -> Mesh    _periodic_to_mesh_ref 1.0e-14 / library 1.0e-14 (2e-13), the Gaussian grid; 4.8e-15 on the 15-degree grids
#   Mesh -> Mesh bilinear    oracle 8.2e-15 / library 8.2e-15, either line type (2e-13)
#   conservative Mesh -> Mesh  _mesh_conserve_ref 4.8e-15 (1.5e-14 under FRACAREA), dst fraction 2.2e-15 / library the same, 2.3e-15 (2e-13)
# No reference exceeds the bar, so the library is held to the same one.
def tol_for(h):
    return max(2e-13, 4e-15 / h)


def _mesh(d):
    from mpassit_amd import synth
    return synth.MpasMesh(np.array(d["latCell"]), np.array(d["lonCell"]), np.array(d["latVertex"]), np.array(d["lonVertex"]),
                          np.array(d["verticesOnCell"], np.int32), **{k: np.array(d[k]) for k in ("latEdge", "lonEdge", "angleEdge") if k in d})


def _chord(lon0, lat0, lon1, lat1):
    xyz = lambda lo, la: np.array([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)])   # noqa: E731
    return float(np.linalg.norm(xyz(lon0, lat0) - xyz(lon1, lat1)))


def mesh_spacing(m):
    """median distance from a cell centre to its nearest neighbour, radians"""
    x = np.stack([np.cos(m.latCell) * np.cos(m.lonCell), np.cos(m.latCell) * np.sin(m.lonCell), np.sin(m.latCell)], axis=1)
    d = np.linalg.norm(x[:, None, :] - x[None, :, :], axis=2)
    np.fill_diagonal(d, np.inf)
    return float(np.median(d.min(axis=1)))


_MESHES = {}


def mesh_of(name):
    """A mesh of the fixtures by name (each is stored once, in the file of the first family that uses it)."""
    if name not in _MESHES:
        _MESHES[name] = _mesh(next(doc["meshes"][name] for doc in (REGIONAL, GLOBAL) if name in doc["meshes"]))
    return _MESHES[name]


def mesh_lonlat(m, loc):
    return {"cell": (m.lonCell, m.latCell), "vertex": (m.lonVertex, m.latVertex), "edge": (m.lonEdge, m.latEdge)}[loc]


class RegionalCase:
    """A Lambert grid (CENTER, EDGE1, EDGE2 coordinates in degrees) and a regional mesh larger than it."""

    def __init__(self, c):
        self.name, self.nx, self.ny = c["name"], c["nx"], c["ny"]
        self.expect = c["expect"]
        self.mesh = mesh_of(c["mesh"])
        shapes = {"center": (self.ny, self.nx), "edge1": (self.ny, self.nx + 1), "edge2": (self.ny + 1, self.nx)}
        keys = {"center": ("lon", "lat"), "edge1": ("lon_u", "lat_u"), "edge2": ("lon_v", "lat_v")}
        self.coords = {s: (np.array(c[keys[s][0]]).reshape(shapes[s]), np.array(c[keys[s][1]]).reshape(shapes[s])) for s in STAGGERS}
        lon, lat = np.radians(self.coords["center"][0]), np.radians(self.coords["center"][1])
        self.dx = {"lambert_120km": 120000.0, "lambert_3km": 3000.0}[self.name]
        self.h = min(_chord(lon[0, 0], lat[0, 0], lon[0, 1], lat[0, 1]), mesh_spacing(self.mesh))

    def target(self):
        """The namelist the fixture's grid came from; its arrays are the fixture's bit for bit."""
        from mpassit_amd import target_grid as tg
        g = tg.define_target_grid_params("lambert", 18, 14, dx=self.dx, dy=self.dx, ref_lat=38.5, ref_lon=-97.5, truelat1=38.5, truelat2=38.5,
                                         stand_lon=-97.5)
        assert np.array_equal(g.lon, self.coords["center"][0]) and np.array_equal(g.lat_u, self.coords["edge1"][1])
        assert np.array_equal(g.lon_v, self.coords["edge2"][0])
        return g


class PeriodicCase:
    def __init__(self, c):
        self.name, self.layout, self.nx, self.ny = c["name"], c["layout"], c["nx"], c["ny"]
        self.expect = {loc: _with_kind(v, self.nx) for loc, v in c["expect"].items()}
        self.mesh = mesh_of(c["mesh"])
        self.lon = np.ascontiguousarray(np.broadcast_to(np.array(c["lon"])[None, :], (self.ny, self.nx)))
        self.lat = np.ascontiguousarray(np.broadcast_to(np.array(c["lat"])[:, None], (self.ny, self.nx)))
        self.on_edge = dict(c["on_edge"], expect=_with_kind(c["on_edge"]["expect"], self.nx))
        lo, la = np.radians(self.lon), np.radians(self.lat)
        j = self.ny // 2
        self.h = min(_chord(lo[j, 0], la[j, 0], lo[j, 1], la[j, 1]), _chord(lo[j, 0], la[j, 0], lo[j + 1, 0], la[j + 1, 0]), mesh_spacing(self.mesh))

    def locs(self):
        return [loc for loc in LOCS if loc in self.expect]


class PairCase:
    def __init__(self, c):
        self.name = c["name"]
        self.expect = dict(c["expect"], conserve=[(int(r), int(col), v) for r, col, v in c["expect"]["conserve"]])
        self.src, self.dst = mesh_of(c["src"]), mesh_of(c["dst"])
        self.h = min(mesh_spacing(self.src), mesh_spacing(self.dst))


def regional_cases():
    return [RegionalCase(c) for c in REGIONAL["cases"]]


def periodic_cases():
    return [PeriodicCase(c) for c in GLOBAL["cases"] if "layout" in c]


def pair_cases():
    return [PairCase(c) for c in GLOBAL["cases"] if "src" in c]


# ---- the shared checkers --------------------------------------------------------------------------------------------------------------
def quad_row(e, snx, periodic=False):
    """The header's row of a quad entry: columns A, B, C, D and weights (1-xi)(1-eta), xi (1-eta), xi eta, (1-xi) eta."""
    qnx = snx if periodic else snx - 1
    b, a = divmod(e["q"], qnx)
    a1 = (a + 1) % snx
    xi, eta = e["xi"], e["eta"]
    return [b * snx + a, b * snx + a1, (b + 1) * snx + a1, (b + 1) * snx + a], [(1 - xi) * (1 - eta), xi * (1 - eta), xi * eta, (1 - xi) * eta]


def _sparse(cols, vals):
    out = {}
    for c, v in zip(cols, vals):
        if c >= 0 and abs(v) > 1e-13:
            out[int(c)] = out.get(int(c), 0.0) + float(v)
    return out


def check_quads(case, stagger, loc, idx, w, floor=50):
    """idx / w [P][4] (slots A, B, C, D; -1 = unmapped) against the golden: the same mapped mask, the same four columns in the same
    slots, weights within tol_for; a point on the border of two quads may sit in either (TIE_TOL), a point on the hull either way."""
    exp = case.expect["bilinear"][stagger][loc]
    snx = case.coords[stagger][0].shape[1]
    assert len(exp) == idx.shape[0]
    worst, n = 0.0, 0
    for p, e in enumerate(exp):
        if e is None:
            assert idx[p, 0] < 0, "%s %s %s: point %d lies in no quad, yet is mapped to %s" % (case.name, stagger, loc, p, idx[p])
            assert not w[p].any()
            continue
        if "hull" in e:
            continue
        assert idx[p, 0] >= 0, "%s %s %s: point %d lies in quad %d, yet is unmapped" % (case.name, stagger, loc, p, e["q"])
        cols, vals = quad_row(e, snx)
        if "tie" in e:
            got, want = _sparse(idx[p], w[p]), _sparse(cols, vals)
            assert max(abs(want.get(k, 0.0) - got.get(k, 0.0)) for k in set(want) | set(got)) < TIE_TOL, (case.name, stagger, loc, p)
            continue
        assert list(idx[p]) == cols, "%s %s %s: point %d: columns %s, expected %s" % (case.name, stagger, loc, p, idx[p], cols)
        worst = max(worst, float(np.abs(w[p] - np.array(vals)).max()))
        n += 1
    assert n >= floor, (case.name, stagger, loc, n)
    assert worst < tol_for(case.h), (case.name, stagger, loc, worst, tol_for(case.h))
    return worst


def check_nearest(exp, idx, label):
    n = 0
    for p, e in enumerate(exp):
        if e >= 0:
            assert int(idx[p]) == e, "%s: point %d: nearest source %d, expected %d" % (label, p, idx[p], e)
            n += 1
    assert n >= 50, (label, n)


def periodic_row(e, nx, ny):
    """(columns ascending, weights, kind) of a periodic entry"""
    if e["kind"] == "cap":
        end, a = divmod(e["cap"], nx)
        tA, tB, tP = e["t"]
        wr = tP / nx
        v = np.full(nx, wr)
        v[a] = tA + wr
        v[(a + 1) % nx] = tB + wr
        return (ny - 1) * nx * end + np.arange(nx), v, "cap"
    cols, vals = quad_row(e, nx, periodic=True)
    order = np.argsort(cols, kind="stable")
    return np.array(cols)[order], np.array(vals)[order], e["kind"]


def row_kind(cols, nx):
    """The kind a CSR row shows: 0 entries null, nx entries a cap (nx == 4: a cap row holds one grid row), 4 a quad -- a seam quad holds
    columns 0 and nx - 1 of a row."""
    if len(cols) == 0:
        return None
    if len(cols) == nx and (nx != 4 or len(set(int(c) // nx for c in cols)) == 1):
        return "cap"
    assert len(cols) == 4, cols
    ci = sorted(int(c) % nx for c in cols)
    return "seam" if ci[0] == 0 and ci[-1] == nx - 1 and nx > 2 else "quad"


def check_periodic(case, exp, rowptr, col, val, pole_method=1, floor=50):
    """CSR rows against the golden's entries `exp`: the same mapped mask, the same row kind (quad rows of exactly 4 entries, cap rows of
    exactly nx, columns ascending), the same columns, weights within tol_for.  pole_method 0 (MPG_POLEMETHOD_NONE): the cap entries are
    empty rows.  -> (worst, rows compared, cap rows, seam rows, skipped)"""
    nx, ny = case.nx, case.ny
    assert rowptr.size - 1 == len(exp)
    worst, n, ncap, nseam, skipped = 0.0, 0, 0, 0, 0
    for p, e in enumerate(exp):
        c, v = col[rowptr[p]:rowptr[p + 1]], val[rowptr[p]:rowptr[p + 1]]
        if e is not None and "kind" not in e:          # {"tie": 1}: on a border
            skipped += 1
            continue
        if e is None or (e["kind"] == "cap" and pole_method == 0):
            assert c.size == 0, "%s: point %d has no quad%s, yet has a row %s" % (case.name, p, "" if e is None else " and caps are off", c)
            continue
        cols, vals, kind = periodic_row(e, nx, ny)
        assert c.size > 0, "%s: point %d lies in %s %s, yet its row is empty" % (case.name, p, kind, e.get("q", e.get("cap")))
        assert np.all(np.diff(c) > 0), "%s: point %d: columns do not ascend: %s" % (case.name, p, c)
        assert row_kind(c, nx) == kind and c.size == (nx if kind == "cap" else 4), "%s: point %d: a %s row expected, got %s" % (case.name, p, kind, c)
        assert np.array_equal(c, cols), "%s: point %d: columns %s, expected %s" % (case.name, p, c, cols)
        d = float(np.abs(v - vals).max())
        if "on_edge" in e:
            assert d < TIE_TOL, (case.name, p, d)
        else:
            worst = max(worst, d)
        n += 1
        ncap += kind == "cap"
        nseam += kind == "seam"
    assert n >= floor, (case.name, n)
    assert worst < tol_for(case.h), (case.name, worst, tol_for(case.h))
    return worst, n, ncap, nseam, skipped


def check_mesh_bilinear(case, key, loc, idx, w):
    """idx / w [P][3] (-1 = unmapped) against the golden of line type `key` ("bilinear0" / "bilinear1"): the same mapped mask, the same
    three cells, weights within tol_for; a point ON a cell centre of the source (src == dst) has weight 1 on that cell."""
    exp = case.expect[key][loc]
    assert len(exp) == idx.shape[0]
    worst, n = 0.0, 0
    for p, e in enumerate(exp):
        if e is None:
            assert idx[p, 0] < 0, "%s %s %s: point %d lies in no dual triangle, yet is mapped to %s" % (case.name, key, loc, p, idx[p])
            continue
        if "tie" in e:
            if "corner" in e:
                assert idx[p, 0] >= 0, (case.name, key, loc, p)
                got = _sparse(idx[p], w[p])
                worst = max(worst, max(abs(got.get(k, 0.0) - (1.0 if k == e["corner"] else 0.0)) for k in set(got) | {e["corner"]}))
                n += 1
            continue
        assert idx[p, 0] >= 0, "%s %s %s: point %d lies in triangle %s, yet is unmapped" % (case.name, key, loc, p, e["col"])
        order = np.argsort(idx[p])
        assert list(idx[p][order]) == e["col"], "%s %s %s: point %d: cells %s, expected %s" % (case.name, key, loc, p, idx[p][order], e["col"])
        worst = max(worst, float(np.abs(w[p][order] - np.array(e["w"])).max()))
        n += 1
    assert n >= 50, (case.name, key, loc, n)
    assert worst < tol_for(case.h), (case.name, key, loc, worst, tol_for(case.h))
    return worst


# The header's fan of spherical triangles (Van Oosterom-Strackee) and Girard's theorem are two formulas for the SAME spherical area, so they
# differ by rounding only: _mesh_conserve_ref is within 1.5e-14 of the Girard goldens on the 600-km / 1400-km meshes (measured above), well
# inside tol_for -- the bar stays tol_for, factor 1.
CONSERVE_FACTOR = 1.0


def conserve_tol(case):
    return CONSERVE_FACTOR * tol_for(case.h)


def check_mesh_conserve(case, rowptr, col, val, frac, norm=0):
    """CSR rows and dst fraction against the golden (Girard areas; the header's fan of spherical triangles is the same area by another
    formula).  norm 0 MPG_NORM_DSTAREA: w = I / area(d); 1 MPG_NORM_FRACAREA: the golden's w / frac.  Entries below SLIVER may exist on
    one side only."""
    gfrac = np.array(case.expect["frac"])
    want = {(r, c): (v if norm == 0 else v / gfrac[r]) for r, c, v in case.expect["conserve"]}
    got = {(int(r), int(c)): float(v) for r in range(rowptr.size - 1) for c, v in zip(col[rowptr[r]:rowptr[r + 1]], val[rowptr[r]:rowptr[r + 1]])}
    assert rowptr.size - 1 == gfrac.size
    worst, n = 0.0, 0
    for k, v in want.items():
        if k in got:
            worst = max(worst, abs(got[k] - v))
            n += 1
        else:
            assert v < SLIVER, "%s: overlap %s = %.3e is missing" % (case.name, k, v)
    for k, v in got.items():
        assert k in want or v < SLIVER, "%s: entry %s = %.3e overlaps nothing" % (case.name, k, v)
    for r in range(gfrac.size):
        assert np.all(np.diff(col[rowptr[r]:rowptr[r + 1]]) > 0), "%s: row %d: columns do not ascend" % (case.name, r)
        if gfrac[r] == 0.0:
            assert rowptr[r] == rowptr[r + 1] or val[rowptr[r]:rowptr[r + 1]].max() < SLIVER, "%s: row %d overlaps nothing" % (case.name, r)
    wf = float(np.abs(np.asarray(frac) - gfrac).max())
    assert n >= 100, (case.name, n)
    assert worst < conserve_tol(case) and wf < 4 * conserve_tol(case), (case.name, worst, wf, conserve_tol(case))   # frac: a sum of up to ~8 entries
    return worst, wf


def check_angles(exp, keys, got, label):
    worst = 0.0
    for k, g in zip(keys, got):
        assert len(exp[k]) == len(g) >= 50, (label, k)
        worst = max(worst, float(np.abs(np.asarray(g) - np.array(exp[k])).max()))
    assert worst < ANGLE_TOL, (label, worst)
    return worst


# ---- the float64 references -----------------------------------------------------------------------------------------------------------
def _xyz(o, lon_rad, lat_rad):
    return o.lonlat_deg_to_xyz(*o.mesh_coords_deg(lon_rad, lat_rad))


@pytest.mark.parametrize("case", regional_cases(), ids=lambda c: c.name)
def test_to_mesh_reference_equals_the_goldens(oracle, case):
    import _to_mesh_ref as TR
    o = oracle
    out = []
    for stagger in STAGGERS:
        lon, lat = case.coords[stagger]
        src = o.lonlat_deg_to_xyz(lon, lat).reshape(lat.shape + (3,))
        for loc in LOCS:
            pts = _xyz(o, *mesh_lonlat(case.mesh, loc))
            idx, w, _ = TR.to_mesh_bilinear(src, pts)
            out.append(check_quads(case, stagger, loc, idx, w))
            check_nearest(case.expect["nearest"][stagger][loc], o.nearest(src.reshape(-1, 3), pts), "%s %s %s" % (case.name, stagger, loc))
    print("%s: _to_mesh_ref vs 50 digits: worst %.1e (bar %.1e)" % (case.name, max(out), tol_for(case.h)))


def _periodic_ref(o, case, loc, **kw):
    import _periodic_to_mesh_ref as PR
    cen = o.lonlat_deg_to_xyz(case.lon, case.lat).reshape(case.ny, case.nx, 3)
    if loc == "on_edge":
        pts = _xyz(o, np.array(case.on_edge["lon"]), np.array(case.on_edge["lat"]))
    else:
        pts = _xyz(o, *mesh_lonlat(case.mesh, loc))
    return PR.periodic_to_mesh(o, cen, pts, **kw)


@pytest.mark.parametrize("pole_method", [1, 0], ids=["allavg", "none"])
@pytest.mark.parametrize("case", periodic_cases(), ids=lambda c: c.name)
def test_periodic_reference_equals_the_goldens(oracle, case, pole_method):
    for loc in case.locs():
        r = _periodic_ref(oracle, case, loc, pole_method=pole_method)
        worst, n, ncap, nseam, skipped = check_periodic(case, case.expect[loc], r["rowptr"], r["col"], r["val"], pole_method)
        kinds = {None: 0, "quad": 1, "seam": 1, "cap": 2}
        for p, e in enumerate(case.expect[loc]):
            if e is None or "kind" in e:
                want = 0 if e is None or (e["kind"] == "cap" and pole_method == 0) else kinds[e["kind"]]
                assert r["kind"][p] == want, (case.name, loc, p)
        print("%s %s pole method %d: _periodic_to_mesh_ref vs 50 digits: worst %.1e over %d rows (%d cap, %d seam, %d skipped)" % (
            case.name, loc, pole_method, worst, n, ncap, nseam, skipped))
    r = _periodic_ref(oracle, case, "on_edge", pole_method=pole_method)
    check_periodic(case, case.on_edge["expect"], r["rowptr"], r["col"], r["val"], pole_method, floor=8)


@pytest.mark.parametrize("mutation", ["seam_swap_bc", "cap_no_division", "caps_first", "caps_by_row_index"])
def test_mutants_of_the_periodic_reference_fail_the_goldens(oracle, mutation):
    """Each deliberately wrong variant of tests/_periodic_to_mesh_ref.py is caught: the seam quads' slots and the division of the pole
    node's weight by the mesh points, a cap tried before the quads by the points ON the chord between an end row's neighbours (a quad
    passes there, so the row is a quad row), the pole taken from the row number by the grids numbered north to south."""
    failed = []
    for case in periodic_cases():
        try:
            for loc in case.locs():
                r = _periodic_ref(oracle, case, loc, mutate=mutation)
                check_periodic(case, case.expect[loc], r["rowptr"], r["col"], r["val"])
            r = _periodic_ref(oracle, case, "on_edge", mutate=mutation)
            check_periodic(case, case.on_edge["expect"], r["rowptr"], r["col"], r["val"], floor=8)
        except AssertionError:
            failed.append(case.name)
    want = [c.name for c in periodic_cases() if mutation != "caps_by_row_index" or c.layout.endswith("n2s")]
    assert failed == want, (mutation, failed)


@pytest.mark.parametrize("case", pair_cases(), ids=lambda c: c.name)
def test_oracle_mesh_to_mesh_equals_the_goldens(oracle, case):
    o, src, dst = oracle, case.src, case.dst
    cxyz, _ = mesh_xyz(o, src)
    tri, _ = o.dual_triangles(src.verticesOnCell, src.nVertices, cxyz)
    out = []
    for loc in ("cell", "vertex"):
        pts = _xyz(o, *mesh_lonlat(dst, loc))
        for lt in (0, 1):
            idx, w = o.bilinear_weights(cxyz, tri, pts, linetype=lt)
            out.append(check_mesh_bilinear(case, "bilinear%d" % lt, loc, idx, w))
        if loc in case.expect["nearest"]:
            check_nearest(case.expect["nearest"][loc], o.nearest(cxyz, pts), "%s %s" % (case.name, loc))
    print("%s: oracle triangle search vs 50 digits: worst %.1e (bar %.1e)" % (case.name, max(out), tol_for(case.h)))


@pytest.mark.parametrize("case", pair_cases(), ids=lambda c: c.name)
def test_mesh_conserve_reference_equals_the_goldens(oracle, case):
    import _mesh_conserve_ref as CR
    a = CR.Answer(oracle, case.src, case.dst)
    for norm in (CR.NORM_DSTAREA, CR.NORM_FRACAREA):
        rowptr, col, val, frac = a.rows(norm)
        worst, wf = check_mesh_conserve(case, rowptr, col, val, frac, norm)
        print("%s norm %d: _mesh_conserve_ref vs 50 digits (Girard): weights %.1e, dst fraction %.1e (bar %.1e)" % (case.name, norm, worst, wf, conserve_tol(case)))


@pytest.mark.parametrize("case", regional_cases(), ids=lambda c: c.name)
def test_rotang_mirrors_equal_the_goldens(case):
    from mpassit_amd import target_grid as tg
    proj, m, exp = case.target().proj, case.mesh, case.expect["angles"]
    out = [check_angles(exp[loc], ("cosa", "sina"), tg.rotang_at(proj, np.degrees(mesh_lonlat(m, loc)[0])), "%s %s" % (case.name, loc)) for loc in LOCS]
    out.append(check_angles(exp["edge"], ("cn", "sn"), tg.edge_rotang_at(proj, np.degrees(m.lonEdge), m.angleEdge), case.name + " edges"))
    print("%s: rotang_at / edge_rotang_at vs the differentiated forward map at 50 digits: worst %.1e" % (case.name, max(out)))


def test_the_checkers_catch_a_wrong_slot_and_the_other_line_type(oracle):
    """What a kernel and its restatement could get wrong alike is caught: B and D exchanged in a quad row, the two line types taken
    for one another (they differ by O(h^2) of the triangle), a conservative row normalised the other way."""
    import _mesh_conserve_ref as CR
    import _to_mesh_ref as TR
    o, case = oracle, regional_cases()[0]
    lon, lat = case.coords["edge1"]
    src = o.lonlat_deg_to_xyz(lon, lat).reshape(lat.shape + (3,))
    idx, w, _ = TR.to_mesh_bilinear(src, _xyz(o, *mesh_lonlat(case.mesh, "edge")))
    check_quads(case, "edge1", "edge", idx, w)
    with pytest.raises(AssertionError):
        check_quads(case, "edge1", "edge", idx[:, [0, 3, 2, 1]], w[:, [0, 3, 2, 1]])
    with pytest.raises(AssertionError):
        check_quads(case, "edge1", "edge", idx, w[:, [0, 3, 2, 1]])
    pair = pair_cases()[0]
    cxyz, _ = mesh_xyz(o, pair.src)
    tri, _ = o.dual_triangles(pair.src.verticesOnCell, pair.src.nVertices, cxyz)
    pts = _xyz(o, *mesh_lonlat(pair.dst, "cell"))
    for lt in (0, 1):
        with pytest.raises(AssertionError):
            check_mesh_bilinear(pair, "bilinear%d" % (1 - lt), "cell", *o.bilinear_weights(cxyz, tri, pts, linetype=lt))
    r2g = pair_cases()[1]
    a = CR.Answer(o, r2g.src, r2g.dst)
    rowptr, col, val, frac = a.rows(CR.NORM_FRACAREA)
    with pytest.raises(AssertionError):
        check_mesh_conserve(r2g, rowptr, col, val, frac, 0)


def test_the_goldens_cover_what_they_claim():
    """Null rows (mesh points outside the grid) in the regional cases; seam rows and cap rows at BOTH poles in every periodic case and the
    points on an end row's chords; unmapped points, empty conservative rows, partly and wholly covered cells between the meshes; few
    ties."""
    for c in regional_cases():
        for stagger in STAGGERS:
            for loc in LOCS:
                exp = c.expect["bilinear"][stagger][loc]
                marked = sum(1 for e in exp if e and ("tie" in e or "hull" in e))
                assert sum(e is None for e in exp) >= 20 and sum(1 for e in exp if e and "q" in e) >= 50 and marked <= 0.02 * len(exp)
                assert sum(e < 0 for e in c.expect["nearest"][stagger][loc]) <= 0.02 * len(exp)
    layouts = set()
    for c in periodic_cases():
        layouts.add(c.layout)
        for loc in c.locs():
            exp = c.expect[loc]
            kinds = [e.get("kind") for e in exp if e]
            ends = [e["cap"] // c.nx for e in exp if e and e.get("kind") == "cap"]
            assert kinds.count("seam") >= 3 and ends.count(0) >= 1 and ends.count(1) >= 1 and kinds.count(None) <= 0.02 * len(exp), (c.name, loc)
        assert len(c.on_edge["expect"]) == 8 and all(e["kind"] in ("quad", "seam") and "on_edge" in e for e in c.on_edge["expect"])
        assert any(e["kind"] == "seam" for e in c.on_edge["expect"])
    assert {"s2n", "n2s"} <= layouts and any(k.startswith("gauss") for k in layouts)
    assert periodic_cases()[0].locs() == list(LOCS)
    by = {c.name: c for c in pair_cases()}
    assert set(by) == {"global_to_regional", "regional_to_global", "regional_self"}
    r2g = by["regional_to_global"]
    frac = np.array(r2g.expect["frac"])
    assert (frac == 0).sum() >= 100 and (np.abs(frac - 1) < 1e-9).sum() >= 5 and ((frac > 1e-3) & (frac < 0.999)).sum() >= 5
    assert sum(e is None for e in r2g.expect["bilinear0"]["cell"]) >= 100
    assert (np.abs(np.array(by["global_to_regional"].expect["frac"]) - 1) < 1e-9).all()
    self_ = by["regional_self"]
    assert sum(1 for e in self_.expect["bilinear0"]["cell"] if e and "corner" in e) >= 50
    assert all(r == c or v < SLIVER for r, c, v in self_.expect["conserve"])
    for c in pair_cases():
        assert len(c.expect["conserve"]) >= 100
        for key in ("bilinear0", "bilinear1"):
            for loc in ("cell", "vertex"):
                exp = c.expect[key][loc]
                assert sum(1 for e in exp if e and "tie" in e and "corner" not in e) <= 0.02 * len(exp), (c.name, key, loc)
