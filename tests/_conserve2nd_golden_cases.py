"""What tests/golden/make_conserve2nd_goldens.py and the two tests of its fixture share, and nothing of the rule: the cases' meshes and
grids from their generator parameters (the "spec" dictionaries of conserve2nd_hp.json), their float64 unit vectors, the first-order
patterns from the CPU references, and the fixture's reader.  No mpmath here: the GPU test imports this module alone."""
import dataclasses
import functools
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LAMBERT = dict(ref_lat=38.5, ref_lon=-97.5, truelat1=38.5, truelat2=38.5, stand_lon=-97.5)
NORM_DSTAREA, NORM_FRACAREA = 0, 1
MASK_EVERY = 17

GEO6 = {"mesh": "geodesic", "freq": 6}
VOR = {"mesh": "voronoi", "cells": 120, "seed": 303}
HEX = {"mesh": "hex", "points": [8, 6], "dx": 300000.0, "cells": 200, "seed": 7}      # under the 7 x 5 cells of the 300-km Lambert grid
GEO6_REV = dict(GEO6, reverse_every=3)
HEX_REV = dict(HEX, reverse_every=3)


def grid_spec(nx_cells, ny_cells, dx=300000.0):
    return {"grid": [nx_cells, ny_cells], "dx": dx}


@functools.lru_cache(maxsize=None)
def _mesh(key):
    from mpassit_amd import synth, target_grid as tg
    spec = json.loads(key)
    if spec["mesh"] == "geodesic":
        m = synth.geodesic_mesh(spec["freq"])
    elif spec["mesh"] == "voronoi":
        m = synth.global_voronoi_mesh(spec["cells"], seed=spec["seed"])
    else:
        px, py = spec["points"]
        g = tg.define_target_grid_params("lambert", px, py, dx=spec["dx"], dy=spec["dx"], **LAMBERT)
        m = synth.regional_mesh_for_lambert(g.proj, px, py, spec["cells"], margin=0.0, seed=spec["seed"])
    every = spec.get("reverse_every", 0)
    if every:                      # the listed vertex order of every `every`-th cell reversed: the same cells, the other orientation
        voc = np.array(m.verticesOnCell, np.int32)
        for c in range(0, voc.shape[0], every):
            n = int((voc[c] > 0).sum())
            voc[c, :n] = voc[c, :n][::-1].copy()
        m = dataclasses.replace(m, verticesOnCell=voc)
    return m


def mesh_of(spec):
    return _mesh(json.dumps(spec, sort_keys=True))


@functools.lru_cache(maxsize=None)
def _grid(nx_cells, ny_cells, dx):
    from mpassit_amd import target_grid as tg
    g = tg.define_target_grid_params("lambert", nx_cells + 1, ny_cells + 1, dx=dx, dy=dx, **LAMBERT)
    assert (g.nx, g.ny) == (nx_cells, ny_cells)
    return g


def grid_of(spec):
    return _grid(spec["grid"][0], spec["grid"][1], spec["dx"])


def side_arrays(o, spec):
    """The float64 inputs of one side, as the fixture stores them: a mesh's vert_xyz [nVertices][3], cell_xyz [nCells][3] and voc; a
    grid's corner_xyz [(ny + 1) * (nx + 1)][3], cell_xyz [ny * nx][3] and shape (nx, ny)."""
    if "mesh" in spec:
        m = mesh_of(spec)
        return {"vert_xyz": o.lonlat_deg_to_xyz(*o.mesh_coords_deg(m.lonVertex, m.latVertex)),
                "cell_xyz": o.lonlat_deg_to_xyz(*o.mesh_coords_deg(m.lonCell, m.latCell)), "voc": np.asarray(m.verticesOnCell, np.int32)}
    g = grid_of(spec)
    return {"corner_xyz": o.lonlat_deg_to_xyz(g.lon_c, g.lat_c), "cell_xyz": o.lonlat_deg_to_xyz(g.lon, g.lat),
            "shape": np.array([g.nx, g.ny], np.int32)}


def first_order_pattern(o, src_spec, dst_spec, norm):
    """(rowptr, col) of the CPU reference's first-order conservative Store for the pairing: tests/_mesh_conserve_ref.py between two meshes,
    the oracle's Mesh -> Grid matrix onto a grid, and tests/_conserve_to_mesh_ref.py's B from that matrix for Grid -> Mesh."""
    import _conserve_to_mesh_ref as CR
    import _mesh_conserve_ref as MR
    if "mesh" in src_spec and "mesh" in dst_spec:
        rp, col = MR.Answer(o, mesh_of(src_spec), mesh_of(dst_spec)).rows(norm)[:2]
        return np.asarray(rp, np.int64), np.asarray(col, np.int32)
    m, g = (mesh_of(src_spec), grid_of(dst_spec)) if "mesh" in src_spec else (mesh_of(dst_spec), grid_of(src_spec))
    vxyz = o.lonlat_deg_to_xyz(*o.mesh_coords_deg(m.lonVertex, m.latVertex))
    kxyz = o.lonlat_deg_to_xyz(g.lon_c, g.lat_c)
    rp, col, val = o.conserve(m.verticesOnCell, vxyz, g.nx, g.ny, kxyz)
    if "mesh" in src_spec:
        assert norm == NORM_DSTAREA
        return np.asarray(rp, np.int64), np.asarray(col, np.int32)
    b = CR.b_ref_from_csr(rp, col, val, CR.grid_cell_areas(kxyz, g.nx, g.ny), CR.mesh_cell_areas(m.verticesOnCell, vxyz), norm)
    return np.asarray(b[0], np.int64), np.asarray(b[1], np.int32)


def source_mask(n_src):
    sm = np.zeros(n_src, np.uint8)
    sm[::MASK_EVERY] = 1
    return sm


def entry_rule(rowptr, col, sm):
    """The pattern MPG_MASKRULE_ENTRY leaves: the entries of masked sources removed, the rest in stored order."""
    keep = sm[col] == 0
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    return np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=rowptr.size - 1))]).astype(np.int64), col[keep]


def load():
    """(the json document, {case name: its arrays by short name and its meta}) of tests/golden/conserve2nd_hp.*"""
    with open(os.path.join(HERE, "golden", "conserve2nd_hp.json")) as f:
        doc = json.load(f)
    with np.load(os.path.join(HERE, "golden", "conserve2nd_hp.npz")) as f:
        z = {k: f[k] for k in f.files}
    z.update({k: z[target] for k, target in doc["aliases"].items()})          # an array stored once for several names
    for a in z.values():
        a.setflags(write=False)
    sides = {k: {f[len(k) + 1:]: z[f] for f in z if f.startswith(k + "/")} for k in doc["sides"]}
    cases = {}
    for name, m in doc["cases"].items():
        pre = "c%d/" % m["index"]
        c = {f[len(pre):]: z[f] for f in z if f.startswith(pre)}
        c.update(meta=m, src=sides[m["src_side"]], dst=sides[m["dst_side"]])
        cases[name] = c
    for k, m in doc["_mutants"].items():
        m["rows"] = tuple(z["m%s/%s" % (k, part)] for part in ("rowptr", "col", "val"))
    return doc, cases


def mirror_polys(tg, side):
    """One side's stored arrays as target_grid.conserve2nd_rows takes them."""
    if "voc" in side:
        return tg.conserve2nd_polygons_mesh(side["voc"], side["vert_xyz"].T, side["cell_xyz"].T)
    nx, ny = (int(v) for v in side["shape"])
    return tg.conserve2nd_polygons_grid(side["corner_xyz"].T, nx, ny, side["cell_xyz"].T)


def mirror_neighbours(o, tg, side):
    if "voc" in side:
        tri, _ = o.dual_triangles(side["voc"], side["vert_xyz"].shape[0], side["cell_xyz"])
        return tg.patch_neighbours_mesh(side["voc"], tri)
    return tg.patch_neighbours_grid(int(side["shape"][0]), int(side["shape"][1]))


def run_mirror(o, tg, c, src=None, dst=None):
    """target_grid._conserve2nd_rows on a case's stored inputs (or on other vectors for its two sides) -> (rowptr, col, val, info)"""
    src, dst = c["src"] if src is None else src, c["dst"] if dst is None else dst
    return tg._conserve2nd_rows(c["in_rowptr"].astype(np.int64), c["in_col"], mirror_polys(tg, src), mirror_polys(tg, dst),
                                mirror_neighbours(o, tg, src), c["meta"]["norm"], c.get("src_mask"))


def nudged(side, rng):
    """The side with every unit vector moved by one unit in the last place of each component, up or down at random, and renormalised."""
    out = dict(side)
    for k in ("vert_xyz", "corner_xyz", "cell_xyz"):
        if k in side:
            x = np.nextafter(side[k], np.where(rng.integers(0, 2, side[k].shape) == 1, np.inf, -np.inf))
            out[k] = x / np.sqrt((x * x).sum(axis=1))[:, None]
    return out


def measure(o, tg, c):
    """The two figures of a case, each against the golden: the worst |mirror - golden| of val on the stored inputs, and on inputs moved
    by a random last-bit change (nudged, seed 1234); the worst change of the mirror's own val between the two goes with them."""
    base = run_mirror(o, tg, c)
    rng = np.random.default_rng(1234)
    moved = run_mirror(o, tg, c, nudged(c["src"], rng), nudged(c["dst"], rng))
    for got in (base, moved):
        assert np.array_equal(got[0], c["rowptr"]) and np.array_equal(got[1], c["col"]), "the mirror's pattern is not the golden's"
    return {"mirror_minus_golden": float(np.abs(base[2] - c["val"]).max()), "one_ulp_minus_golden": float(np.abs(moved[2] - c["val"]).max()),
            "one_ulp_sensitivity": float(np.abs(moved[2] - base[2]).max())}


def union_difference(a, b):
    """(worst |a - b|, worst entry present on one side only, how many of those) of two CSR matrices (rowptr, col, val) over the union of
    their entries, a missing entry counting as 0."""
    keys, vals = [], []
    for rp, col, val in (a, b):
        rows = np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp))
        keys.append((rows << 32) | np.asarray(col, np.int64))
        vals.append(np.asarray(val, np.float64))
    both = np.union1d(keys[0], keys[1])
    dense = [np.zeros(both.size), np.zeros(both.size)]
    have = [np.zeros(both.size, bool), np.zeros(both.size, bool)]
    for k in range(2):
        at = np.searchsorted(both, keys[k])
        np.add.at(dense[k], at, vals[k])
        have[k][at] = True
    one = have[0] != have[1]
    diff = np.abs(dense[0] - dense[1])
    return float(diff.max()) if both.size else 0.0, float(diff[one].max()) if one.any() else 0.0, int(one.sum())
