"""The mesh pairs of the Mesh -> Mesh tests, built once per process, and the oracle's answer for them.

test_mesh_to_mesh_abi.py qualifies these inputs on the CPU (the oracle alone must show no destination point within TIE_TOL of a
triangle edge beyond TIE_CAP of the mapped points: the pairs are unrelated point sets); test_mesh_to_mesh_gpu.py holds the Store to the
same oracle answers.  Everything is a few thousand cells: the oracle's all-triangles search takes milliseconds."""
import functools

import numpy as np

TIE_TOL = 1e-9     # a destination point this close (in barycentric weight) to a triangle edge may sit in either neighbour
TIE_CAP = 1e-3     # at most 0.1 % of a pair's mapped points may be that close

LAMBERT = dict(ref_lat=38.5, ref_lon=-97.5, truelat1=38.5, truelat2=38.5, stand_lon=-97.5)

# name -> (source mesh, destination mesh, destination location: 0 cells, 1 vertices)
PAIR_NAMES = ("geo10_to_vor1500", "vor2500_to_hex", "hex_to_geo10", "varres3000_to_geo8", "geo10_to_vor1500_nodes")


@functools.lru_cache(maxsize=None)
def mesh(name):
    from mpassit_amd import synth, target_grid as tg
    if name == "geo10":
        return synth.geodesic_mesh(10)                                   # 1002 cells: 42 points in the last block of 64
    if name == "geo8":
        return synth.geodesic_mesh(8)                                    # 642 cells
    if name == "vor1500":
        return synth.global_voronoi_mesh(1500, seed=101)
    if name == "vor2500":
        return synth.global_voronoi_mesh(2500, seed=202)                 # valences 4 .. 7
    if name == "varres3000":
        return synth.variable_resolution_mesh(3000)
    if name == "hex_small":                                              # a limited-area mesh inside a few dozen global cells
        g = tg.define_target_grid_params("lambert", 61, 41, dx=30000.0, dy=30000.0, **LAMBERT)
        return synth.regional_mesh_for_lambert(g.proj, 61, 41, 1201, margin=0.02, seed=31)
    if name == "hex_large":                                              # a regional SOURCE: 9000 x 5400 km, most of the globe outside it
        g = tg.define_target_grid_params("lambert", 151, 91, dx=60000.0, dy=60000.0, **LAMBERT)
        return synth.regional_mesh_for_lambert(g.proj, 151, 91, 2001, margin=0.0, seed=32)
    raise KeyError(name)


def pair(name):
    src, dst, loc = {"geo10_to_vor1500": ("geo10", "vor1500", 0), "vor2500_to_hex": ("vor2500", "hex_small", 0),
                     "hex_to_geo10": ("hex_large", "geo10", 0), "varres3000_to_geo8": ("varres3000", "geo8", 0),
                     "geo10_to_vor1500_nodes": ("geo10", "vor1500", 1)}[name]
    return mesh(src), mesh(dst), loc


def cell_xyz(o, m):
    return o.lonlat_deg_to_xyz(*o.mesh_coords_deg(m.lonCell, m.latCell))


def points(o, m, loc):
    lon, lat = (m.lonCell, m.latCell) if loc == 0 else (m.lonVertex, m.latVertex)
    return o.lonlat_deg_to_xyz(*o.mesh_coords_deg(lon, lat))


_ANSWERS = {}


def oracle_bilinear(o, name, linetype):
    """(idx [P][3], w [P][3], pts, source cell xyz) of the oracle for pair `name`; computed once, never modified."""
    key = (name, linetype)
    if key not in _ANSWERS:
        src, dst, loc = pair(name)
        cx = cell_xyz(o, src)
        tri, _ = o.dual_triangles(src.verticesOnCell, src.nVertices, cx)
        pts = points(o, dst, loc)
        idx, w = o.bilinear_weights(cx, tri, pts, linetype)
        for a in (idx, w, pts, cx):
            a.setflags(write=False)
        _ANSWERS[key] = (idx, w, pts, cx)
    return _ANSWERS[key]


def edge_share(idx, w):
    """Share of the mapped points with a weight within TIE_TOL of zero: on (or within the tolerance of) a triangle edge."""
    mapped = idx[:, 0] >= 0
    if not mapped.any():
        return 0.0
    return float((np.abs(w[mapped]).min(axis=1) < TIE_TOL).mean())


def smooth_field(m, nlev=1):
    """A smooth function of position on the cells of `m`, [nCells][nlev] (MPAS file order): the same function on any numbering."""
    from mpassit_amd import synth
    return synth.analytic_field(m.latCell, m.lonCell, nlev, cell_fast=False)
