#!/usr/bin/env python3
"""Every array of every RegridStore handle of a fixed list of small cases, as raw bytes: the evidence that a change to the Stores' code
leaves their results bit for bit what they were.

    MPASSIT_AMD_LIB=<library A> python tools/store_handles_dump.py --out dirA      (a fresh process per library)
    MPASSIT_AMD_LIB=<library B> python tools/store_handles_dump.py --out dirB
    python tools/store_handles_dump.py --compare dirA dirB                         -> one JSON line, exit status 1 unless all are equal

Per handle <case>.idx / .w (fixed handles) or .rowptr / .col / .val (CSR), .dst_frac and .pole_dst / .pole_src0 / .pole_w where the handle
has them, and <case>.info.json = mpg_handle_info, store_path and store_stats.  store_stats[3] of the Mesh -> Mesh Stores is a time (the
microseconds their tree took to build) and is written as 0.

The cases are the smallest that reach every search of the Stores: the four mesh / grid pairs of tests/golden/store_hp.json (whole mesh and
mesh window, every Mesh -> Grid method, with and without "store_boxes", both "nn_variant"s, both "bilinear_linetype"s, their destaggering
Stores), a coarse mesh under fine grids (triangles handed to the wave rasteriser, polygons to the cooperative conservative passes),
Grid -> Mesh on every stagger by both routes, the periodic layouts of tests/_periodic_layouts.py by both routes, conservative Grid -> Mesh
with both norms, and the Mesh -> Mesh pairs of tests/_mesh_to_mesh_cases.py."""
import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def compare(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    equal, different, nbytes = 0, [], 0
    for f in sorted(set(fa) & set(fb)):
        xa, xb = open(os.path.join(a, f), "rb").read(), open(os.path.join(b, f), "rb").read()
        nbytes += len(xa)
        if xa == xb:
            equal += 1
        else:
            different.append(f)
    missing = sorted(set(fa) ^ set(fb))
    print(json.dumps({"files": len(set(fa) | set(fb)), "bytes": nbytes, "equal": equal, "different": different, "missing": missing}))
    return 0 if not different and not missing and equal else 1


class Dump:
    def __init__(self, out):
        self.out, self.n = out, 0
        os.makedirs(out, exist_ok=True)

    def __call__(self, name, rh, zero_stat3=False):
        def put(ext, a):
            a.tofile(os.path.join(self.out, "%s.%s" % (name, ext)))
        if rh.nnz_per_row > 0:
            idx, w = rh.weights()
            put("idx", idx)
            put("w", w)
        else:
            rowptr, col, val = rh.csr()
            put("rowptr", rowptr)
            put("col", col)
            put("val", val)
        try:
            put("dst_frac", rh.dst_frac())
        except Exception:
            pass   # the handle has none
        dst, src0, wp, row_len = rh.pole()
        if dst.size:
            put("pole_dst", dst)
            put("pole_src0", src0)
            put("pole_w", wp)
        stats = rh.store_stats
        if zero_stat3:
            stats[3] = 0
        info = dict(n_src=rh.n_src, n_dst=rh.n_dst, nx_dst=rh.nx_dst, ny_dst=rh.ny_dst, nnz_per_row=rh.nnz_per_row, nnz=rh.nnz,
                    store_path=rh.store_path, store_stats=stats, pole_len=row_len)
        with open(os.path.join(self.out, name + ".info.json"), "w") as f:
            json.dump(info, f, sort_keys=True)
        rh.release()
        self.n += 1


def run(out):
    from mpassit_amd import _lib, regrid as R, synth, target_grid as tg
    import _mesh_conserve_ref as MCR
    import _mesh_to_mesh_cases as MC
    import _periodic_layouts as PL
    from test_store_goldens import cases
    _lib.init(0)
    dump = Dump(out)
    BIL, NEAR, CONS = R.REGRIDMETHOD_BILINEAR, R.REGRIDMETHOD_NEAREST_STOD, R.REGRIDMETHOD_CONSERVE

    def mesh_to_grid(tag, make_mesh, make_grid):
        """the four Mesh -> Grid Stores under every setting of the three knobs; fresh objects per setting (nothing from the handle cache)"""
        for boxes, nnv, line in itertools.product((1, 0), (1, 0), (0, 1)):
            _lib.tune("store_boxes", boxes)
            _lib.tune("nn_variant", nnv)
            _lib.tune("bilinear_linetype", line)
            mesh, grid = make_mesh(), make_grid()
            knobs = "b%dn%dl%d" % (boxes, nnv, line)
            if nnv == 1:    # (the bilinear and conservative Stores do not read "nn_variant")
                dump("%s.%s.bil_elem" % (tag, knobs), R.regrid_store(mesh, grid, BIL))
                dump("%s.%s.bil_node" % (tag, knobs), R.regrid_store(mesh, grid, BIL, meshloc=R.MESHLOC_NODE))
            if line == 0:
                dump("%s.%s.nearest" % (tag, knobs), R.regrid_store(mesh, grid, NEAR))
            if nnv == 1 and line == 0:
                dump("%s.%s.conserve" % (tag, knobs), R.regrid_store(mesh, grid, CONS))
            mesh.destroy()
            grid.destroy()
        _lib.tune("store_boxes", 1)
        _lib.tune("nn_variant", 1)
        _lib.tune("bilinear_linetype", 0)

    # 1. the pairs of tests/golden/store_hp.json: grids from arrays; the first also from its namelist (index-space route); mesh windows
    for c in cases():
        def arrays_grid(c=c):
            return R.Grid(c.lon, c.lat, c.lon_c, c.lat_c, c.lon_u, c.lat_u, c.lon_v, c.lat_v)
        mesh_to_grid(c.name, lambda c=c: R.Mesh.from_mpas(c.mesh), arrays_grid)
        grid = arrays_grid()
        for key, stag in (("edge1", R.STAGGERLOC_EDGE1), ("edge2", R.STAGGERLOC_EDGE2)):
            dump("%s.destagger_%s" % (c.name, key), R.regrid_store_grid(grid, stag))
        wmesh = R.Mesh.from_mpas(c.mesh, window_grid=grid)     # k_cell_dist and the closure of the window
        with open(os.path.join(out, "%s.window.info.json" % c.name), "w") as f:
            json.dump([float(x) for x in wmesh.window_info()], f)
        for name, method in (("bil", BIL), ("nearest", NEAR), ("conserve", CONS)):
            dump("%s.window.%s" % (c.name, name), R.regrid_store(wmesh, grid, method))
        wmesh.destroy()
        grid.destroy()
    g0 = tg.define_target_grid_params("lambert", 18, 14, dx=120000.0, dy=120000.0, **MC.LAMBERT)
    mesh_to_grid("regional_lambert_120km_proj", lambda: R.Mesh.from_mpas(cases()[0].mesh), lambda: R.Grid.from_target(g0))
    # 2. a coarse mesh under fine grids
    coarse = synth.geodesic_mesh(4)
    gl = tg.define_target_grid_params("lat-lon", 201, 121, stand_lon=0.0, is_regional=False)
    mesh_to_grid("geo4_under_latlon_200x120", lambda: R.Mesh.from_mpas(coarse), lambda: R.Grid.from_proj(gl))
    gr = tg.define_target_grid_params("lambert", 201, 121, dx=12000.0, dy=12000.0, **MC.LAMBERT)
    mesh_to_grid("geo4_under_lambert_200x120", lambda: R.Mesh.from_mpas(coarse), lambda: R.Grid.from_proj(gr))
    # 3. Grid -> Mesh: every stagger, bilinear and nearest, index route and walk; conservative with both norms
    g = tg.define_target_grid_params("lambert", 61, 41, dx=30000.0, dy=30000.0, **MC.LAMBERT)
    meshes = dict(over=synth.regional_mesh_for_lambert(g.proj, 61, 41, 6001, margin=0.05, seed=11),
                  coarse=synth.regional_mesh_for_lambert(g.proj, 61, 41, 201, margin=0.05, seed=13))
    ga = R.Grid.from_proj(g, fill_target=False)
    co = {st: ga.coords(st) for st in range(4)}
    gb = R.Grid(co[0][0], co[0][1], co[3][0], co[3][1], co[1][0], co[1][1], co[2][0], co[2][1])
    for mname, m in meshes.items():
        mesh = R.Mesh.from_mpas(m)
        for route, grid in (("index", ga), ("walk", gb)):
            for st, loc in itertools.product(range(4), (R.MESHLOC_ELEMENT, R.MESHLOC_NODE)):
                dump("to_mesh.%s.%s.st%d.loc%d.bil" % (mname, route, st, loc), R.regrid_store_to_mesh(grid, mesh, BIL, staggerloc=st, meshloc=loc))
                dump("to_mesh.%s.%s.st%d.loc%d.nearest" % (mname, route, st, loc), R.regrid_store_to_mesh(grid, mesh, NEAR, staggerloc=st, meshloc=loc))
            for norm in (R.NORM_DSTAREA, R.NORM_FRACAREA):
                dump("conserve_to_mesh.%s.%s.norm%d" % (mname, route, norm), R.regrid_store_conserve_to_mesh(grid, mesh, norm))
        mesh.destroy()
    _lib.tune("store_boxes", 0)     # ... and the walk on the grid that has an index space
    ga2, mesh2 = R.Grid.from_proj(g, fill_target=False), R.Mesh.from_mpas(meshes["over"])
    dump("to_mesh.over.boxes0.bil", R.regrid_store_to_mesh(ga2, mesh2))
    dump("to_mesh.over.boxes0.nearest", R.regrid_store_to_mesh(ga2, mesh2, NEAR))
    dump("conserve_to_mesh.over.boxes0", R.regrid_store_conserve_to_mesh(ga2, mesh2))
    _lib.tune("store_boxes", 1)
    for o in (ga, gb, ga2, mesh2):
        o.destroy()
    # 4. the periodic layouts by both routes, cells and vertices
    gm = R.Mesh.from_mpas(MC.mesh("vor1500"))
    for name in PL.LAYOUTS:
        lon, lat = PL.coords(name)
        for route in ("walk", "index") if name in PL.UNIFORM else ("walk",):
            grid = R.Grid(lon, lat, periodic=_lib.GRID_PERIODIC_I)
            if route == "index":
                grid.attach_proj(PL.proj(name))
            for loc in (R.MESHLOC_ELEMENT, R.MESHLOC_NODE):
                dump("periodic.%s.%s.loc%d" % (name, route, loc), R.regrid_store_periodic_to_mesh(grid, gm, meshloc=loc))
            dump("periodic.%s.%s.nopole" % (name, route), R.regrid_store_periodic_to_mesh(grid, gm, pole_method=R.POLEMETHOD_NONE))
            grid.destroy()
    gm.destroy()
    # 5. Mesh -> Mesh: bilinear with both line types, nearest, conservative with both norms
    for name in MC.PAIR_NAMES:
        s, d, loc = MC.pair(name)
        for line in (0, 1):
            _lib.tune("bilinear_linetype", line)
            src, dst = R.Mesh.from_mpas(s), R.Mesh.from_mpas(d)
            dump("mesh.%s.bil_l%d" % (name, line), R.regrid_store_mesh(src, dst, BIL, dst_meshloc=loc), zero_stat3=True)
            if line == 0:
                dump("mesh.%s.nearest" % name, R.regrid_store_mesh(src, dst, NEAR, dst_meshloc=loc), zero_stat3=True)
                if name in MCR.PAIRS:
                    for norm in (R.NORM_DSTAREA, R.NORM_FRACAREA):
                        dump("mesh.%s.conserve_norm%d" % (name, norm), R.regrid_store_conserve_mesh(src, dst, norm), zero_stat3=True)
            src.destroy()
            dst.destroy()
    _lib.tune("bilinear_linetype", 0)
    print("%d handles written to %s" % (dump.n, out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("DIR_A", "DIR_B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    run(args.out)
