"""The library's Grid -> Mesh, periodic Grid -> Mesh and Mesh -> Mesh Stores and its mesh rotation angles, through the C-ABI, against the
50-digit brute-force goldens of tests/test_mesh_store_goldens.py (the checkers are that file's): both candidate routes of the two
Grid -> Mesh Stores (index space and pyramid, grids made from arrays and from their projection), all three mesh locations, both pole
methods, both line types, both conservative normalisations with the dst fraction.  Not the oracle and not a float64 restatement: an
answer that shares no code with either side.  The bars are the ones the float64 references meet on the CPU."""
import numpy as np
import pytest

import test_mesh_store_goldens as G

pytestmark = pytest.mark.gpu

LOC_ID = {"cell": 0, "vertex": 1, "edge": 2}
STAGGER_ID = {"center": 0, "edge1": 1, "edge2": 2}


def _regional_grid(R, case, from_projection):
    if from_projection:            # the arrays of the fixture, with their projection attached: the index route
        return R.Grid.from_target(case.target())
    (lon, lat), (lon_u, lat_u), (lon_v, lat_v) = (case.coords[s] for s in G.STAGGERS)
    return R.Grid(lon, lat, None, None, lon_u, lat_u, lon_v, lat_v)


@pytest.mark.parametrize("route", ["arrays", "projection", "projection_boxes_off"])
@pytest.mark.parametrize("case", G.regional_cases(), ids=lambda c: c.name)
def test_library_grid_to_mesh_stores_equal_the_goldens(gpu_lib, case, route):
    """EDGE1, EDGE2 and CENTER onto cells, vertices and edges, bilinear and nearest; `projection` must take the index route and
    mpg_tune("store_boxes", 0) the pyramid on the same grid.  Fresh objects per route: nothing comes from the handle cache."""
    from mpassit_amd import regrid as R
    grid, mesh = _regional_grid(R, case, route != "arrays"), R.Mesh.from_mpas(case.mesh)
    worst = 0.0
    gpu_lib.tune("store_boxes", 0 if route == "projection_boxes_off" else 1)
    try:
        for stagger in G.STAGGERS:
            for loc in G.LOCS:
                rb = R.regrid_store_to_mesh(grid, mesh, R.REGRIDMETHOD_BILINEAR, staggerloc=STAGGER_ID[stagger], meshloc=LOC_ID[loc])
                assert rb.store_path == (1 if route == "projection" else 0), (route, stagger, loc, rb.store_path)
                assert rb.nnz_per_row == 4
                worst = max(worst, G.check_quads(case, stagger, loc, *rb.weights()))
                rn = R.regrid_store_to_mesh(grid, mesh, R.REGRIDMETHOD_NEAREST_STOD, staggerloc=STAGGER_ID[stagger], meshloc=LOC_ID[loc])
                G.check_nearest(case.expect["nearest"][stagger][loc], rn.weights()[0][:, 0], "%s %s %s" % (case.name, stagger, loc))
                rb.release()
                rn.release()
    finally:
        gpu_lib.tune("store_boxes", 1)
        mesh.destroy()
        grid.destroy()
    print("%s %s: library vs 50 digits: bilinear %.1e (bar %.1e)" % (case.name, route, worst, G.tol_for(case.h)))


def _periodic_grid(R, L, case, with_projection):
    import _periodic_layouts as PL
    g = R.Grid(case.lon, case.lat, periodic=L.GRID_PERIODIC_I)
    if with_projection:
        g.attach_proj(PL.proj(case.layout))
    return g


def _periodic_routes(case):
    uniform = not case.layout.startswith("gauss")      # a lat-lon projection describes uniform rows only
    return ["arrays"] + (["projection", "projection_boxes_off"] if uniform else [])


@pytest.mark.parametrize("case,route", [(c, r) for c in G.periodic_cases() for r in _periodic_routes(c)], ids=lambda v: getattr(v, "name", v))
def test_library_periodic_to_mesh_stores_equal_the_goldens(gpu_lib, case, route):
    from mpassit_amd import _lib as L, regrid as R
    grid, mesh = _periodic_grid(R, L, case, route != "arrays"), R.Mesh.from_mpas(case.mesh)
    gpu_lib.tune("store_boxes", 0 if route == "projection_boxes_off" else 1)
    try:
        for loc in case.locs():
            for pole_method in (R.POLEMETHOD_ALLAVG, R.POLEMETHOD_NONE):
                rh = R.regrid_store_periodic_to_mesh(grid, mesh, meshloc=LOC_ID[loc], pole_method=pole_method)
                assert rh.store_path == (1 if route == "projection" else 0), (route, loc, rh.store_path)
                assert rh.nnz_per_row == 0
                worst, n, ncap, nseam, skipped = G.check_periodic(case, case.expect[loc], *rh.csr(), pole_method=pole_method)
                st = rh.store_stats
                golden_caps = sum(1 for e in case.expect[loc] if e and e.get("kind") == "cap") if pole_method == R.POLEMETHOD_ALLAVG else 0
                golden_seams = sum(1 for e in case.expect[loc] if e and e.get("kind") == "seam")
                assert st[2] == len(case.expect[loc])
                assert abs(st[3] - golden_caps) <= skipped and abs(st[4] - golden_seams) <= skipped, (case.name, loc, st[:5], golden_caps, golden_seams)
                print("%s %s %s pole method %d: library vs 50 digits %.1e over %d rows (%d cap, %d seam)" % (case.name, route, loc, pole_method, worst, n, ncap, nseam))
                rh.release()
    finally:
        gpu_lib.tune("store_boxes", 1)
        mesh.destroy()
        grid.destroy()


@pytest.mark.parametrize("linetype", [0, 1])
@pytest.mark.parametrize("case", G.pair_cases(), ids=lambda c: c.name)
def test_library_mesh_to_mesh_stores_equal_the_goldens(gpu_lib, case, linetype):
    from mpassit_amd import regrid as R
    src = R.Mesh.from_mpas(case.src)
    dst = src if case.dst is case.src else R.Mesh.from_mpas(case.dst)
    try:
        for loc in ("cell", "vertex"):
            gpu_lib.tune("bilinear_linetype", linetype)
            try:
                rb = R.regrid_store_mesh(src, dst, R.REGRIDMETHOD_BILINEAR, dst_meshloc=LOC_ID[loc])
            finally:
                gpu_lib.tune("bilinear_linetype", 0)
            assert rb.nnz_per_row == 3
            worst = G.check_mesh_bilinear(case, "bilinear%d" % linetype, loc, *rb.weights())
            print("%s line type %d %s: library vs 50 digits %.1e (bar %.1e)" % (case.name, linetype, loc, worst, G.tol_for(case.h)))
            rb.release()
            if linetype == 0 and loc in case.expect["nearest"]:
                rn = R.regrid_store_mesh(src, dst, R.REGRIDMETHOD_NEAREST_STOD, dst_meshloc=LOC_ID[loc])
                G.check_nearest(case.expect["nearest"][loc], rn.weights()[0][:, 0], "%s %s" % (case.name, loc))
                rn.release()
    finally:
        if dst is not src:
            dst.destroy()
        src.destroy()


@pytest.mark.parametrize("case", G.pair_cases(), ids=lambda c: c.name)
def test_library_conservative_mesh_to_mesh_stores_equal_the_goldens(gpu_lib, case):
    from mpassit_amd import regrid as R
    src = R.Mesh.from_mpas(case.src)
    dst = src if case.dst is case.src else R.Mesh.from_mpas(case.dst)
    try:
        for norm in (R.NORM_DSTAREA, R.NORM_FRACAREA):
            rh = R.regrid_store_conserve_mesh(src, dst, norm)
            worst, wf = G.check_mesh_conserve(case, *rh.csr(), rh.dst_frac(), norm)
            print("%s norm %d: library vs 50 digits (Girard): weights %.1e, dst fraction %.1e (bar %.1e)" % (case.name, norm, worst, wf, G.conserve_tol(case)))
            rh.release()
    finally:
        if dst is not src:
            dst.destroy()
        src.destroy()


@pytest.mark.parametrize("case", G.regional_cases(), ids=lambda c: c.name)
def test_library_mesh_angles_equal_the_goldens(gpu_lib, case):
    """mesh_rotang on cells and vertices, mesh_edge_rotang with the grid and with grid=None (alpha = 0: cos / sin of angleEdge itself)."""
    from mpassit_amd import regrid as R
    grid, mesh = R.Grid.from_target(case.target()), R.Mesh.from_mpas(case.mesh)
    try:
        exp = case.expect["angles"]
        out = [G.check_angles(exp[loc], ("cosa", "sina"), [t.cpu().numpy() for t in R.mesh_rotang(grid, mesh, LOC_ID[loc])], "%s %s" % (case.name, loc))
               for loc in ("cell", "vertex")]
        out.append(G.check_angles(exp["edge"], ("cn", "sn"), [t.cpu().numpy() for t in R.mesh_edge_rotang(grid, mesh)], case.name + " edges"))
        cn, sn = (t.cpu().numpy() for t in R.mesh_edge_rotang(None, mesh))
        theta = case.mesh.angleEdge
        assert np.abs(cn - np.cos(theta)).max() < G.ANGLE_TOL and np.abs(sn - np.sin(theta)).max() < G.ANGLE_TOL
        print("%s: library angles vs the differentiated forward map at 50 digits: worst %.1e" % (case.name, max(out)))
    finally:
        mesh.destroy()
        grid.destroy()
