"""The periodic Grid -> Mesh reference (tests/_periodic_to_mesh_ref.py) checked on its own, on the CPU: the inputs of the GPU tests map
as the issue's table says, rows are well formed, and deliberately wrong variants of the rule are told apart -- so a library that made one
of those mistakes could not pass the GPU comparison.

Caps and quads share nothing but their common edge (the cap triangle (A, B, pole) and the quads of the end row meet in the great circle
through A and B), so on points away from every edge the ORDER in which they are tried cannot show.  That mutation is therefore checked on
points placed on that edge, where both pass: the rule gives them a quad row, a cap tried first a cap row."""
import numpy as np
import pytest

import _periodic_to_mesh_ref as PR
from _parity_helpers import assert_csr_equal

TIE_CAP = 1e-4            # tests/test_to_mesh_gpu.py
GRIDS = {"72x36": (73, 37), "24x12": (25, 13)}
# (points, mapped by quads, in caps, in seam quads) per grid and mesh location
TABLE = {("72x36", 0): (20000, 19981, 19, 280), ("24x12", 0): (20000, 19831, 169, 829),
         ("72x36", 1): (39996, 39957, 39, 550), ("24x12", 1): (39996, 39660, 336, 1650)}


@pytest.fixture(scope="module")
def inputs(oracle, global_mesh):
    from mpassit_amd import target_grid as tg
    d = {}
    for name, (nxn, nyn) in GRIDS.items():
        g = tg.define_target_grid_params("lat-lon", nx=nxn, ny=nyn, stand_lon=0.0, is_regional=False)
        d[name] = oracle.lonlat_deg_to_xyz(g.lon, g.lat).reshape(g.lat.shape + (3,))
    m = global_mesh
    d["pts"] = {0: oracle.lonlat_deg_to_xyz(*oracle.mesh_coords_deg(m.lonCell, m.latCell)),
                1: oracle.lonlat_deg_to_xyz(*oracle.mesh_coords_deg(m.lonVertex, m.latVertex))}
    return d


@pytest.fixture(scope="module")
def refs(oracle, inputs):
    return {(name, loc): PR.periodic_to_mesh(oracle, inputs[name], inputs["pts"][loc]) for name in GRIDS for loc in (0, 1)}


@pytest.mark.parametrize("name", list(GRIDS))
@pytest.mark.parametrize("loc", [0, 1])
def test_rows_are_well_formed(refs, name, loc):
    r = refs[(name, loc)]
    n, nx, ny = r["kind"].size, r["nx"], r["ny"]
    quads, caps, seam = r["kind"] == PR.KIND_QUAD, r["kind"] == PR.KIND_CAP, PR.seam_rows(r)
    assert (n, int(quads.sum()), int(caps.sum()), seam.size) == TABLE[(name, loc)]
    assert not (r["kind"] == PR.KIND_NONE).any(), "every point is mapped under ALLAVG"
    lens = np.diff(r["rowptr"])
    assert np.all(lens[quads] == 4) and np.all(lens[caps] == nx)
    rows = np.repeat(np.arange(n), lens)
    assert np.abs(np.bincount(rows, weights=r["val"], minlength=n) - 1.0).max() < 1e-12
    inside = np.ones(r["col"].size - 1, bool)
    inside[r["rowptr"][1:-1] - 1] = False
    assert np.all(np.diff(r["col"])[inside] > 0), "columns ascend within a row"
    assert r["col"].min() >= 0 and r["col"].max() < nx * ny
    for p in seam:      # a seam row references column 0 and column nx - 1 of both its rows
        c = r["col"][r["rowptr"][p]:r["rowptr"][p + 1]]
        assert sorted(c % nx) == [0, 0, nx - 1, nx - 1] and c[2] - c[0] == nx
    for p in np.nonzero(caps)[0]:
        c = r["col"][r["rowptr"][p]:r["rowptr"][p + 1]]
        assert c[0] in (0, (ny - 1) * nx) and np.array_equal(c, c[0] + np.arange(nx))
    share = PR.edge_share(r)
    print("%s loc %d: smallest margin %.3g (quads) %.3g (caps), share within 1e-9 of an edge %.3g" % (
        name, loc, np.nanmin(r["edge"][quads]), np.nanmin(r["edge"][caps]), share))
    assert share <= TIE_CAP and share == 0.0


@pytest.mark.parametrize("name", list(GRIDS))
def test_pole_method_none_and_row_block_flags(oracle, inputs, refs, name):
    r = refs[(name, 0)]
    caps = r["kind"] == PR.KIND_CAP
    none = PR.periodic_to_mesh(oracle, inputs[name], inputs["pts"][0], pole_method=PR.POLE_NONE)
    assert np.array_equal(np.diff(none["rowptr"]) == 0, caps), "under NONE exactly the cap points are empty"
    keep = np.repeat(~caps, np.diff(r["rowptr"]))
    assert np.array_equal(none["col"], r["col"][keep]) and np.array_equal(none["val"], r["val"][keep])
    north = caps & (r["cap"] >= r["nx"])
    blk = PR.periodic_to_mesh(oracle, inputs[name], inputs["pts"][0], flags=PR.NO_NORTH)
    assert np.array_equal(np.diff(blk["rowptr"]) == 0, north) and north.any() and (caps & ~north).any()
    blk = PR.periodic_to_mesh(oracle, inputs[name], inputs["pts"][0], flags=PR.NO_SOUTH)
    assert np.array_equal(np.diff(blk["rowptr"]) == 0, caps & ~north)


@pytest.mark.parametrize("mutation", ["seam_swap_bc", "cap_no_division"])
@pytest.mark.parametrize("name", list(GRIDS))
def test_mutations_fail_the_comparison(oracle, inputs, refs, name, mutation):
    r = refs[(name, 0)]
    bad = PR.periodic_to_mesh(oracle, inputs[name], inputs["pts"][0], mutate=mutation)
    with pytest.raises(AssertionError):
        assert_csr_equal(r["rowptr"], r["col"], r["val"], bad["rowptr"], bad["col"], bad["val"], r["nx"] * r["ny"], tol=1e-11)


@pytest.mark.parametrize("name", list(GRIDS))
def test_a_cap_tried_first_shows_on_the_shared_edge(oracle, inputs, name):
    cen = inputs[name]
    ny, nx, _ = cen.shape
    a = np.array([0, 1, nx // 2, nx - 1])                      # the seam's cap edge included
    mid = np.concatenate([cen[ny - 1, a] + cen[ny - 1, (a + 1) % nx], cen[0, a] + cen[0, (a + 1) % nx]])
    mid /= np.linalg.norm(mid, axis=1, keepdims=True)
    r = PR.periodic_to_mesh(oracle, cen, mid)
    assert np.all(r["kind"] == PR.KIND_QUAD) and np.all(np.diff(r["rowptr"]) == 4), "quads are tried first: a point on the edge has a quad row"
    assert np.array_equal(r["quad"], np.concatenate([(ny - 2) * nx + a, a]))
    bad = PR.periodic_to_mesh(oracle, cen, mid, mutate="caps_first")
    assert np.all(bad["kind"] == PR.KIND_CAP) and np.all(np.diff(bad["rowptr"]) == nx)
    # ... and away from every edge it cannot: the mesh points give the same rows either way
    pts = inputs["pts"][0][::7]
    x, y = PR.periodic_to_mesh(oracle, cen, pts), PR.periodic_to_mesh(oracle, cen, pts, mutate="caps_first")
    assert np.array_equal(x["rowptr"], y["rowptr"]) and np.array_equal(x["col"], y["col"]) and np.array_equal(x["val"], y["val"])
