"""The periodic Grid -> Mesh Store onto mesh EDGES on the GPU (mpg_regrid_store_periodic_to_mesh with MPG_MESHLOC_EDGE): parity with the
numpy restatement of the rule (tests/_periodic_to_mesh_ref.py) on the edge points, the reference's own counts, POLEMETHOD_NONE, the
handle's structure, byte identity with the Store onto cells at the same points, the cache and the refusal of a mesh without edges.

Inputs: the 20 000-cell global mesh with the 59 994 edges synth.mesh_edges derives, and the two global lat-lon grids of
tests/test_periodic_to_mesh_gpu.py, 72 x 36 and 24 x 12, each from its projection (the index route) and as arrays (the pyramid walk)."""
import ctypes as C

import numpy as np
import pytest

import _periodic_to_mesh_ref as PR
from _parity_helpers import assert_csr_equal

pytestmark = pytest.mark.gpu

TIE_CAP = 1e-4            # at most 1 row in 10 000 may be a point within 1e-9 of an edge (tests/test_periodic_to_mesh_gpu.py)
GRIDS = {"72x36": (73, 37), "24x12": (25, 13)}
NEDGES = 59994
# the reference's counts on these inputs, computed on the CPU: (cap edges, seam-quad edges, share within 1e-9 of an edge)
COUNTS = {"72x36": (57, 835, 0.0), "24x12": (505, 2482, 0.0)}


def _csr_identical(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x, y)) and np.array_equal(x[2].view(np.int64), y[2].view(np.int64))


@pytest.fixture(scope="module")
def case(gpu_lib, oracle, global_mesh):
    """Both grids both ways, the mesh with its edges, and the reference per (grid, pole method), computed once and left unchanged."""
    from mpassit_amd import _lib as L, regrid as R, synth, target_grid as tg
    m = synth.mesh_edges(global_mesh)
    assert m.nEdges == NEDGES
    d = dict(m=m, mesh=R.Mesh.from_mpas(m), tg={}, proj={}, arr={}, cen={}, ref={})
    assert d["mesh"].nEdges == NEDGES
    pts = oracle.lonlat_deg_to_xyz(*oracle.mesh_coords_deg(m.lonEdge, m.latEdge))
    for name, (nxn, nyn) in GRIDS.items():
        g = tg.define_target_grid_params("lat-lon", nx=nxn, ny=nyn, stand_lon=0.0, is_regional=False)
        d["tg"][name] = g
        d["proj"][name] = R.Grid.from_target(g)
        d["arr"][name] = R.Grid(g.lon, g.lat, periodic=L.GRID_PERIODIC_I)
        d["cen"][name] = oracle.lonlat_deg_to_xyz(g.lon, g.lat).reshape(g.lat.shape + (3,))

    def ref(name, pole_method=PR.POLE_ALLAVG):
        if (name, pole_method) not in d["ref"]:
            d["ref"][(name, pole_method)] = PR.periodic_to_mesh(oracle, d["cen"][name], pts, pole_method=pole_method)
        return d["ref"][(name, pole_method)]
    d["get_ref"] = ref
    yield d
    d["mesh"].destroy()
    for k in ("proj", "arr"):
        for grid in d[k].values():
            grid.destroy()


def _tie_rows(r, rp, col):
    """Rows whose column sets differ between the reference and the library: only a point within 1e-9 of an edge may be one."""
    rl, gl = np.diff(r["rowptr"]), np.diff(rp)
    diff = rl != gl
    same = np.nonzero(~diff)[0]
    for length in np.unique(rl[same]):
        if length == 0:
            continue
        rows = same[rl[same] == length]
        a = r["col"][r["rowptr"][rows][:, None] + np.arange(length)[None, :]]
        b = col[rp[rows][:, None] + np.arange(length)[None, :]]
        diff[rows[(a != b).any(axis=1)]] = True
    return np.nonzero(diff)[0]


@pytest.mark.parametrize("name", list(GRIDS))
def test_store_parity_counts_and_structure(case, name):
    """The Store onto edges against the reference by both routes; the reference's own counts; identical CSR bytes from the two routes;
    nnz = 4 (n - ncap) + nx ncap; no pole terms."""
    from mpassit_amd import regrid as R
    r = case["get_ref"](name)
    share = PR.edge_share(r)
    ncap, nseam = int((r["kind"] == PR.KIND_CAP).sum()), int(PR.seam_rows(r).size)
    print("reference %s edges: %d points, %d in caps, %d in seam quads, share within 1e-9 of an edge %.3g" % (name, r["kind"].size, ncap, nseam, share))
    assert (ncap, nseam, share) == COUNTS[name] and share <= TIE_CAP
    g, n = case["tg"][name], NEDGES
    got = {}
    for route, grid in (("index", case["proj"][name]), ("walk", case["arr"][name])):
        rh = R.regrid_store_periodic_to_mesh(grid, case["mesh"], meshloc=R.MESHLOC_EDGE)
        assert (rh.n_src, rh.n_dst, rh.nx_dst, rh.ny_dst, rh.nnz_per_row) == (g.lon.size, n, n, 1, 0)
        assert rh.nnz == 4 * (n - ncap) + g.lon.shape[1] * ncap
        assert all(a.size == 0 for a in rh.pole()[:3]), "the handle carries no pole terms"
        assert rh.store_ms > 0.0 and rh.store_path == (1 if route == "index" else 0)
        st = rh.store_stats
        print("%s route: store_path %d, stats %s, %.3f ms" % (route, rh.store_path, st[:5], rh.store_ms))
        assert st[2] == n and st[3] == ncap and st[4] == nseam
        rp, col, val = got[route] = rh.csr()
        ties = _tie_rows(r, rp, col)
        print("tie rows %d of %d" % (ties.size, n))
        assert ties.size <= TIE_CAP * n
        assert np.all(r["edge"][ties] < 1e-9), "a row differs from the reference's away from every edge"
        keep = np.ones(n, bool)
        keep[ties] = False
        if ties.size:   # examined above; the entry comparison below runs on the rows both sides agree on
            sel_r, sel_g = np.repeat(keep, np.diff(r["rowptr"])), np.repeat(keep, np.diff(rp))
            rr = (np.concatenate([[0], np.cumsum(np.where(keep, np.diff(r["rowptr"]), 0))]), r["col"][sel_r], r["val"][sel_r])
            gg = (np.concatenate([[0], np.cumsum(np.where(keep, np.diff(rp), 0))]), col[sel_g], val[sel_g])
        else:
            rr, gg = (r["rowptr"], r["col"], r["val"]), (rp, col, val)
        common, only_r, only_g = assert_csr_equal(rr[0], rr[1], rr[2], gg[0], gg[1], gg[2], rh.n_src, tol=1e-11)
        assert only_r == 0 and only_g == 0 and common == rr[1].size
        rows = np.repeat(np.arange(n), np.diff(rp))
        assert np.abs(np.bincount(rows, weights=val, minlength=n) - 1.0).max() < 1e-12, "every row sums to 1 under ALLAVG"
        rh.release()
    assert _csr_identical(got["index"], got["walk"]), "the two candidate routes give different CSR bytes"


@pytest.mark.parametrize("name", list(GRIDS))
def test_polemethod_none_leaves_the_cap_edges_empty(case, name):
    from mpassit_amd import regrid as R
    r = case["get_ref"](name)
    cap = r["kind"] == PR.KIND_CAP
    r0 = case["get_ref"](name, PR.POLE_NONE)
    assert np.array_equal(np.diff(r0["rowptr"]) == 0, cap) and int(cap.sum()) == COUNTS[name][0]
    avg = R.regrid_store_periodic_to_mesh(case["arr"][name], case["mesh"], meshloc=R.MESHLOC_EDGE)
    none = R.regrid_store_periodic_to_mesh(case["arr"][name], case["mesh"], meshloc=R.MESHLOC_EDGE, pole_method=R.POLEMETHOD_NONE)
    assert none._h.value != avg._h.value
    rp0, col0, val0 = none.csr()
    empty = np.diff(rp0) == 0
    assert int(empty.sum()) == COUNTS[name][0] and np.array_equal(empty, cap), "under NONE exactly the cap edges are empty"
    assert none.store_stats[3] == 0 and none.nnz == 4 * int((~cap).sum()) and none.store_stats[2] == NEDGES
    rp, col, val = avg.csr()
    q = np.nonzero(~cap)[0]
    at, at0 = rp[q][:, None] + np.arange(4)[None, :], rp0[q][:, None] + np.arange(4)[None, :]
    assert np.array_equal(col[at], col0[at0]) and np.array_equal(val[at].view(np.int64), val0[at0].view(np.int64)), "quad rows do not depend on the pole method"
    avg.release()
    none.release()


@pytest.mark.parametrize("name", list(GRIDS))
def test_edges_at_the_cell_centres_get_the_cell_handle(case, name):
    """A second mesh object whose EDGES are its own cell centres: MESHLOC_EDGE gives the rowptr / col / val bytes of MESHLOC_ELEMENT."""
    from mpassit_amd import regrid as R
    m = case["m"]
    mesh = R.Mesh(m.latCell, m.lonCell, m.latVertex, m.lonVertex, m.verticesOnCell)
    assert mesh.nEdges == 0
    mesh.set_edges(m.latCell, m.lonCell)
    assert mesh.nEdges == m.nCells
    for grid in (case["proj"][name], case["arr"][name]):
        for pm in (R.POLEMETHOD_ALLAVG, R.POLEMETHOD_NONE):
            re_ = R.regrid_store_periodic_to_mesh(grid, mesh, meshloc=R.MESHLOC_EDGE, pole_method=pm)
            rc = R.regrid_store_periodic_to_mesh(grid, mesh, meshloc=R.MESHLOC_ELEMENT, pole_method=pm)
            assert re_._h.value != rc._h.value
            assert (re_.n_dst, re_.nx_dst, re_.ny_dst, re_.nnz) == (m.nCells, m.nCells, 1, rc.nnz)
            assert _csr_identical(re_.csr(), rc.csr())
            assert re_.store_stats[2:5] == rc.store_stats[2:5]
            re_.release()
            rc.release()
    mesh.destroy()


def test_cache_and_refusal(case):
    from mpassit_amd import _lib as L, regrid as R
    lib = L.load()
    grid, mesh, m = case["arr"]["24x12"], case["mesh"], case["m"]
    a = R.regrid_store_periodic_to_mesh(grid, mesh, meshloc=R.MESHLOC_EDGE)
    b = R.regrid_store_periodic_to_mesh(grid, mesh, meshloc=R.MESHLOC_EDGE)
    assert a._h.value == b._h.value, "a second Store of the same key returns the cached handle"
    node = R.regrid_store_periodic_to_mesh(grid, mesh, meshloc=R.MESHLOC_NODE)
    cell = R.regrid_store_periodic_to_mesh(grid, mesh, meshloc=R.MESHLOC_ELEMENT)
    assert len({a._h.value, node._h.value, cell._h.value}) == 3, "EDGE, NODE and ELEMENT are three handles"
    assert (a.n_dst, node.n_dst, cell.n_dst) == (NEDGES, m.nVertices, m.nCells)
    for rh in (a, b, node, cell):
        rh.release()

    def refused(rc, want, *words):
        msg = lib.mpg_last_error().decode()
        assert rc == want and msg, (rc, want, msg)
        for word in words:
            assert word in msg, msg

    bare = R.Mesh(m.latCell, m.lonCell, m.latVertex, m.lonVertex, m.verticesOnCell)
    h = C.c_void_p()
    store = L.regrid_store_periodic_to_mesh
    refused(store(grid._h, bare._h, 2, 1, C.byref(h)), L.MPG_ERR_INVALID_ARG, "mesh location", "MPG_MESHLOC_NODE", "mpg_mesh_set_edges")
    with pytest.raises(L.MpgError) as e:
        R.regrid_store_periodic_to_mesh(grid, bare, meshloc=R.MESHLOC_EDGE)
    assert e.value.rc == L.MPG_ERR_INVALID_ARG and "mpg_mesh_set_edges" in str(e.value)
    # any other unknown location keeps its message, with and without edges
    for msh in (bare, mesh):
        for loc in (3, -1):
            refused(store(grid._h, msh._h, loc, 1, C.byref(h)), L.MPG_ERR_INVALID_ARG, "mesh location", "MPG_MESHLOC_NODE")
            assert "mpg_mesh_set_edges" not in lib.mpg_last_error().decode()
    bare.destroy()
