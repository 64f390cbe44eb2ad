"""CPU checks of the numpy side of the wind reconstruction from edge-normal u: synth.edges_on_cell against cellsOnEdge,
synth.reconstruct_coeffs (tangent results, the solid-body rotation and its convergence) and target_grid.reconstruct_blocks against
"Cartesian sum, then projection".  The measured errors are printed before they are held to their bars."""
import numpy as np
import pytest

import _wind_reconstruct_helpers as H


@pytest.fixture(scope="module")
def cases(global_mesh):
    from mpassit_amd import synth
    return {"global": H.mesh_case(global_mesh), "ico3": H.mesh_case(synth.icosahedral_mesh(3)), "ico5": H.mesh_case(synth.icosahedral_mesh(5))}


@pytest.mark.parametrize("name,lengths,nedges", [("ico3", {5, 6}, 1920), ("global", {4, 5, 6, 7, 8}, 59994)])
def test_edges_on_cell(cases, name, lengths, nedges):
    c = cases[name]
    m, n_on, eoc = c["m"], c["n_on"], c["eoc"]
    assert m.nEdges == nedges and set(n_on.tolist()) == lengths and eoc.shape == (m.nCells, max(lengths))
    assert n_on.dtype == np.int32 and eoc.dtype == np.int32
    valid = np.arange(eoc.shape[1])[None, :] < n_on[:, None]
    assert (eoc[~valid] == 0).all() and (eoc[valid] >= 1).all() and (eoc[valid] <= m.nEdges).all()
    # ascending within a cell
    pad = np.where(valid, eoc, np.iinfo(np.int32).max)
    assert (np.diff(pad.astype(np.int64), axis=1)[valid[:, 1:]] > 0).all()
    # every edge is listed by exactly the cells of cellsOnEdge
    cell = np.broadcast_to(np.arange(1, m.nCells + 1)[:, None], eoc.shape)[valid]
    got = sorted(zip(eoc[valid].tolist(), cell.tolist()))
    coe = np.asarray(m.cellsOnEdge)
    want = sorted((e + 1, int(cc)) for e in range(m.nEdges) for cc in coe[e] if cc > 0)
    assert got == want


def test_reconstruct_coeffs_docstring_and_tangency(cases):
    from mpassit_amd import synth
    assert "NOT MPAS's" in synth.reconstruct_coeffs.__doc__ and "coeffs_reconstruct" in synth.reconstruct_coeffs.__doc__
    rng = np.random.default_rng(5)
    for name in ("global", "ico3"):
        c = dict(cases[name])
        assert c["coeffs"].shape == c["eoc"].shape + (3,) and c["coeffs"].dtype == np.float64
        valid = np.arange(c["eoc"].shape[1])[None, :] < c["n_on"][:, None]
        assert (c["coeffs"][~valid] == 0.0).all()
        c["u"] = rng.uniform(-1.0, 1.0, c["m"].nEdges)
        V = H.cartesian(c)
        radial = np.abs((V * c["r"]).sum(axis=1)).max()
        print("%s: radial component of a reconstructed vector %.3e" % (name, radial))
        assert radial <= 1e-14


def test_solid_body_rotation(cases):
    err = {name: float(np.abs(H.cartesian(c) - c["exact"]).max()) for name, c in cases.items()}
    print("solid-body rotation, max component error: global %.3e  ico3 %.3e  ico5 %.3e" % (err["global"], err["ico3"], err["ico5"]))
    assert err["global"] <= 3.5e-3
    assert err["ico3"] <= 6.5e-3
    assert err["ico5"] < err["ico3"] / 3.0


def test_degenerate_cells_get_zero_coefficients(cases):
    from mpassit_amd import synth
    c = cases["ico3"]
    n_on = c["n_on"].copy()
    n_on[3] = 1          # one edge does not span the tangent plane
    n_on[7] = 0
    co = synth.reconstruct_coeffs(c["m"], n_on, c["eoc"])
    assert (co[3] == 0.0).all() and (co[7] == 0.0).all() and np.isfinite(co).all() and (co[4] != 0.0).any()


def test_blocks_equal_sum_then_projection(cases):
    from mpassit_amd import target_grid as tg
    rng = np.random.default_rng(11)
    for name in ("global", "ico3"):
        c = cases[name]
        m = c["m"]
        V = H.cartesian(c)
        val = np.ones(c["col"].size)
        ca, sa = np.cos(0.3 + m.lonCell), np.sin(0.3 + m.lonCell)
        for frames in (tg.sphere_frames_at(m.lonCell, m.latCell), tg.sphere_frames_at(m.lonCell, m.latCell, ca, sa)):
            mm = tg.reconstruct_blocks(c["rowptr"], c["coeffs"], val, frames)
            assert mm.shape == (2, c["col"].size)
            W = tg.reconstruct_apply(c["rowptr"], c["col"], mm, c["u"])
            for k in range(2):
                d = np.abs(W[k] - (V * frames[3 * k:3 * k + 3].T).sum(axis=1)).max()
                print("%s: blocks against sum-then-projection, component %d: %.3e" % (name, k, d))
                assert d <= 1e-14
        # the values scale the blocks, and a row longer than coeffs has slots is refused
        w = rng.uniform(0.5, 2.0, c["col"].size)
        assert np.array_equal(tg.reconstruct_blocks(c["rowptr"], c["coeffs"], w, None), w * tg.reconstruct_blocks(c["rowptr"], c["coeffs"], val, None))
        with pytest.raises(ValueError):
            tg.reconstruct_blocks(c["rowptr"], c["coeffs"][:, :3], val, None)
