"""CPU: the numpy restatement of the Grid -> Mesh bilinear rule (tests/_to_mesh_ref.py) is tied to the oracle.  On a 40 x 30 Lambert
grid the helper, fed the grid's own EDGE1 / EDGE2 points as "mesh points", must return the indices and weights of the oracle's
Grid -> Grid search (which looks at two quads per point; the helper looks at all of them); points built from a known quad and
(xi, eta) must come back in that quad with those coordinates; the weights of a mapped point sum to one."""
import numpy as np
import pytest

import _to_mesh_ref as TR
from conftest import LAMBERT

TOL_ORACLE = 1e-12     # tests/test_wind_oracle_gpu.py's bar for oracle.grid_bilinear on the 0.1-degree grid; a 30-km cell is coarser still


@pytest.fixture(scope="module")
def grid40x30():
    from mpassit_amd import target_grid as tg
    return tg.define_target_grid_params("lambert", 41, 31, dx=30000.0, dy=30000.0, **LAMBERT)


def test_helper_matches_oracle_grid_bilinear(oracle, grid40x30):
    g, o = grid40x30, oracle
    assert (g.nx, g.ny) == (40, 30)
    cen = o.lonlat_deg_to_xyz(g.lon, g.lat)
    for st, lon, lat in ((1, g.lon_u, g.lat_u), (2, g.lon_v, g.lat_v)):
        dxyz = o.lonlat_deg_to_xyz(lon, lat)
        oi, ow = o.grid_bilinear(g.nx, g.ny, cen, st, dxyz)
        hi, hw, edge = TR.to_mesh_bilinear(cen.reshape(g.ny, g.nx, 3), dxyz)
        assert (oi[:, 0] >= 0).sum() > 0.8 * oi.shape[0]
        assert np.array_equal(hi, oi)
        assert np.abs(hw - ow).max() < TOL_ORACLE
        m = hi[:, 0] >= 0
        assert np.abs(hw[m].sum(axis=1) - 1.0).max() < 1e-12
        assert np.isnan(edge[~m]).all() and (edge[m] >= -1e-10).all()
        # the index-estimate route of the helper (large grids) finds the same quads: a stagger point sits half a cell off a centre
        ii, jj = np.meshgrid(np.arange(lon.shape[1], dtype=np.float64), np.arange(lon.shape[0], dtype=np.float64))
        ci, cj = ii.reshape(-1) - (0.5 if st == 1 else 0.0), jj.reshape(-1) - (0.5 if st == 2 else 0.0)
        ci_, cw_, _ = TR.to_mesh_bilinear(cen.reshape(g.ny, g.nx, 3), dxyz, cand=(ci, cj))
        assert np.array_equal(ci_, hi) and np.array_equal(cw_, hw)


def test_points_of_a_known_quad_come_back(oracle, grid40x30):
    g, o = grid40x30, oracle
    cen = o.lonlat_deg_to_xyz(g.lon, g.lat).reshape(g.ny, g.nx, 3)
    rng = np.random.default_rng(7)
    n = 500
    a, b = rng.integers(0, g.nx - 1, n), rng.integers(0, g.ny - 1, n)
    xi, eta = rng.uniform(0.02, 0.98, n), rng.uniform(0.02, 0.98, n)
    A, B, C, D = cen[b, a], cen[b, a + 1], cen[b + 1, a + 1], cen[b + 1, a]
    X = A + (B - A) * xi[:, None] + (D - A) * eta[:, None] + ((A - B) + (C - D)) * (xi * eta)[:, None]
    P = X / np.linalg.norm(X, axis=1)[:, None]
    idx, w, edge = TR.to_mesh_bilinear(cen, P)
    iA = b * g.nx + a
    assert np.array_equal(idx, np.stack([iA, iA + 1, iA + 1 + g.nx, iA + g.nx], axis=1))
    want = np.stack([(1 - xi) * (1 - eta), xi * (1 - eta), xi * eta, (1 - xi) * eta], axis=1)
    assert np.abs(w - want).max() < 1e-12
    assert np.abs(edge - np.minimum(np.minimum(xi, 1 - xi), np.minimum(eta, 1 - eta))).max() < 1e-12
    assert np.abs(w.sum(axis=1) - 1.0).max() < 1e-12
    # a point off the grid is unmapped
    far = o.lonlat_deg_to_xyz(np.array([10.0]), np.array([-40.0]))
    fi, fw, fe = TR.to_mesh_bilinear(cen, far)
    assert (fi == -1).all() and (fw == 0.0).all() and np.isnan(fe).all()
