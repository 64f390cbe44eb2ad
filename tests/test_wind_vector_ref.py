"""The numpy mirror of the Cartesian-vector wind Regrid alone (target_grid.sphere_frames_at, wind_vector_blocks, wind_vector_apply), on
the CPU: the frames are orthonormal and right-handed, an identity handle with equal frames gives identity blocks, and the solid-body
rotation of unit speed about an axis tilted 45 degrees, through the weights of tests/_periodic_to_mesh_ref.py from 72 x 36 and 24 x 12
global grids onto the edges (un, ut) and the cells (ue, ve) of the 20 000-cell mesh, is a wind on the cap rows: there the vector route's
error does not exceed what the scalar route (two Regrids, then the rotation) leaves on its QUAD rows, while the scalar route's own cap
error exceeds 0.1."""
import numpy as np
import pytest

from _wind_vector_helpers import CAP_ROWS, solid_body_case, solid_body_errors

EPS = np.finfo(np.float64).eps


def _random_points(n, seed):
    rng = np.random.default_rng(seed)
    lon, lat = rng.uniform(-np.pi, np.pi, n), np.arcsin(rng.uniform(-1.0, 1.0, n))
    lon[:4], lat[:4] = (0.0, np.pi, -np.pi / 2, 1.0), (np.pi / 2, -np.pi / 2, 0.0, 0.0)      # the poles and the axes
    return lon, lat, rng.uniform(0.0, 2.0 * np.pi, n)


def test_frames_are_orthonormal_and_right_handed():
    from mpassit_amd import target_grid as tg
    lon, lat, phi = _random_points(5000, 1)
    rhat = np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)])
    for c, s in ((None, None), (np.cos(phi), np.sin(phi))):
        f = tg.sphere_frames_at(lon, lat, c, s)
        assert f.shape == (6, lon.size) and f.dtype == np.float64
        d0, d1 = f[:3], f[3:]
        assert np.abs((d0 * d0).sum(axis=0) - 1.0).max() <= 4 * EPS and np.abs((d1 * d1).sum(axis=0) - 1.0).max() <= 4 * EPS
        assert np.abs((d0 * d1).sum(axis=0)).max() <= 4 * EPS
        assert np.abs((d0 * rhat).sum(axis=0)).max() <= 4 * EPS and np.abs((d1 * rhat).sum(axis=0)).max() <= 4 * EPS
        assert np.abs(np.cross(d0, d1, axis=0) - rhat).max() <= 4 * EPS, "D0 x D1 is the outward radial"
    # without (c, s): east and north themselves
    f = tg.sphere_frames_at(lon, lat)
    assert np.array_equal(f[0], -np.sin(lon)) and np.array_equal(f[1], np.cos(lon)) and not f[2].any() and np.array_equal(f[5], np.cos(lat))
    with pytest.raises(ValueError):
        tg.sphere_frames_at(lon, lat, np.cos(phi), None)


def test_identity_handle_gives_identity_blocks():
    from mpassit_amd import target_grid as tg
    lon, lat, phi = _random_points(3000, 2)
    n = lon.size
    rowptr, col, val = np.arange(n + 1), np.arange(n), np.ones(n)
    for c, s in ((None, None), (np.cos(phi), np.sin(phi))):
        f = tg.sphere_frames_at(lon, lat, c, s)
        m = tg.wind_vector_blocks(rowptr, col, val, f, f)
        assert m.shape == (4, n)
        assert np.abs(m[0] - 1.0).max() <= 4 * EPS and np.abs(m[3] - 1.0).max() <= 4 * EPS
        assert np.abs(m[1]).max() <= 4 * EPS and np.abs(m[2]).max() <= 4 * EPS
        u, v = np.cos(3.0 * lon), np.sin(2.0 * lat)
        r0, r1 = tg.wind_vector_apply(rowptr, col, m, u, v)
        assert np.abs(r0 - u).max() <= 8 * EPS and np.abs(r1 - v).max() <= 8 * EPS
    # frames turned by phi on the destination side only: the blocks are the rotation by phi
    m = tg.wind_vector_blocks(rowptr, col, val, tg.sphere_frames_at(lon, lat), tg.sphere_frames_at(lon, lat, np.cos(phi), np.sin(phi)))
    for k, want in enumerate((np.cos(phi), np.sin(phi), -np.sin(phi), np.cos(phi))):
        assert np.abs(m[k] - want).max() <= 4 * EPS


@pytest.mark.parametrize("onto", ["edges", "cells"])
@pytest.mark.parametrize("grid", ["72x36", "24x12"])
def test_solid_body_rotation_is_a_wind_on_the_caps(oracle, global_mesh, grid, onto):
    from mpassit_amd import synth, target_grid as tg
    m = synth.mesh_edges(global_mesh)
    nx, ny = (73, 37) if grid == "72x36" else (25, 13)
    g = tg.define_target_grid_params("lat-lon", nx=nx, ny=ny, stand_lon=0.0, is_regional=False)
    case = solid_body_case(oracle, m, g, onto)
    ncap = int(case["cap"].sum())
    assert ncap == CAP_ROWS[(grid, onto)]
    assert int(case["quad"].sum()) == case["cap"].size - ncap
    s_quad, s_cap, v_quad, v_cap = solid_body_errors(case)
    print("%s -> %s: scalar route quad %.3g cap %.3g; vector route quad %.3g cap %.3g (%d cap rows)" % (grid, onto, s_quad, s_cap, v_quad, v_cap, ncap))
    assert v_cap <= s_quad, "the vector route's cap rows are worse than the scalar route's quad rows"
    assert s_cap > 0.1, "the scalar route's cap rows are not the row mean of each component: the check's inputs are wrong"
    # per component too, and with the margin of two that all four cases had when this was written
    for x, sc, e in zip(case["vector"], case["scalar"], case["exact"]):
        assert np.abs(x - e)[case["cap"]].max() <= np.abs(sc - e)[case["quad"]].max()
    assert 2.0 * v_cap <= s_quad and s_cap > 0.2
    # every row sums to one and the blocks carry it: |M_q| <= val[q]
    assert np.abs(case["blocks"]).max() <= np.abs(case["r"]["val"]).max() * (1.0 + 4 * EPS)
