"""What the CPU and GPU tests of the Cartesian-vector wind Regrid share (test_wind_vector_ref.py, test_wind_vector_gpu.py): the solid-body
rotation of unit speed about an axis tilted 45 degrees through the reference weights of tests/_periodic_to_mesh_ref.py, by the scalar route
(two Regrids, then the rotation) and by the numpy mirror of the vector route, and its worst errors by row kind."""
import numpy as np

import _periodic_to_mesh_ref as PR

AXIS = np.array([np.sin(np.pi / 4), 0.0, np.cos(np.pi / 4)])
CAP_ROWS = {("72x36", "edges"): 57, ("72x36", "cells"): 19, ("24x12", "edges"): 505, ("24x12", "cells"): 169}


def solid_body_case(oracle, m, g, onto):
    """The solid-body case on one (grid, point set): a dict with the reference weights, the frames, the source winds, the analytic
    results `exact`, the scalar route's `scalar` and the vector route's `vector` (pairs: (un, ut) or (ue, ve)), and the row kinds."""
    from mpassit_amd import target_grid as tg
    cen = oracle.lonlat_deg_to_xyz(g.lon, g.lat).reshape(g.lat.shape + (3,))
    glon, glat = np.radians(g.lon).reshape(-1), np.radians(g.lat).reshape(-1)
    if onto == "edges":
        lon, lat = m.lonEdge, m.latEdge
        c, s = np.cos(m.angleEdge), np.sin(m.angleEdge)
    else:
        lon, lat = m.lonCell, m.latCell
        c = s = None
    pts = oracle.lonlat_deg_to_xyz(*oracle.mesh_coords_deg(lon, lat))
    sf, df = tg.sphere_frames_at(glon, glat), tg.sphere_frames_at(lon, lat, c, s)
    vel = np.cross(AXIS, cen.reshape(-1, 3))
    u, v = (vel * sf[:3].T).sum(axis=1), (vel * sf[3:].T).sum(axis=1)
    assert np.abs(np.hypot(u, v) - np.linalg.norm(vel, axis=1)).max() < 1e-14
    vp = np.cross(AXIS, pts)
    exact = ((vp * df[:3].T).sum(axis=1), (vp * df[3:].T).sum(axis=1))
    r = PR.periodic_to_mesh(oracle, cen, pts)
    n = pts.shape[0]
    rows = np.repeat(np.arange(n), np.diff(r["rowptr"]))
    a = np.bincount(rows, weights=r["val"] * u[r["col"]], minlength=n)
    b = np.bincount(rows, weights=r["val"] * v[r["col"]], minlength=n)
    scalar = (a, b) if c is None else (a * c + b * s, b * c - a * s)
    blocks = tg.wind_vector_blocks(r["rowptr"], r["col"], r["val"], sf, df)
    vector = tg.wind_vector_apply(r["rowptr"], r["col"], blocks, u, v)
    return dict(r=r, sf=sf, df=df, u=u, v=v, exact=exact, scalar=scalar, vector=vector, blocks=blocks,
                quad=r["kind"] == PR.KIND_QUAD, cap=r["kind"] == PR.KIND_CAP)


def solid_body_errors(case, got=None):
    """worst |result - exact| over both components: (scalar quad, scalar cap, vector quad, vector cap); got: results in place of the
    mirror's own vector route"""
    def worst(res, rows):
        return max(float(np.abs(x - e)[rows].max()) for x, e in zip(res, case["exact"]))
    vec = case["vector"] if got is None else got
    return worst(case["scalar"], case["quad"]), worst(case["scalar"], case["cap"]), worst(vec, case["quad"]), worst(vec, case["cap"])
