"""CPU checks of the mesh edges the synthetic meshes derive (synth.mesh_edges) and of the numpy mirror of the edge angles
(target_grid.edge_rotang_at): the edge count of a closed mesh, cellsOnEdge and the direction of the normal on a global and a regional
mesh, angleEdge on a hand-made pair of cells, and phi = angleEdge - alpha against rotang_at."""
import numpy as np

from conftest import LAMBERT


def _normals(synth, m):
    """(edge points, unit normals rebuilt from angleEdge, centre 1, centre 2 or NaN) as unit vectors / 3-vectors"""
    p = synth.latlon_rad_to_xyz(m.latEdge, m.lonEdge)
    lat, lon = m.latEdge, m.lonEdge
    east = np.stack([-np.sin(lon), np.cos(lon), np.zeros_like(lon)], axis=1)
    north = np.stack([-np.sin(lat) * np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat)], axis=1)
    n = np.cos(m.angleEdge)[:, None] * east + np.sin(m.angleEdge)[:, None] * north
    cen = synth.latlon_rad_to_xyz(m.latCell, m.lonCell)
    c1 = cen[m.cellsOnEdge[:, 0] - 1]
    c2 = np.where((m.cellsOnEdge[:, 1] > 0)[:, None], cen[np.maximum(m.cellsOnEdge[:, 1] - 1, 0)], np.nan)
    return p, n, c1, c2


def test_fields_default_to_none():
    from mpassit_amd import synth
    m = synth.global_voronoi_mesh(200, seed=3)
    assert m.latEdge is None and m.lonEdge is None and m.angleEdge is None and m.cellsOnEdge is None and m.nEdges == 0


def test_global_mesh():
    from mpassit_amd import synth
    m0 = synth.global_voronoi_mesh(1500, seed=5)
    m = synth.mesh_edges(m0)
    assert m.latCell is m0.latCell and m.verticesOnCell is m0.verticesOnCell
    ne = m.nEdges
    assert ne == m.nCells + m.nVertices - 2, "Euler's formula on a closed mesh"
    assert m.lonEdge.shape == (ne,) and m.angleEdge.shape == (ne,) and m.cellsOnEdge.shape == (ne, 2) and m.cellsOnEdge.dtype == np.int32
    assert (m.cellsOnEdge >= 1).all() and (m.cellsOnEdge <= m.nCells).all(), "every edge of a closed mesh has two cells"
    assert (m.cellsOnEdge[:, 0] < m.cellsOnEdge[:, 1]).all(), "lower id first"
    assert (m.lonEdge >= 0).all() and (m.lonEdge < 2 * np.pi).all() and (np.abs(m.latEdge) <= np.pi / 2).all()
    p, n, c1, c2 = _normals(synth, m)
    assert np.abs(np.einsum("ij,ij->i", n, p)).max() < 1e-14, "the normal lies in the tangent plane"
    assert (np.einsum("ij,ij->i", n, c2 - c1) > 0).all(), "the normal points from cell 1 to cell 2"
    # the edge point is the midpoint of its two vertices: equidistant from both cells of a Voronoi mesh
    d1, d2 = np.linalg.norm(p - c1, axis=1), np.linalg.norm(p - c2, axis=1)
    assert np.abs(d1 - d2).max() < 1e-12
    # ascending (min vertex, max vertex) order: every cell's consecutive pairs are there, once
    voc = m.verticesOnCell
    pairs = set()
    for row in voc:
        r = row[row > 0]
        for a, b in zip(r, np.roll(r, -1)):
            pairs.add((min(a, b), max(a, b)))
    assert len(pairs) == ne


def test_regional_mesh_has_a_rim():
    from mpassit_amd import synth, target_grid as tg
    g = tg.define_target_grid_params("lambert", 61, 41, dx=30000.0, dy=30000.0, **LAMBERT)
    m = synth.mesh_edges(synth.regional_mesh_for_lambert(g.proj, 61, 41, 5003, margin=-0.08, seed=12))
    rim = m.cellsOnEdge[:, 1] == 0
    assert 0 < rim.sum() < m.nEdges / 10 and (m.cellsOnEdge[:, 0] >= 1).all()
    assert 2.9 * m.nCells < m.nEdges < 3.2 * m.nCells, "about three edges per cell"
    p, n, c1, c2 = _normals(synth, m)
    assert (np.einsum("ij,ij->i", n[rim], (p - c1)[rim]) > 0).all(), "a rim edge's normal points away from its cell"
    assert (np.einsum("ij,ij->i", n[~rim], (c2 - c1)[~rim]) > 0).all()


def test_angle_edge_on_a_hand_made_pair():
    """Two square cells on the equator that share one side: the neighbour to the east gives angleEdge = 0, the one to the north pi / 2."""
    from mpassit_amd import synth
    h = 0.01

    def pair(dlat, dlon):
        # cell 1 around (0, 0), cell 2 around (dlat, dlon); vertices: the corners of both squares, the shared side listed by both
        latc, lonc = np.array([0.0, dlat]), np.array([0.0, dlon])
        if dlon:        # east: the shared side is lon = h
            latv = np.array([-h, -h, h, h, -h, h])
            lonv = np.array([-h, h, h, -h, 3 * h, 3 * h])
            voc = np.array([[1, 2, 3, 4], [2, 5, 6, 3]], np.int32)
        else:           # north: the shared side is lat = h
            latv = np.array([-h, -h, h, h, 3 * h, 3 * h])
            lonv = np.array([-h, h, h, -h, h, -h])
            voc = np.array([[1, 2, 3, 4], [4, 3, 5, 6]], np.int32)
        return synth.mesh_edges(synth.MpasMesh(latc, lonc % (2 * np.pi), latv, lonv % (2 * np.pi), voc))

    for (dlat, dlon), want in (((0.0, 2 * h), 0.0), ((2 * h, 0.0), np.pi / 2)):
        m = pair(dlat, dlon)
        assert m.nEdges == 7
        shared = np.flatnonzero(m.cellsOnEdge[:, 1] > 0)
        assert shared.size == 1 and tuple(m.cellsOnEdge[shared[0]]) == (1, 2)
        assert abs(m.angleEdge[shared[0]] - want) < 1e-12, (m.angleEdge[shared[0]], want)
        # (the midpoint of the great circle between two points of latitude h lies O(h^3) = 5e-7 poleward of that latitude)
        lon = m.lonEdge[shared[0]]
        assert abs(m.latEdge[shared[0]] - dlat / 2) < 1e-6 and abs((lon + np.pi) % (2 * np.pi) - np.pi - dlon / 2) < 1e-12


def test_edge_rotang_at():
    from mpassit_amd import synth, target_grid as tg
    import pytest
    g = tg.define_target_grid_params("lambert", 61, 41, dx=30000.0, dy=30000.0, **LAMBERT)
    m = synth.mesh_edges(synth.regional_mesh_for_lambert(g.proj, 61, 41, 6001, margin=0.05, seed=11))
    theta, lon = m.angleEdge, np.degrees(m.lonEdge)
    cn, sn = tg.edge_rotang_at(None, lon, theta)
    assert np.array_equal(cn, np.cos(theta)) and np.array_equal(sn, np.sin(theta))
    cn, sn = tg.edge_rotang_at(g.proj, lon, theta)
    ca, sa = tg.rotang_at(g.proj, lon)
    assert np.abs(sa).max() > 0.05, "alpha matters on this mesh"
    # phi = theta - alpha, so theta = phi + alpha and the addition theorems carry a MINUS in the cosine, a PLUS in the sine (with the other
    # signs the sums would be cos / sin(theta - 2 alpha)); they recover cos / sin(theta) within 4 eps (two products and a sum of numbers <= 1, the
    # rounding of phi = theta - alpha, |phi| <= 2 pi, and of the four functions)
    eps = np.finfo(np.float64).eps
    ec, es = np.abs(cn * ca - sn * sa - np.cos(theta)).max(), np.abs(sn * ca + cn * sa - np.sin(theta)).max()
    print("cos / sin(phi + alpha) against cos / sin(theta): %.3g, %.3g (bound %.3g)" % (ec, es, 4 * eps))
    assert ec <= 4 * eps and es <= 4 * eps
    lat_lon = tg.define_target_grid_params("lat-lon", 81, 61, dx=0.25, dy=0.25, ref_lat=30.0, ref_lon=-110.0, ref_x=1.0, ref_y=1.0, stand_lon=-110.0)
    with pytest.raises(ValueError):
        tg.edge_rotang_at(lat_lon.proj, lon, theta)
