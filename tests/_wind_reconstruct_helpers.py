"""What the CPU and GPU tests of the wind reconstruction from edge-normal u share (test_wind_reconstruct_ref.py,
test_wind_reconstruct_gpu.py): a mesh with its edges, edgesOnCell, the stand-in coefficients and the CSR pattern; the solid-body rotation of
unit speed about an axis tilted 45 degrees as edge-normal u; and a Python copy of the tile plan the kernel takes its level chunks from."""
import numpy as np

AXIS = np.array([np.sin(np.pi / 4), 0.0, np.cos(np.pi / 4)])


def mesh_case(m):
    """dict: the mesh with edges, nEdgesOnCell / edgesOnCell, coeffs [nCells][maxEdges][3], the CSR pattern (rowptr, col 0-based, file slot
    order), the solid-body u at the edges and the exact Cartesian wind at the centres."""
    from mpassit_amd import synth, target_grid as tg
    m = synth.mesh_edges(m)
    n_on, eoc = synth.edges_on_cell(m)
    coeffs = synth.reconstruct_coeffs(m, n_on, eoc)
    rowptr = np.concatenate([[0], np.cumsum(n_on)]).astype(np.int64)
    col = eoc[np.arange(eoc.shape[1])[None, :] < n_on[:, None]].astype(np.int64) - 1
    pe = synth.latlon_rad_to_xyz(m.latEdge, m.lonEdge)
    ne = tg.sphere_frames_at(m.lonEdge, m.latEdge, np.cos(m.angleEdge), np.sin(m.angleEdge))[:3].T     # the edge normals
    u = (np.cross(AXIS, pe) * ne).sum(axis=1)
    r = synth.latlon_rad_to_xyz(m.latCell, m.lonCell)
    return dict(m=m, n_on=n_on, eoc=eoc, coeffs=coeffs, rowptr=rowptr, col=col, u=u, r=r, exact=np.cross(AXIS, r))


def cartesian(case, coeffs=None):
    """[nCells][3]: the reconstructed Cartesian wind of the case's u through the numpy mirror"""
    from mpassit_amd import target_grid as tg
    mm = tg.reconstruct_blocks(case["rowptr"], case["coeffs"] if coeffs is None else coeffs, np.ones(case["col"].size), None)
    return tg.reconstruct_apply(case["rowptr"], case["col"], mm, case["u"]).T


# ---- the tile plan (apply_mesh.h am_tile_plan), so that the level sweep can find its thresholds instead of copying them ----
AM_CELLS, AM_TILE_BYTES = 64, 64 * 1024


def tile_plan_kc(nlev, esz, ntiles):
    """levels per chunk of `ntiles` [cell][lev] tiles of element size esz: nlev when all levels fit"""
    cap = AM_TILE_BYTES // ntiles
    if AM_CELLS * (nlev | 1) * esz > cap:
        return (cap // (AM_CELLS * esz) - 1) // 32 * 32
    return nlev


def tile_thresholds():
    """{(esz, ntiles): the largest level count that still fits one chunk} for 2 and 3 tiles of float32 and float64"""
    out = {}
    for esz in (4, 8):
        for nt in (2, 3):
            k = 1
            while tile_plan_kc(k + 1, esz, nt) == k + 1:
                k += 1
            out[(esz, nt)] = k
    return out
