"""float64 references of the Stores between two grids (include/mpassit_amd.h, mpg_regrid_store_grid_to_grid and
mpg_regrid_store_conserve_grid_to_grid): a thin layer over the references of the Stores whose rules they state.

  bilinear, non-periodic source   _to_mesh_ref.to_mesh_bilinear on the destination stagger's points
  bilinear, periodic source       _periodic_to_mesh_ref.periodic_to_mesh
  nearest                         brute force: the smallest chord distance, the lowest source index on ties
  conservative                    _mesh_conserve_ref.polygons_of_grid / intersections / rows, area(d) = |fan area| of the CORNER quadrilateral

The cases are named grids from target_grid.define_target_grid_params with namelist counts.  One answer per (kind, grids, options) is
cached and never modified."""
import numpy as np

import _mesh_conserve_ref as CR
import _periodic_to_mesh_ref as PR
import _to_mesh_ref as TR
from conftest import LAMBERT

NORM_DSTAREA, NORM_FRACAREA = CR.NORM_DSTAREA, CR.NORM_FRACAREA
SLIVER, SLIVER_CAP = CR.SLIVER, CR.SLIVER_CAP
TIE_CAP = 1e-4            # at most 1 point in 10 000 may be an edge tie (tests/test_to_mesh_gpu.py)
CENTER, EDGE1, EDGE2, CORNER = 0, 1, 2, 3

CASES = {
    "L": (("lambert", 41, 31), dict(dx=30000.0, dy=30000.0, **LAMBERT)),
    "G": (("lat-lon", 61, 41), dict(dx=0.25, dy=0.25, ref_lat=40.07, ref_lon=-92.13)),
    "N": (("lambert", 37, 31), dict(dx=10000.0, dy=10000.0, ref_x=18.5, ref_y=15.5, **LAMBERT)),   # a 3 : 1 nest of L, corners on L's corners
    "A1": (("lat-lon", 25, 17), dict(dx=1.0, dy=1.0, ref_lat=40.0, ref_lon=-100.0)),
    "A2": (("lat-lon", 49, 33), dict(dx=0.5, dy=0.5, ref_lat=40.0, ref_lon=-100.0)),
    "W": (("lat-lon", 73, 37), dict(stand_lon=-180.0, is_regional=False)),
    "W2": (("lat-lon", 51, 27), dict(stand_lon=-171.3, is_regional=False)),
    "P": (("polar", 41, 41), dict(dx=100000.0, dy=100000.0, ref_lat=89.3, ref_lon=13.0, truelat1=60.0, stand_lon=-33.0)),
    "D": (("lambert", 41, 31), dict(dx=100000.0, dy=100000.0, ref_lat=45.3, ref_lon=179.2, truelat1=45.0, truelat2=45.0, stand_lon=179.2)),
}
_TARGETS, _XYZ, _ANSWERS = {}, {}, {}


def target(name):
    """The TargetGrid of case `name`, made once."""
    if name not in _TARGETS:
        from mpassit_amd import target_grid as tg
        args, kw = CASES[name]
        _TARGETS[name] = tg.define_target_grid_params(*args, **kw)
    return _TARGETS[name]


def stagger_lonlat(g, stagger):
    return {CENTER: (g.lon, g.lat), EDGE1: (g.lon_u, g.lat_u), EDGE2: (g.lon_v, g.lat_v), CORNER: (g.lon_c, g.lat_c)}[stagger]


def stagger_xyz(o, name, stagger=CENTER):
    """[sny][snx][3] unit vectors of a stagger's points of case `name` (the oracle's lon / lat -> xyz)."""
    key = (name, stagger)
    if key not in _XYZ:
        lon, lat = stagger_lonlat(target(name), stagger)
        x = o.lonlat_deg_to_xyz(lon, lat).reshape(lat.shape + (3,))
        x.setflags(write=False)
        _XYZ[key] = x
    return _XYZ[key]


def _cached(key, make):
    if key not in _ANSWERS:
        r = make()
        for a in (r.values() if isinstance(r, dict) else r):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _ANSWERS[key] = r
    return _ANSWERS[key]


def bilinear(o, src, dst, src_stagger=CENTER, dst_stagger=CENTER, tol=1e-10):
    """(idx [n][4], w [n][4], edge [n]) of the non-periodic bilinear Store src -> dst."""
    return _cached(("bil", src, dst, src_stagger, dst_stagger, tol),
                   lambda: TR.to_mesh_bilinear(stagger_xyz(o, src, src_stagger), stagger_xyz(o, dst, dst_stagger).reshape(-1, 3), tol=tol))


def periodic(o, src, dst, dst_stagger=CENTER, pole_method=PR.POLE_ALLAVG, mutate=None):
    """The dict of _periodic_to_mesh_ref.periodic_to_mesh for the CENTER points of the periodic grid `src` onto a stagger of `dst`."""
    return _cached(("per", src, dst, dst_stagger, pole_method, mutate),
                   lambda: PR.periodic_to_mesh(o, stagger_xyz(o, src, CENTER), stagger_xyz(o, dst, dst_stagger).reshape(-1, 3), pole_method=pole_method,
                                               mutate=mutate))


def nearest_brute(src_pts, dst_pts, chunk=2048):
    """[n] int32: the source point at the smallest squared chord distance (differences squared and summed x, y, z), lowest index on ties."""
    src_pts, dst_pts = np.asarray(src_pts, np.float64), np.asarray(dst_pts, np.float64)
    out = np.empty(dst_pts.shape[0], np.int32)
    for p0 in range(0, dst_pts.shape[0], chunk):
        d = dst_pts[p0:p0 + chunk, None, :] - src_pts[None, :, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        out[p0:p0 + chunk] = d2.argmin(axis=1)            # (argmin returns the first minimum: the lowest index)
    return out


def nearest(o, src, dst, src_stagger=CENTER, dst_stagger=CENTER):
    return _cached(("near", src, dst, src_stagger, dst_stagger),
                   lambda: (nearest_brute(stagger_xyz(o, src, src_stagger).reshape(-1, 3), stagger_xyz(o, dst, dst_stagger).reshape(-1, 3)),))[0]


def polygons(o, name, corners=None):
    """The cells of case `name` as polygons.  corners: None = the CORNER points from the oracle's lon / lat -> xyz; else a mapping name ->
    [(ny + 1) * (nx + 1)][3], the unit vectors a device grid holds (Grid.xyz: the bits its Stores read), so that both sides of a comparison
    clip the SAME polygons."""
    g = target(name)
    return CR.polygons_of_grid(stagger_xyz(o, name, CORNER).reshape(-1, 3) if corners is None else corners[name], g.nx, g.ny)


def cell_areas(o, name, corners=None):
    return _cached(("area", name, corners is not None), lambda: (np.abs(CR.fan_areas(*polygons(o, name, corners))),))[0]


def thin(o, name, corners=None):
    """h = area / diameter of every cell of case `name` that has an area."""
    xyz, _ = polygons(o, name, corners)
    a = cell_areas(o, name, corners)
    diam = np.linalg.norm(xyz[:, :, None, :] - xyz[:, None, :, :], axis=-1).max(axis=(1, 2))
    return (a / np.maximum(diam, 1e-300))[a > 0]


def tol_grids(o, src, dst, corners=None):
    """The project's conservative bar, max(1e-11, 64 eps / min h), h = area / diameter over BOTH grids' cells."""
    return max(1e-11, 64 * np.finfo(np.float64).eps / min(thin(o, src, corners).min(), thin(o, dst, corners).min()))


def conserve_pairs(o, src, dst, corners=None):
    """(d, s, I) over the cap pairs of the two grids' cells, d-major and s ascending within d."""
    return _cached(("inter", src, dst, corners is not None), lambda: CR.intersections(polygons(o, dst, corners), polygons(o, src, corners)))


def conserve(o, src, dst, norm=NORM_DSTAREA, corners=None):
    """(rowptr, col, val, frac) of the conservative Store src -> dst."""
    return _cached(("cons", src, dst, norm, corners is not None),
                   lambda: CR.rows(*conserve_pairs(o, src, dst, corners), cell_areas(o, dst, corners), norm))


def csr_of_fixed(idx, w):
    """A fixed handle's rows as CSR with columns ascending (zeros kept): what a periodic Store's quad rows look like."""
    mapped = idx[:, 0] >= 0
    order = np.argsort(idx, axis=1, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.where(mapped, idx.shape[1], 0))]).astype(np.int64)
    return rowptr, np.take_along_axis(idx, order, axis=1)[mapped].reshape(-1), np.take_along_axis(w, order, axis=1)[mapped].reshape(-1)
