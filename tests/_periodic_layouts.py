"""Global periodic grids in the layouts analyses come in, for the periodic Grid -> Mesh Store (tests/test_periodic_layouts_ref.py on the
CPU, tests/test_periodic_layouts_gpu.py on the GPU): rows numbered south to north and north to south (GRIB, ERA5, the IFS and JRA-55
Gaussian grids), uniform and Gaussian rows, rows on both poles, and a longitude origin away from 0.  The sizes are the smallest at which
both caps, the seam column and both candidate routes still occur.

A layout is a pair of 1-D arrays (lon [nx], lat [ny]) in degrees.  Every north-to-south layout is the SAME physical grid as its
south-to-north twin with the rows reversed, so the interpolation it gives must be the twin's: the twin's error on an analytic field is its
bound, and its handle with every column mapped by j -> ny - 1 - j is the twin's handle (`flip_rows`).

The analytic check compares an interpolated field with the field itself at the mesh points -- not with a restatement of the rule, which
could be wrong in the same way as the kernel."""
import numpy as np


def _gauss_lat(n):
    """Latitudes of the n-row Gaussian grid, ascending: the arcsines of the Gauss-Legendre nodes."""
    return np.degrees(np.arcsin(np.polynomial.legendre.leggauss(n)[0]))


LAYOUTS = {
    "s2n": (7.5 + 15.0 * np.arange(24), -82.5 + 15.0 * np.arange(12)),          # the case of tests/test_periodic_to_mesh_gpu.py
    "n2s": (7.5 + 15.0 * np.arange(24), 82.5 - 15.0 * np.arange(12)),           # a regular grid as GRIB stores it
    "poles_s2n": (15.0 * np.arange(24), -90.0 + 15.0 * np.arange(13)),          # rows on both poles: degenerate end quads, no cap points
    "poles_n2s": (15.0 * np.arange(24), 90.0 - 15.0 * np.arange(13)),           # ERA5 / GFS 0.25 degree ordering
    "gauss_s2n": (7.5 * np.arange(48), _gauss_lat(24)),                         # non-uniform rows
    "gauss_n2s": (7.5 * np.arange(48), _gauss_lat(24)[::-1].copy()),            # IFS / JRA-55 ordering
    "west": (-180.0 + 15.0 * np.arange(24), -82.5 + 15.0 * np.arange(12)),      # seam away from longitude 0
    "fine_s2n": (2.5 + 5.0 * np.arange(72), -87.5 + 5.0 * np.arange(36)),       # the twin of the next
    "fine_n2s": (2.5 + 5.0 * np.arange(72), 87.5 - 5.0 * np.arange(36)),        # index route with few cap points
}
TWIN = {"n2s": "s2n", "poles_n2s": "poles_s2n", "gauss_n2s": "gauss_s2n", "fine_n2s": "fine_s2n"}     # north to south -> south to north
UNIFORM = [k for k in LAYOUTS if not k.startswith("gauss")]          # a lat-lon projection describes these: they can take the index route
WITH_VERTICES = ("n2s", "gauss_n2s")                                 # layouts run on the mesh's vertices as well as on its cells

# (cap points, seam-quad points) the reference gives on the 20 000-cell global mesh, cells / vertices; a north-to-south layout has its twin's
COUNTS = {("s2n", 0): (169, 829), ("s2n", 1): (336, 1650), ("poles_s2n", 0): (0, 829), ("poles_s2n", 1): (0, 1664),
          ("gauss_s2n", 0): (94, 415), ("gauss_s2n", 1): (192, 831), ("west", 0): (169, 831), ("west", 1): (335, 1663),
          ("fine_s2n", 0): (19, 280), ("fine_s2n", 1): (39, 550)}
for _n, _s in TWIN.items():
    for _loc in (0, 1):
        COUNTS[(_n, _loc)] = COUNTS[(_s, _loc)]

FIELDS = ("z", "x", "1+z+xy")
# largest |interpolated - field| of the south-to-north layouts on the cells of that mesh, as the reference gave them (bilinear
# interpolation's own error on these coarse grids); "cap z": over the cap rows only.  Asserted with three digits' slack, 1.05 x.
S2N_ERRORS = {"s2n": {"z": 0.009242, "x": 0.01695, "1+z+xy": 0.0267, "cap z": 0.008497},
              "poles_s2n": {"z": 0.009303, "x": 0.01656, "1+z+xy": 0.02597, "cap z": None},
              "gauss_s2n": {"z": 0.004755, "x": 0.004176, "1+z+xy": 0.006625, "cap z": 0.004755},
              "west": {"z": 0.009249, "x": 0.01684, "1+z+xy": 0.02598, "cap z": 0.008497},
              "fine_s2n": {"z": 0.001036, "x": 0.001877, "1+z+xy": 0.003007, "cap z": 0.0008938}}


def coords(name):
    """-> (lon, lat) [ny][nx] in degrees"""
    lon, lat = LAYOUTS[name]
    return np.ascontiguousarray(np.broadcast_to(lon[None, :], (lat.size, lon.size))), np.ascontiguousarray(
        np.broadcast_to(lat[:, None], (lat.size, lon.size)))


def centers(oracle, name):
    """-> unit vectors of the CENTER points [ny][nx][3]"""
    lon, lat = coords(name)
    return oracle.lonlat_deg_to_xyz(lon, lat).reshape(lat.shape + (3,))


def proj(name):
    """The lat-lon projection of a layout with uniform rows (target_grid.Proj for Grid.attach_proj): point (0, 0) is the known point, index
    (1, 1) in the projection's 1-based numbering; latinc is negative where the rows run north to south."""
    from mpassit_amd import target_grid as tg
    lon, lat = LAYOUTS[name]
    return tg.Proj.latlon(float(lat[0]), float(lon[0]), 1.0, 1.0, float(lat[1] - lat[0]), float(lon[1] - lon[0]))


def fields(xyz):
    """The three analytic fields at unit vectors [..., 3] -> dict name -> [...]"""
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    return {"z": z, "x": x, "1+z+xy": 1.0 + z + x * y}


def apply_csr(rowptr, col, val, src):
    """A CSR matrix times one source vector, in numpy."""
    n = rowptr.size - 1
    return np.bincount(np.repeat(np.arange(n), np.diff(rowptr)), weights=val * src[col], minlength=n)


def field_errors(result, truth, cap_rows):
    """result, truth: dict field -> [n]; -> dict (field, "all" | "cap") -> largest |result - truth| over all rows / over cap_rows (a bool
    mask; None where it selects nothing)."""
    out = {}
    for f in FIELDS:
        d = np.abs(result[f] - truth[f])
        out[(f, "all")] = float(d.max())
        out[(f, "cap")] = float(d[cap_rows].max()) if cap_rows.any() else None
    return out


def twin_bounds(twin_errors):
    """The bound of a north-to-south layout: its twin's error times 1.01 plus 1e-12 -- the same grid, so only rounding may differ."""
    return {k: None if v is None else 1.01 * v + 1e-12 for k, v in twin_errors.items()}


def flip_rows(rowptr, col, val, nx, ny):
    """The same matrix with every column's grid row mapped by j -> ny - 1 - j, columns ascending within each row again."""
    col2 = (ny - 1 - col // nx) * nx + col % nx
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    order = np.lexsort((col2, rows))
    return rowptr, col2[order].astype(col.dtype), val[order]
