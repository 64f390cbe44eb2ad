"""Target-grid coordinates from namelist parameters (host side, numpy, float64).

Mirrors what the reference computes on the host before the hot path runs:
`define_target_grid_params` (model_grid.F90:644-1201) -> `get_lat_lon_fields` (:2188-2219) ->
`xytoll` (llxy_module.F90:166-216) -> `ij_to_latlon` (module_map_utils.F90:629-679; Lambert
:1160-1233 with `set_lc` :1083-1121 / `lc_cone` :1124-1157; lat-lon :1398-1428), plus `get_rotang`
(model_grid.F90:2450-2507) and the namelist-derived sizes of `read_setup_namelist`
(program_setup.F90:87-249: i_target = nx-1, j_target = ny-1, default known point = domain centre).

These coordinates are INPUTS of the HIP kernels ("generation is out of scope for HIP
but must be reproduced"); parity is pinned by the compiled-reference goldens of SURVEY App. E
(tests/golden/projection_lc.json).
"""
from dataclasses import dataclass, field

import numpy as np

PI = 3.141592653589793  # constants_module.F90:8
RAD_PER_DEG = PI / 180.0
DEG_PER_RAD = 180.0 / PI
EARTH_RADIUS_M = 6370000.0  # constants_module.F90:25
NAN = 1.0e20  # misc_definitions_module.F90:12 (namelist "unset" sentinel)

PROJ_LATLON, PROJ_LC, PROJ_PS, PROJ_MERC = 0, 1, 2, 3  # misc_definitions_module.F90:38-42
M, U, V, CORNER = 1, 2, 3, 6  # misc_definitions_module.F90:29


def _wrap180(x):
    it = 0
    while abs(x) > 180.0 and it < 10:
        if x < -180.0:
            x += 360.0
        if x > 180.0:
            x -= 360.0
        it += 1
    return x


@dataclass
class Proj:
    """`proj_info` subset (module_map_utils.F90:140-192) for PROJ_LC, PROJ_LATLON, PROJ_PS and PROJ_MERC."""
    code: int
    lat1: float = 0.0
    lon1: float = 0.0
    knowni: float = 0.0
    knownj: float = 0.0
    dx: float = 0.0
    stdlon: float = 0.0
    truelat1: float = 0.0
    truelat2: float = 0.0
    hemi: float = 1.0
    cone: float = 0.0
    polei: float = 0.0
    polej: float = 0.0
    rsw: float = 0.0
    rebydx: float = 0.0
    latinc: float = 0.0
    loninc: float = 0.0
    nxmin: int = 1
    nxmax: int = 0
    dlon: float = 0.0

    @staticmethod
    def lc_cone(truelat1, truelat2):
        if abs(truelat1 - truelat2) > 0.1:
            cone = np.log10(np.cos(truelat1 * RAD_PER_DEG)) - np.log10(np.cos(truelat2 * RAD_PER_DEG))
            cone = cone / (np.log10(np.tan((45.0 - abs(truelat1) / 2.0) * RAD_PER_DEG))
                           - np.log10(np.tan((45.0 - abs(truelat2) / 2.0) * RAD_PER_DEG)))
            return float(cone)
        return float(np.sin(abs(truelat1) * RAD_PER_DEG))

    @classmethod
    def lambert(cls, truelat1, truelat2, stdlon, lat1, lon1, knowni, knownj, dx):
        p = cls(PROJ_LC, lat1=lat1, lon1=_wrap180(lon1), knowni=knowni, knownj=knownj, dx=dx,
                stdlon=_wrap180(stdlon), truelat1=truelat1, truelat2=truelat2)
        p.hemi = -1.0 if truelat1 < 0.0 else 1.0
        p.rebydx = EARTH_RADIUS_M / dx
        if abs(p.truelat2) > 90.0:
            p.truelat2 = p.truelat1
        p.cone = cls.lc_cone(p.truelat1, p.truelat2)
        deltalon1 = p.lon1 - p.stdlon
        if deltalon1 > 180.0:
            deltalon1 -= 360.0
        if deltalon1 < -180.0:
            deltalon1 += 360.0
        ctl1r = np.cos(p.truelat1 * RAD_PER_DEG)
        p.rsw = float(p.rebydx * ctl1r / p.cone *
                      (np.tan((90.0 * p.hemi - p.lat1) * RAD_PER_DEG / 2.0) /
                       np.tan((90.0 * p.hemi - p.truelat1) * RAD_PER_DEG / 2.0)) ** p.cone)
        arg = p.cone * (deltalon1 * RAD_PER_DEG)
        p.polei = float(p.hemi * p.knowni - p.hemi * p.rsw * np.sin(arg))
        p.polej = float(p.hemi * p.knownj + p.rsw * np.cos(arg))
        return p

    @classmethod
    def polar(cls, truelat1, stdlon, lat1, lon1, knowni, knownj, dx):
        """map_set(PROJ_PS) + set_ps (module_map_utils.F90:682-715), arguments as push_source_projection passes them
        (llxy_module.F90:123-132)."""
        p = cls(PROJ_PS, lat1=lat1, lon1=_wrap180(lon1), knowni=knowni, knownj=knownj, dx=dx, stdlon=_wrap180(stdlon), truelat1=truelat1)
        p.hemi = -1.0 if truelat1 < 0.0 else 1.0
        p.rebydx = EARTH_RADIUS_M / dx
        reflon = p.stdlon + 90.0
        scale_top = 1.0 + p.hemi * np.sin(p.truelat1 * RAD_PER_DEG)
        ala1 = p.lat1 * RAD_PER_DEG
        p.rsw = float(p.rebydx * np.cos(ala1) * scale_top / (1.0 + p.hemi * np.sin(ala1)))
        alo1 = (p.lon1 - reflon) * RAD_PER_DEG
        p.polei = float(p.knowni - p.rsw * np.cos(alo1))
        p.polej = float(p.knownj - p.hemi * p.rsw * np.sin(alo1))
        return p

    @classmethod
    def mercator(cls, truelat1, lat1, lon1, knowni, knownj, dx):
        """map_set(PROJ_MERC) + set_merc (module_map_utils.F90:1293-1317; llxy_module.F90:71-79)."""
        p = cls(PROJ_MERC, lat1=lat1, lon1=_wrap180(lon1), knowni=knowni, knownj=knownj, dx=dx, truelat1=truelat1)
        p.hemi = -1.0 if truelat1 < 0.0 else 1.0
        p.rebydx = EARTH_RADIUS_M / dx
        clain = np.cos(RAD_PER_DEG * truelat1)
        p.dlon = float(dx / (EARTH_RADIUS_M * clain))
        p.rsw = 0.0
        if lat1 != 0.0:
            p.rsw = float(np.log(np.tan(0.5 * ((lat1 + 90.0) * RAD_PER_DEG))) / p.dlon)
        return p

    @classmethod
    def latlon(cls, lat1, lon1, knowni, knownj, latinc, loninc):
        return cls(PROJ_LATLON, lat1=lat1, lon1=_wrap180(lon1), knowni=knowni, knownj=knownj,
                   latinc=latinc, loninc=loninc, nxmin=1, nxmax=int(round(360.0 / loninc)))

    # -- ij_to_latlon, vectorised over numpy arrays of (i, j) in grid-index units (1-based)
    def ij_to_latlon(self, i, j):
        i = np.asarray(i, np.float64)
        j = np.asarray(j, np.float64)
        if self.code == PROJ_LC:
            chi1 = (90.0 - self.hemi * self.truelat1) * RAD_PER_DEG
            chi2 = (90.0 - self.hemi * self.truelat2) * RAD_PER_DEG
            xx = self.hemi * i - self.polei
            yy = self.polej - self.hemi * j
            r2 = xx * xx + yy * yy
            r = np.sqrt(r2) / self.rebydx
            lon = self.stdlon + DEG_PER_RAD * np.arctan2(self.hemi * xx, yy) / self.cone
            lon = np.fmod(lon + 360.0, 360.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                if chi1 == chi2:
                    chi = 2.0 * np.arctan((r / np.tan(chi1)) ** (1.0 / self.cone) * np.tan(chi1 * 0.5))
                else:
                    chi = 2.0 * np.arctan((r * self.cone / np.sin(chi1)) ** (1.0 / self.cone) * np.tan(chi1 * 0.5))
            lat = (90.0 - chi * DEG_PER_RAD) * self.hemi
            pole = r2 == 0.0
            lat = np.where(pole, self.hemi * 90.0, lat)
            lon = np.where(pole, self.stdlon, lon)
            lon = np.where(lon > 180.0, lon - 360.0, lon)
            lon = np.where(lon < -180.0, lon + 360.0, lon)
            return lat, lon
        if self.code == PROJ_PS:                      # ijll_ps (module_map_utils.F90:763-822)
            reflon = self.stdlon + 90.0
            scale_top = 1.0 + self.hemi * np.sin(self.truelat1 * RAD_PER_DEG)
            xx = i - self.polei
            yy = (j - self.polej) * self.hemi
            r2 = xx * xx + yy * yy
            gi2 = (self.rebydx * scale_top) ** 2.0
            with np.errstate(divide="ignore", invalid="ignore"):
                lat = DEG_PER_RAD * self.hemi * np.arcsin((gi2 - r2) / (gi2 + r2))
                arccos = np.arccos(np.clip(xx / np.sqrt(r2), -1.0, 1.0))
            lon = np.where(yy > 0, reflon + DEG_PER_RAD * arccos, reflon - DEG_PER_RAD * arccos)
            pole = r2 == 0.0
            lat = np.where(pole, self.hemi * 90.0, lat)
            lon = np.where(pole, reflon, lon)
            lon = np.where(lon > 180.0, lon - 360.0, lon)
            lon = np.where(lon < -180.0, lon + 360.0, lon)
            return lat, lon
        if self.code == PROJ_MERC:                    # ijll_merc (:1344-1362)
            lat = 2.0 * np.arctan(np.exp(self.dlon * (self.rsw + j - self.knownj))) * DEG_PER_RAD - 90.0
            lon = (i - self.knowni) * self.dlon * DEG_PER_RAD + self.lon1
            lon = np.where(lon > 180.0, lon - 360.0, lon)
            lon = np.where(lon < -180.0, lon + 360.0, lon)
            return lat, lon
        span = float(self.nxmax - self.nxmin + 1)
        i_work = np.where(i < self.nxmin - 0.5, i + span, i)
        i_work = np.where(i >= self.nxmax + 0.5, i - span, i_work)
        lat = self.lat1 + (j - self.knownj) * self.latinc
        lon = self.lon1 + (i_work - self.knowni) * self.loninc
        return lat, lon

    def latlon_to_ij(self, lat, lon):
        """llij_lc (module_map_utils.F90:1236-1290), llij_ps (:718-760), llij_merc (:1320-1341); used by the synthetic
        meshes and the round-trip tests."""
        lat = np.asarray(lat, np.float64)
        lon = np.asarray(lon, np.float64)
        if self.code == PROJ_PS:
            reflon = self.stdlon + 90.0
            scale_top = 1.0 + self.hemi * np.sin(self.truelat1 * RAD_PER_DEG)
            ala = lat * RAD_PER_DEG
            rm = self.rebydx * np.cos(ala) * scale_top / (1.0 + self.hemi * np.sin(ala))
            alo = (lon - reflon) * RAD_PER_DEG
            return self.polei + rm * np.cos(alo), self.polej + self.hemi * rm * np.sin(alo)
        if self.code == PROJ_MERC:
            deltalon = lon - self.lon1
            deltalon = np.where(deltalon < -180.0, deltalon + 360.0, deltalon)
            deltalon = np.where(deltalon > 180.0, deltalon - 360.0, deltalon)
            i = self.knowni + (deltalon / (self.dlon * DEG_PER_RAD))
            j = self.knownj + np.log(np.tan(0.5 * ((lat + 90.0) * RAD_PER_DEG))) / self.dlon - self.rsw
            return i, j
        assert self.code == PROJ_LC
        deltalon = lon - self.stdlon
        deltalon = np.where(deltalon > 180.0, deltalon - 360.0, deltalon)
        deltalon = np.where(deltalon < -180.0, deltalon + 360.0, deltalon)
        ctl1r = np.cos(self.truelat1 * RAD_PER_DEG)
        rm = self.rebydx * ctl1r / self.cone * (np.tan((90.0 * self.hemi - lat) * RAD_PER_DEG / 2.0) /
                                                np.tan((90.0 * self.hemi - self.truelat1) * RAD_PER_DEG / 2.0)) ** self.cone
        arg = self.cone * (deltalon * RAD_PER_DEG)
        i = self.hemi * (self.polei + self.hemi * rm * np.sin(arg))
        j = self.hemi * (self.polej - rm * np.cos(arg))
        return i, j

    def xytoll(self, x, y, stagger=M):
        x = np.asarray(x, np.float64)
        y = np.asarray(y, np.float64)
        if stagger == U:
            x = x - 0.5
        elif stagger == V:
            y = y - 0.5
        elif stagger == CORNER:
            x, y = x - 0.5, y - 0.5
        return self.ij_to_latlon(x, y)

    def lat_lon_fields(self, ni, nj, stagger):
        """get_lat_lon_fields: arrays [nj][ni] (i fastest) for 1-based points (i, j)."""
        jj, ii = np.meshgrid(np.arange(1, nj + 1, dtype=np.float64), np.arange(1, ni + 1, dtype=np.float64), indexing="ij")
        return self.xytoll((ii - 0.5) + 0.5, (jj - 0.5) + 0.5, stagger)


def get_map_factor(proj, xlat):
    """MAPFAC at the points with latitude xlat (get_map_factor, model_grid.F90:2229-2365): Lambert (one or two true
    latitudes), polar stereographic, Mercator; lat-lon has no branch there (1.0 here, like the device kernel)."""
    xlat = np.asarray(xlat, np.float64)
    if proj.code == PROJ_LC:
        colat = RAD_PER_DEG * (90.0 - xlat)
        if proj.truelat1 != proj.truelat2:
            colat1, colat2 = RAD_PER_DEG * (90.0 - proj.truelat1), RAD_PER_DEG * (90.0 - proj.truelat2)
            n = (np.log(np.sin(colat1)) - np.log(np.sin(colat2))) / (np.log(np.tan(colat1 / 2.0)) - np.log(np.tan(colat2 / 2.0)))
            return np.sin(colat2) / np.sin(colat) * (np.tan(colat / 2.0) / np.tan(colat2 / 2.0)) ** n
        colat0 = RAD_PER_DEG * (90.0 - proj.truelat1)
        return np.sin(colat0) / np.sin(colat) * (np.tan(colat / 2.0) / np.tan(colat0 / 2.0)) ** np.cos(colat0)
    if proj.code == PROJ_PS:
        return (1.0 + np.sin(RAD_PER_DEG * abs(proj.truelat1))) / (1.0 + np.sin(RAD_PER_DEG * np.copysign(1.0, proj.truelat1) * xlat))
    if proj.code == PROJ_MERC:
        return np.sin(RAD_PER_DEG * (90.0 - proj.truelat1)) / np.sin(RAD_PER_DEG * (90.0 - xlat))
    return np.ones_like(xlat)


def get_rotang(xlat, xlon):
    """cos/sin of the grid rotation angle, arrays [nj][ni] (model_grid.F90:2450-2507)."""
    nj = xlat.shape[0]
    jm = np.maximum(np.arange(nj) - 1, 0)
    jp = np.minimum(np.arange(nj) + 1, nj - 1)
    d_lon = xlon[jp, :] - xlon[jm, :]
    d_lon = np.where(d_lon > 180.0, d_lon - 360.0, np.where(d_lon < -180.0, d_lon + 360.0, d_lon))
    alpha = np.arctan2(-np.cos(xlat * RAD_PER_DEG) * (d_lon * RAD_PER_DEG), (xlat[jp, :] - xlat[jm, :]) * RAD_PER_DEG)
    return np.cos(alpha), np.sin(alpha)


def rotang_at(proj, lon_deg):
    """(cosa, sina) of a Lambert grid's rotation angle at ANY longitude (degrees; scalar or array), in closed form: alpha =
    -hemi * cone * wrap180(lon - stand_lon) * pi / 180, get_rotang's sign convention (the +j axis of the grid points along the meridian
    turned by cone * (lon - stand_lon)).  The host mirror of mpg_mesh_rotang_dev; on a 30-km grid it meets get_rotang's centred
    differences to 2.3e-6 in sina on the interior rows.  PROJ_LC only."""
    if proj.code != PROJ_LC:
        raise ValueError("rotang_at: cos/sin(alpha) exist for PROJ_LC only; the forward chain does not rotate elsewhere")
    d = np.asarray(lon_deg, dtype=np.float64) - proj.stdlon
    for _ in range(2):
        d = np.where(d > 180.0, d - 360.0, np.where(d < -180.0, d + 360.0, d))
    alpha = -proj.hemi * proj.cone * d * RAD_PER_DEG
    return np.cos(alpha), np.sin(alpha)


def rotate_winds_transpose_at(cosa, sina, gu, gv):
    """The host mirror of mpg_rotate_winds_transpose_dev: the adjoint of rotate_winds_cgrid (interp.F90:737-748) on the gradients gu, gv
    ([nlev][ny][nx] or [ny][nx], float64) with cosa / sina [ny][nx] reused over the levels.  The same float64 operations in the same
    order as the kernel, each rounded once (numpy contracts nothing): the same bits.  Returns new arrays (guo, gvo)."""
    ca, sa = np.asarray(cosa, dtype=np.float64), np.asarray(sina, dtype=np.float64)
    gun, gvn = np.asarray(gu, dtype=np.float64), np.asarray(gv, dtype=np.float64)
    with np.errstate(all="ignore"):
        tana = sa / ca
        den = ca + sa * tana
        a = gvn / ca
        t = a * sa
        b = gun - t
        guo = b / den
        p = guo * tana
        gvo = a + p
    return guo, gvo


def edge_rotang_at(proj, lon_deg, angle_edge):
    """(cn, sn) = cos / sin of phi = angle_edge - alpha at mesh edges: alpha as rotang_at at the edges' longitudes (degrees), angle_edge
    the MPAS angleEdge (radians) -- the rotation to earth-relative winds and the projection onto the edge normal as ONE rotation.  The
    host mirror of mpg_mesh_edge_rotang_dev.  proj=None: alpha = 0 (winds that are earth-relative already); else PROJ_LC only."""
    theta = np.asarray(angle_edge, dtype=np.float64)
    if proj is None:
        phi = theta - 0.0
    else:
        if proj.code != PROJ_LC:
            raise ValueError("edge_rotang_at: cos/sin(alpha) exist for PROJ_LC only; the forward chain does not rotate elsewhere: pass proj=None")
        d = np.asarray(lon_deg, dtype=np.float64) - proj.stdlon
        for _ in range(2):
            d = np.where(d > 180.0, d - 360.0, np.where(d < -180.0, d + 360.0, d))
        phi = theta - (-proj.hemi * proj.cone * d * RAD_PER_DEG)
    return np.cos(phi), np.sin(phi)


def sphere_frames_at(lon, lat, c=None, s=None):
    """The local frames of n points on the sphere (lon, lat in RADIANS) as a [6][n] float64 array, the planes D0x D0y D0z D1x D1y D1z:
    east = (-sin lon, cos lon, 0), north = (-sin lat cos lon, -sin lat sin lon, cos lat).  c, s both None: D0 = east, D1 = north
    (earth-relative winds); else D0 = c east + s north, D1 = c north - s east, every product and sum an operation of its own -- rotang_at's
    (cosa, sina) for the grid-relative winds of a Lambert grid, cos / sin of angleEdge for (normal, tangent) at mesh edges,
    edge_rotang_at's (cn, sn) for both at once.  The host mirror of mpg_sphere_frames_dev (which it meets to the device's sin / cos)."""
    if (c is None) != (s is None):
        raise ValueError("sphere_frames_at: c and s come together (both None: east and north)")
    lon, lat = np.asarray(lon, dtype=np.float64).reshape(-1), np.asarray(lat, dtype=np.float64).reshape(-1)
    sl, cl, sp, cp = np.sin(lon), np.cos(lon), np.sin(lat), np.cos(lat)
    east = np.stack([-sl, cl, np.zeros_like(sl)])
    north = np.stack([-sp * cl, -sp * sl, cp])
    if c is None:
        return np.concatenate([east, north])
    c, s = np.asarray(c, dtype=np.float64).reshape(1, -1), np.asarray(s, dtype=np.float64).reshape(1, -1)
    return np.concatenate([c * east + s * north, c * north - s * east])


def wind_vector_blocks(rowptr, col, val, src_frames, dst_frames):
    """The 2 x 2 blocks m[4][nnz] (planes m00 m01 m10 m11, CSR entry order) of a Cartesian-vector Regrid through the CSR weights
    (rowptr, col, val): for entry q of row p with c = col[q], e / n the source frame at c and D0 / D1 the destination frame at p,
        m00 = val[q] * ((e.x*D0.x + e.y*D0.y) + e.z*D0.z)      m01 = val[q] * ((n.x*D0.x + n.y*D0.y) + n.z*D0.z)
    and m10, m11 the same against D1 -- (r0, r1) at p = sum_q M_q (u, v)[col[q]].  numpy rounds every operation and contracts nothing:
    mpg_wind_vector_weights_dev gives these bits."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    val, sf, df = np.asarray(val, dtype=np.float64), np.asarray(src_frames, dtype=np.float64), np.asarray(dst_frames, dtype=np.float64)
    row = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    e, n = sf[0:3][:, col], sf[3:6][:, col]
    m = np.empty((4, col.size))
    for k, d in enumerate((df[0:3][:, row], df[3:6][:, row])):
        m[2 * k] = val * ((e[0] * d[0] + e[1] * d[1]) + e[2] * d[2])
        m[2 * k + 1] = val * ((n[0] * d[0] + n[1] * d[1]) + n[2] * d[2])
    return m


def wind_vector_apply(rowptr, col, m, u, v):
    """(r0, r1) [n_dst] of one level: r_k = sum over the row's entries of m_k0 u[col] + m_k1 v[col] (the blocks of wind_vector_blocks; float64
    sums by np.bincount, not in the device's order: a reference for values, not for bits)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n = rowptr.size - 1
    row = np.repeat(np.arange(n), np.diff(rowptr))
    uu, vv = np.asarray(u, dtype=np.float64).reshape(-1)[col], np.asarray(v, dtype=np.float64).reshape(-1)[col]
    return tuple(np.bincount(row, weights=m[2 * k] * uu, minlength=n) + np.bincount(row, weights=m[2 * k + 1] * vv, minlength=n)
                 for k in range(2))


def reconstruct_blocks(rowptr, coeffs, val, dst_frames):
    """The values m[nout][nnz] (CSR entry order) of the wind reconstruction from edge-normal u (MPAS's mpas_reconstruct) through the
    pattern rowptr of edgesOnCell: for entry q of row c, slot i = q - rowptr[c] and (cx, cy, cz) = coeffs[c][i][:] (coeffs
    [nCells][maxEdges][3], the file's coeffs_reconstruct),
        frames [6][nCells]:  m0 = val[q] * ((cx*D0.x + cy*D0.y) + cz*D0.z)     m1 the same against D1          (nout = 2)
        dst_frames None:     m_k = val[q] * c_k,  k = X, Y, Z                                                   (nout = 3)
    numpy rounds every operation and contracts nothing: mpg_reconstruct_weights_dev gives these bits."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    coeffs, val = np.asarray(coeffs, dtype=np.float64), np.asarray(val, dtype=np.float64)
    n = np.diff(rowptr)
    if n.size and n.max(initial=0) > coeffs.shape[1]:
        raise ValueError("reconstruct_blocks: the longest row has %d entries, coeffs has %d slots" % (n.max(), coeffs.shape[1]))
    row = np.repeat(np.arange(rowptr.size - 1), n)
    slot = np.arange(row.size) - rowptr[row]
    c = coeffs[row, slot].T                                   # [3][nnz]
    if dst_frames is None:
        return np.stack([val * c[0], val * c[1], val * c[2]])
    df = np.asarray(dst_frames, dtype=np.float64)
    return np.stack([val * ((c[0] * d[0] + c[1] * d[1]) + c[2] * d[2]) for d in (df[0:3][:, row], df[3:6][:, row])])


def reconstruct_apply(rowptr, col, m, u):
    """The results [nout][n_dst] of one level: r_k = sum over the row's entries of m_k u[col] (float64 sums by np.bincount, not in the
    device's order: a reference for values, not for bits)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n = rowptr.size - 1
    row = np.repeat(np.arange(n), np.diff(rowptr))
    uu = np.asarray(u, dtype=np.float64).reshape(-1)[col]
    return np.stack([np.bincount(row, weights=mk * uu, minlength=n) for mk in m])


def fixed_to_csr(idx, w=None):
    """(rowptr, col, val) of a fixed handle's weights() -- idx [n_dst][nnz_per_row] with -1 = no entry, w the same shape or None (a nearest
    handle: every value 1.0): the slots of a row in their order, the -1 entries dropped.  What mpg_handle_compose reads of a fixed operand."""
    idx = np.asarray(idx, dtype=np.int64)
    idx = idx.reshape(idx.shape[0], -1)
    keep = idx >= 0
    rowptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    val = np.ones(idx.shape) if w is None else np.asarray(w, dtype=np.float64).reshape(idx.shape)
    return rowptr, idx[keep].astype(np.int32), np.ascontiguousarray(val[keep])


EXTRAPMETHOD_NEAREST_STOD, EXTRAPMETHOD_NEAREST_IDAVG = 1, 2


def extrapolate_neighbours(src_xyz, dst_xyz, rows, K):
    """The K nearest sources of the destination points `rows` by brute force -> (ids [n][K] int32, d2 [n][K]): per point a lexsort on
    (d2, id) with d2 = (dx*dx + dy*dy) + dz*dz in float64, dist2_nofma's expression; ties go to the lower id at every rank.  (The sort
    runs over the sources at or below the point's K-th smallest d2: every tie at the last rank is among them.)"""
    src_xyz, dst_xyz = np.asarray(src_xyz, np.float64), np.asarray(dst_xyz, np.float64)
    rows = np.asarray(rows, np.int64)
    n_src = src_xyz.shape[1]
    K = min(int(K), n_src)
    ids, d2k = np.full((rows.size, K), -1, np.int32), np.zeros((rows.size, K))
    if rows.size == 0 or K == 0:
        return ids, d2k
    step = max(1, (1 << 22) // n_src)
    for a in range(0, rows.size, step):
        p = dst_xyz[:, rows[a:a + step]]
        dx, dy, dz = (p[k][:, None] - src_xyz[k][None, :] for k in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        kth = np.partition(d2, K - 1, axis=1)[:, K - 1]
        for u in range(d2.shape[0]):
            cand = np.flatnonzero(d2[u] <= kth[u])
            order = cand[np.lexsort((cand, d2[u][cand]))[:K]]
            ids[a + u] = order
            d2k[a + u] = d2[u][order]
    return ids, d2k


def extrapolate_weights(d2k, method=EXTRAPMETHOD_NEAREST_STOD, dist_exponent=2.0):
    """The value rule of mpg_handle_extrapolate for rows of K ascending squared distances d2k [n][K] -> (rowlen [n] int32, w [n][K] with
    0.0 behind a row's end).  STOD, K == 1 or d2_0 == 0: one entry of weight 1; else r_i = d2_0 / d2_i, t_i = r_i (e == 2) or
    r_i ** (e / 2), S = ((t_0 + t_1) + ...) from left to right, w_i = t_i / S, every operation rounded on its own."""
    d2k = np.asarray(d2k, np.float64)
    n, K = d2k.shape
    rowlen, w = np.zeros(n, np.int32), np.zeros((n, K))
    if n == 0 or K == 0:
        return rowlen, w
    one = np.full(n, method != EXTRAPMETHOD_NEAREST_IDAVG) | (d2k[:, 0] == 0.0) | (K == 1)
    rowlen[:] = np.where(one, 1, K)
    w[:, 0] = 1.0
    many = np.flatnonzero(~one)
    if many.size:
        r = d2k[many, :1] / d2k[many]
        t = r if dist_exponent == 2.0 else np.power(r, 0.5 * dist_exponent)
        S = t[:, 0].copy()
        for i in range(1, K):
            S = S + t[:, i]
        w[many] = t / S[:, None]
    return rowlen, w


def extrapolate_rows(src_xyz, dst_xyz, unmapped, method=EXTRAPMETHOD_NEAREST_STOD, num_src_pnts=8, dist_exponent=2.0):
    """The numpy mirror of mpg_handle_extrapolate's new rows, by brute force.  src_xyz [3][n_src], dst_xyz [3][n_dst]: the library's stored
    unit vectors (Mesh.xyz / Grid.xyz); unmapped: the rows to fill (a bool mask of n_dst, or row numbers).  Per row, in ascending row order:
    the K = min(N, n_src) nearest sources by a lexsort on (d2, id), d2 = (dx*dx + dy*dy) + dz*dz in float64 (dist2_nofma's expression),
    N = 1 for STOD (extrapolate_neighbours); the weights of extrapolate_weights.
    -> (rowlen [nu] int32, ids [nu][K] int32 with -1 behind a row's end, w [nu][K] with 0.0 there)."""
    unmapped = np.asarray(unmapped)
    rows = np.flatnonzero(unmapped) if unmapped.dtype == bool else np.sort(unmapped.astype(np.int64))
    if method not in (EXTRAPMETHOD_NEAREST_STOD, EXTRAPMETHOD_NEAREST_IDAVG):
        raise ValueError("extrapolate_rows: unknown method")
    ids, d2k = extrapolate_neighbours(src_xyz, dst_xyz, rows, int(num_src_pnts) if method == EXTRAPMETHOD_NEAREST_IDAVG else 1)
    rowlen, w = extrapolate_weights(d2k, method, dist_exponent)
    ids[np.arange(ids.shape[1])[None, :] >= rowlen[:, None]] = -1
    return rowlen, ids, w


MASKRULE_ROW, MASKRULE_ENTRY = 1, 2
NORM_DSTAREA, NORM_FRACAREA = 0, 1


def mask_rows(rowptr, col, val, frac, src_mask, dst_mask, rule, norm_type=NORM_DSTAREA):
    """The numpy mirror of mpg_handle_mask on a CSR pattern (a fixed handle: fixed_to_csr of its weights(); its rows that come back empty
    are the ones the call writes as idx -1, w +0.0).  frac: dst_frac [n] or None; src_mask / dst_mask: bool or uint8, None = no mask;
    rule: MASKRULE_ROW or MASKRULE_ENTRY (no AUTO here: a pattern records no method).
    A destination-masked row is empty (frac' +0.0).  ROW: a row with an entry on a masked source is empty (frac' +0.0), every other row is
    copied.  ENTRY: the entries of masked sources go; Wk = ((0.0 + v_0) + v_1) + ... over the kept values in stored order; DSTAREA: values
    unchanged, frac' = Wk; FRACAREA: w' = w / Wk, frac' = frac * Wk; nothing kept or not Wk > 0: empty, frac' = +0.0; a row with no masked
    entry is copied verbatim with its frac.
    -> (rowptr int64, col int32, val, frac' or None, stats): stats = [mapped rows the source rule unmapped, mapped rows the destination
    mask unmapped, entries removed], mpg_handle_store_stats [1..3]."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64).reshape(-1)
    val = np.asarray(val, dtype=np.float64).reshape(-1)
    n = rowptr.size - 1
    if rule not in (MASKRULE_ROW, MASKRULE_ENTRY):
        raise ValueError("mask_rows: rule must be MASKRULE_ROW or MASKRULE_ENTRY")
    if rule == MASKRULE_ENTRY and norm_type not in (NORM_DSTAREA, NORM_FRACAREA):
        raise ValueError("mask_rows: unknown norm_type")
    sm = np.zeros(int(col.max()) + 1 if col.size else 0, bool) if src_mask is None else np.asarray(src_mask).reshape(-1) != 0
    dm = np.zeros(n, bool) if dst_mask is None else np.asarray(dst_mask).reshape(-1) != 0
    had = np.diff(rowptr)
    row = np.repeat(np.arange(n), had)
    hit = sm[col]                                                   # per entry: its source is masked
    nhit = np.bincount(row, weights=hit, minlength=n).astype(np.int64)
    fin = np.zeros(n) if frac is None else np.asarray(frac, dtype=np.float64).reshape(-1)
    fout = fin.copy()
    keep = ~dm[row]
    newval = val.copy()
    if rule == MASKRULE_ROW:
        keep &= (nhit == 0)[row]
    else:
        keep &= ~hit
        # Wk per row over the kept entries, left to right: pass t adds every row's t-th kept entry
        live = ~hit
        rank = np.cumsum(live) - 1
        first = np.concatenate([[0], np.cumsum(np.bincount(row, weights=live, minlength=n).astype(np.int64))])[:-1]
        rank = rank - first[row]                                     # position among the row's kept entries (meaningful where live)
        nkept = had - nhit
        Wk = np.zeros(n)
        for t in range(int(nkept.max()) if n else 0):
            sel = np.flatnonzero(live & (rank == t))
            Wk[row[sel]] = Wk[row[sel]] + val[sel]
        touched = nhit > 0
        dead = touched & ((nkept == 0) | ~(Wk > 0.0))
        keep &= ~dead[row]
        scale = touched & ~dead
        if norm_type == NORM_FRACAREA:
            with np.errstate(all="ignore"):
                newval = np.where(scale[row], val / np.where(scale, Wk, 1.0)[row], val)
            fout = np.where(scale, fin * Wk, fout)
        else:
            fout = np.where(scale, Wk, fout)
        fout = np.where(dead, 0.0, fout)
    now = np.bincount(row, weights=keep, minlength=n).astype(np.int64)
    if rule == MASKRULE_ROW:
        fout = np.where((had > 0) & (now == 0) & ~dm, 0.0, fout)
    fout = np.where(dm, 0.0, fout)
    out_rowptr = np.concatenate([[0], np.cumsum(now)]).astype(np.int64)
    stats = [int(((had > 0) & (now == 0) & ~dm).sum()), int(((had > 0) & dm).sum()), int(had.sum() - now.sum())]
    return out_rowptr, col[keep].astype(np.int32), np.ascontiguousarray(newval[keep]), (None if frac is None else fout), stats


def extrapolate_rows_masked(src_xyz, dst_xyz, unmapped, src_mask, method=EXTRAPMETHOD_NEAREST_STOD, num_src_pnts=8, dist_exponent=2.0):
    """The numpy mirror of mpg_handle_extrapolate_masked's new rows, by brute force: extrapolate_rows over the compacted unmasked sources
    (ascending id, so the (d2, id) order and its ties are those of the unmasked ids), the ids mapped back.  src_mask: bool or uint8 of
    n_src, None = nothing masked.  `unmapped`: the rows to fill -- the caller leaves the dst_skip rows out.  K = min(N, unmasked sources);
    with every source masked the rows come back with length 0.  -> (rowlen, ids, w) as extrapolate_rows."""
    src_xyz = np.asarray(src_xyz, np.float64)
    if src_mask is None:
        return extrapolate_rows(src_xyz, dst_xyz, unmapped, method, num_src_pnts, dist_exponent)
    live = np.flatnonzero(np.asarray(src_mask).reshape(-1) == 0)
    rowlen, ids, w = extrapolate_rows(src_xyz[:, live], dst_xyz, unmapped, method, num_src_pnts, dist_exponent)
    back = np.where(ids >= 0, live[np.maximum(ids, 0)] if live.size else -1, -1).astype(np.int32) if ids.size else ids
    return rowlen, back, w


DTOS_SUM, DTOS_MEAN = 0, 1


def nearest_dtos_rows(src_xyz, dst_xyz, norm=DTOS_SUM, src_mask=None, dst_mask=None):
    """The numpy mirror of mpg_regrid_store_nearest_dtos, by brute force.  src_xyz [3][n_src], dst_xyz [3][n_dst]: the library's stored unit
    vectors (Mesh.xyz / Grid.xyz); src_mask / dst_mask: bool or uint8, non-zero = masked, None = nothing masked.  For every unmasked source
    nearest = the first of a lexsort on (d2, id) over the unmasked destinations, d2 = (dx*dx + dy*dy) + dz*dz in float64 (dist2_nofma's
    expression): a tie goes to the lower id; -1 for a masked source and when every destination is masked.  The sources are visited in
    chunks, so that memory stays small.  Row d holds the sources with nearest == d in ascending id; DTOS_SUM: every value 1.0, DTOS_MEAN:
    1.0 / len(d), one float64 division.  -> (rowptr [n_dst + 1] int64, col int32, val float64, nearest [n_src] int32)."""
    if norm not in (DTOS_SUM, DTOS_MEAN):
        raise ValueError("nearest_dtos_rows: unknown norm")
    src_xyz, dst_xyz = np.asarray(src_xyz, np.float64).reshape(3, -1), np.asarray(dst_xyz, np.float64).reshape(3, -1)
    n_src, n_dst = src_xyz.shape[1], dst_xyz.shape[1]
    live_s = np.arange(n_src) if src_mask is None else np.flatnonzero(np.asarray(src_mask).reshape(-1) == 0)
    live_d = np.arange(n_dst) if dst_mask is None else np.flatnonzero(np.asarray(dst_mask).reshape(-1) == 0)
    nearest = np.full(n_src, -1, np.int32)
    if live_s.size and live_d.size:
        q = dst_xyz[:, live_d]
        step = max(1, (1 << 22) // live_d.size)
        for a in range(0, live_s.size, step):
            rows = live_s[a:a + step]
            p = src_xyz[:, rows]
            dx, dy, dz = (p[k][:, None] - q[k][None, :] for k in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            lo = d2.min(axis=1)
            for u in range(rows.size):
                cand = np.flatnonzero(d2[u] <= lo[u])            # every tie at the first rank is among them
                nearest[rows[u]] = live_d[cand[np.lexsort((live_d[cand], d2[u][cand]))[0]]]
    mapped = np.flatnonzero(nearest >= 0)
    order = mapped[np.argsort(nearest[mapped], kind="stable")]   # by destination, ascending source id inside a row
    cnt = np.bincount(nearest[mapped], minlength=n_dst).astype(np.int64)
    rowptr = np.zeros(n_dst + 1, np.int64)
    np.cumsum(cnt, out=rowptr[1:])
    col = order.astype(np.int32)
    if norm == DTOS_MEAN:
        val = np.float64(1.0) / np.repeat(cnt[cnt > 0], cnt[cnt > 0]).astype(np.float64)
    else:
        val = np.ones(col.size, np.float64)
    return rowptr, col, np.ascontiguousarray(val, dtype=np.float64), nearest


CREEP_ALL_LEVELS = 0x7fffffff


def creep_neighbours_grid(snx, sny):
    """Nb(p) of mpg_handle_creep on a grid stagger of snx x sny points, id = j * snx + i: the points of [i - 1, i + 1] x [j - 1, j + 1]
    inside the grid, p itself excluded, ascending; no shift and no wrap.  -> (nbr [n][8] int32 with -1 behind a row's end, cnt [n])."""
    snx, sny = int(snx), int(sny)
    j, i = np.divmod(np.arange(snx * sny, dtype=np.int64), snx)
    cols = []
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            if di == 0 and dj == 0:
                continue
            a, b = i + di, j + dj
            cols.append(np.where((a >= 0) & (a < snx) & (b >= 0) & (b < sny), b * snx + a, _PATCH_NONE))
    cand = np.sort(np.stack(cols, axis=1), axis=1)
    return np.where(cand != _PATCH_NONE, cand, -1).astype(np.int32), (cand != _PATCH_NONE).sum(axis=1)


def creep_neighbours_mesh(voc, tri):
    """Nb(p) of mpg_handle_creep on a mesh's cells: patch_neighbours_mesh's N1(p) minus p, ascending (the cells that share a valid dual
    triangle with p).  A cell without verticesOnCell entries has none.  -> (nbr [nCells][K] int32 with -1 behind a row's end, cnt)."""
    n1, cnt, _ = patch_neighbours_mesh(voc, tri)
    if (cnt > PATCH_MAX_PNTS).any():
        raise ValueError("creep_neighbours_mesh: a ring of more than %d cells" % PATCH_MAX_PNTS)
    cand = np.where((n1 >= 0) & (n1 != np.arange(n1.shape[0])[:, None]), n1.astype(np.int64), _PATCH_NONE)
    cand = np.sort(cand, axis=1)[:, :max(n1.shape[1] - 1, 1)]
    return np.where(cand != _PATCH_NONE, cand, -1).astype(np.int32), (cand != _PATCH_NONE).sum(axis=1)


def creep_rows(rowptr, col, val, neighbours, num_levels=CREEP_ALL_LEVELS, dst_skip=None):
    """The numpy mirror of mpg_handle_creep on a CSR pattern (a fixed handle: fixed_to_csr of its weights()).  neighbours: (nbr, cnt) of
    creep_neighbours_grid / creep_neighbours_mesh; dst_skip: bool or uint8 of n_dst, None = none.
    level[p] = 0 for a non-empty row; an empty row with dst_skip never gets a level; for L = 1 .. num_levels an empty, unskipped row
    without a level gets level L iff a neighbour has level L - 1, and the loop ends at the first L that assigns nothing.  The row of a
    point of level L: its contributors are the neighbours of level L - 1 in ascending id, m of them; the columns are the ascending distinct
    union of theirs; a column's value is acc = acc + v from 0.0 over the contributors in ascending id and, within one, over its entries
    with that column in stored order, then acc / float(m) -- every operation rounded on its own.
    -> (level [n] int32 with -1 = no level, rowptr int64, col int32, val)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64).reshape(-1)
    val = np.asarray(val, dtype=np.float64).reshape(-1)
    nbr, cnt = neighbours
    nbr = np.asarray(nbr, dtype=np.int64)
    n = rowptr.size - 1
    nbr = nbr.reshape(n, -1)
    if int(num_levels) < 1:
        raise ValueError("creep_rows: num_levels must be >= 1")
    skip = np.zeros(n, bool) if dst_skip is None else np.asarray(dst_skip).reshape(-1) != 0
    level = np.where(np.diff(rowptr) > 0, 0, -1).astype(np.int32)
    rows = [None] * n                                                # (col, val) of the filled rows
    open_ = (level < 0) & ~skip
    L = 0
    while L < int(num_levels) and open_.any():
        L += 1
        cand = np.flatnonzero(open_)
        nb = nbr[cand]
        has = (nb >= 0) & (level[np.maximum(nb, 0)] == L - 1)
        front = cand[has.any(axis=1)]
        if front.size == 0:
            break
        new = {}
        for p, q_all, h in zip(front, nb[has.any(axis=1)], has[has.any(axis=1)]):
            Q = q_all[h]                                             # ascending: nbr is
            cc, vv = [], []
            for q in Q:
                if level[q] == 0:
                    cc.append(col[rowptr[q]:rowptr[q + 1]])
                    vv.append(val[rowptr[q]:rowptr[q + 1]])
                else:
                    cc.append(rows[q][0])
                    vv.append(rows[q][1])
            cc, vv = np.concatenate(cc), np.concatenate(vv)
            order = np.argsort(cc, kind="stable")                    # a column's terms stay in (contributor, stored) order
            sc, sv = cc[order], vv[order]
            head = np.ones(sc.size, bool)
            head[1:] = sc[1:] != sc[:-1]
            gid = np.cumsum(head) - 1
            first = np.flatnonzero(head)
            rank = np.arange(sc.size) - first[gid]
            acc = np.zeros(first.size)
            for t in range(int(rank.max()) + 1):
                sel = rank == t
                acc[gid[sel]] = acc[gid[sel]] + sv[sel]
            new[p] = (sc[first], acc / float(Q.size))
        for p, r in new.items():                                     # a level reads only the level below it
            rows[p] = r
        level[front] = L
        open_[front] = False
    lens = np.diff(rowptr).copy()
    filled = np.flatnonzero(level > 0)
    for p in filled:
        lens[p] = rows[p][0].size
    out_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    out_col, out_val = np.empty(out_ptr[-1], np.int32), np.empty(out_ptr[-1])
    mapped = np.repeat(level == 0, np.diff(rowptr))
    keep = np.repeat(level == 0, lens)
    out_col[keep], out_val[keep] = col[mapped], val[mapped]
    for p in filled:
        out_col[out_ptr[p]:out_ptr[p + 1]], out_val[out_ptr[p]:out_ptr[p + 1]] = rows[p]
    return level, out_ptr, out_col, out_val


REGRIDMETHOD_PATCH = 3
PATCH_MAX_PNTS = 32
_PATCH_NONE = np.iinfo(np.int64).max
_PATCH_TOL = 2.0 ** -26


def _patch_pack(cand):
    """Rows of candidate ids (_PATCH_NONE = no candidate) -> (nbr [n][K] int32 ascending and distinct, -1 behind a row's end;
    cnt [n], PATCH_MAX_PNTS + 1 for a row that holds more than PATCH_MAX_PNTS)."""
    cand = np.sort(np.asarray(cand, np.int64), axis=1)
    dup = np.zeros(cand.shape, bool)
    dup[:, 1:] = cand[:, 1:] == cand[:, :-1]
    cand[dup] = _PATCH_NONE
    cand = np.sort(cand, axis=1)
    cnt = (cand != _PATCH_NONE).sum(axis=1)
    width = min(max(int(cnt.max()) if cnt.size else 1, 1), PATCH_MAX_PNTS)
    head = cand[:, :width]
    return np.where(head != _PATCH_NONE, head, -1).astype(np.int32), np.minimum(cnt, PATCH_MAX_PNTS + 1)


def patch_neighbours_mesh(voc, tri):
    """The ring-1 patches of a mesh's cells for patch_rows.  voc: verticesOnCell [nCells][maxEdges], 1-based and 0-padded; tri: the dual
    triangles [nVertices][3] (Mesh.triangles(): cell ids, -1 = none).  N1(c) = c and the three cells of every valid triangle of every
    listed vertex of c, ascending.  -> (nbr [nCells][K] int32 with -1 behind a row's end, cnt [nCells], True): True = a mesh, whose nodes
    may fall back on the ring-2 patch."""
    voc = np.asarray(voc, np.int64)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    nC, mE = voc.shape
    v = voc - 1
    listed = (v >= 0) & (v < tri.shape[0])
    t = tri[np.where(listed, v, 0)]
    ok = listed & (t >= 0).all(axis=2)
    cand = np.where(ok[:, :, None], t, _PATCH_NONE).reshape(nC, mE * 3)
    nbr, cnt = _patch_pack(np.concatenate([np.arange(nC, dtype=np.int64)[:, None], cand], axis=1))
    return nbr, cnt, True


def patch_neighbours_grid(snx, sny):
    """The ring-1 patches of a grid stagger of snx x sny points, id = j * snx + i: the window [i0, i0 + 2] x [j0, j0 + 2] cut to the grid,
    i0 = clamp(i - 1, 0, max(snx - 3, 0)), j0 likewise.  -> (nbr [n][K] int32, cnt [n], False): no ring-2 patch on a grid."""
    snx, sny = int(snx), int(sny)
    j, i = np.divmod(np.arange(snx * sny, dtype=np.int64), snx)
    i0, j0 = np.clip(i - 1, 0, max(snx - 3, 0)), np.clip(j - 1, 0, max(sny - 3, 0))
    cols = []
    for dj in range(3):
        for di in range(3):
            a, b = i0 + di, j0 + dj
            cols.append(np.where((a < snx) & (b < sny), b * snx + a, _PATCH_NONE))
    nbr, cnt = _patch_pack(np.stack(cols, axis=1))
    return nbr, cnt, False


def _patch_dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _patch_frame(X):
    """e1, e2 [3][m] of the frames about the unit vectors X [3][m], patch.h's pt_frame."""
    ax = np.argmin(np.abs(X), axis=0)                       # the lowest axis on ties
    a = [(ax == k).astype(np.float64) for k in range(3)]
    s = _patch_dot(a, X)
    t = [a[k] - s * X[k] for k in range(3)]
    r = np.sqrt(_patch_dot(t, t))
    e1 = [t[k] / r for k in range(3)]
    e2 = [X[1] * e1[2] - X[2] * e1[1], X[2] * e1[0] - X[0] * e1[2], X[0] * e1[1] - X[1] * e1[0]]
    return e1, e2


def _patch_phi(u, v, M):
    return [np.ones_like(u), u, v] + ([u * u, u * v, v * v] if M == 6 else [])


def _patch_uv(X, e1, e2, h, Q, gnomonic=False):
    if gnomonic:                                            # (a mutant of the tests: the point scaled onto the tangent plane first)
        qn = _patch_dot(Q, X)
        Q = [Q[k] / qn for k in range(3)]
    d = [Q[k] - X[k] for k in range(3)]
    return _patch_dot(d, e1) / h, _patch_dot(d, e2) / h


def _patch_fit(src_xyz, nodes, pat, M, gnomonic=False):
    """pt_fit<M> of patch.h for the nodes [m] on their patches pat [m][K] (-1 = none) -> (passes [m], fit): frame, h, G summed in patch
    order, the thresholded Cholesky in place."""
    m, K = pat.shape
    X = [src_xyz[k][nodes] for k in range(3)]
    e1, e2 = _patch_frame(X)
    valid = pat >= 0
    safe = np.where(valid, pat, 0)
    hm = np.zeros(m)
    for k in range(K):
        d = [src_xyz[c][safe[:, k]] - X[c] for c in range(3)]
        dd = _patch_dot(d, d)
        hm = np.where(valid[:, k] & (dd > hm), dd, hm)
    h = np.sqrt(hm)
    R = [[np.zeros(m) for _ in range(M)] for _ in range(M)]
    for k in range(K):
        u, v = _patch_uv(X, e1, e2, h, [src_xyz[c][safe[:, k]] for c in range(3)], gnomonic)
        phi = _patch_phi(u, v, M)
        for a in range(M):
            for b in range(a, M):
                R[a][b] = np.where(valid[:, k], R[a][b] + phi[a] * phi[b], R[a][b])
    ok = h > 0.0
    for k in range(M):
        g = R[k][k]
        p = g
        for i in range(k):
            p = p - R[i][k] * R[i][k]
        ok = ok & (p > _PATCH_TOL * g)
        r = np.sqrt(p)
        R[k][k] = r
        for j in range(k + 1, M):
            t = R[k][j]
            for i in range(k):
                t = t - R[i][k] * R[i][j]
            R[k][j] = t / r
    return ok, (X, e1, e2, h, R)


def _patch_shape(src_xyz, fit, sel, pat, P, M, gnomonic=False):
    """pt_shape<M> of patch.h: fit rows `sel` (one per pair), their patches pat [n][K], the destination points P [3][n] -> L [n][K]."""
    X, e1, e2, h, R = fit
    X, e1, e2, h = [x[sel] for x in X], [x[sel] for x in e1], [x[sel] for x in e2], h[sel]
    R = [[R[a][b][sel] for b in range(M)] for a in range(M)]
    u, v = _patch_uv(X, e1, e2, h, P, gnomonic)
    y = _patch_phi(u, v, M)
    for k in range(M):
        t = y[k]
        for i in range(k):
            t = t - R[i][k] * y[i]
        y[k] = t / R[k][k]
    for k in range(M - 1, -1, -1):
        t = y[k]
        for j in range(k + 1, M):
            t = t - R[k][j] * y[j]
        y[k] = t / R[k][k]
    n, K = pat.shape
    safe = np.where(pat >= 0, pat, 0)
    L = np.zeros((n, K))
    for k in range(K):
        u, v = _patch_uv(X, e1, e2, h, [src_xyz[c][safe[:, k]] for c in range(3)], gnomonic)
        phi = _patch_phi(u, v, M)
        acc = np.zeros(n)
        for a in range(M):
            acc = acc + phi[a] * y[a]
        L[:, k] = acc
    return L


def _patch_rows(idx, w, src_xyz, dst_xyz, neighbours, degree2=True, ring2=True, blend=True, gnomonic=False):
    """patch_rows with the switches of the mutation tests (tests/test_patch_ref.py): degree2 False = degree 1 everywhere, ring2 False = no
    attempt B, blend False = the polynomial of the row's heaviest slot alone, gnomonic True = gnomonic local coordinates."""
    idx = np.asarray(idx, np.int64)
    idx = idx.reshape(idx.shape[0], -1)
    w = np.asarray(w, np.float64).reshape(idx.shape)
    src_xyz, dst_xyz = np.asarray(src_xyz, np.float64), np.asarray(dst_xyz, np.float64)
    nbr, cnt, is_mesh = neighbours
    nbr, cnt = np.asarray(nbr, np.int64), np.asarray(cnt, np.int64)
    n_dst, S = idx.shape
    n_src = src_xyz.shape[1]
    take = (idx >= 0) & (idx[:, :1] >= 0)
    if not blend:
        top = np.argmax(np.where(take, w, -np.inf), axis=1)
        take &= np.arange(S)[None, :] == top[:, None]
    prow, pslot = np.nonzero(take)                              # row-major: (row, slot) ascending
    pnode, pb = idx[prow, pslot], (w[prow, pslot] if blend else np.ones(prow.size))
    nodes, inv = np.unique(pnode, return_inverse=True)
    att = np.full(nodes.size, 3, np.int8)
    K1 = nbr.shape[1]
    pat = np.full((nodes.size, PATCH_MAX_PNTS), -1, np.int64)
    pat[:, 0] = nodes
    fits = {}
    with np.errstate(all="ignore"):
        p1, c1 = nbr[nodes], cnt[nodes]
        fitsin = c1 <= PATCH_MAX_PNTS
        todo = fitsin.copy()
        if degree2:
            sel = np.flatnonzero(todo & (c1 >= 6))
            ok, fits[0] = _patch_fit(src_xyz, nodes[sel], p1[sel], 6, gnomonic)
            fits[0] = (sel, fits[0])
            att[sel[ok]] = 0
            pat[sel[ok], :K1] = p1[sel[ok]]
            todo[sel[ok]] = False
            if is_mesh and ring2:
                sel = np.flatnonzero(todo)
                d = np.where(p1[sel] >= 0, p1[sel], 0)
                cand = np.where((p1[sel] >= 0)[:, :, None] & (nbr[d] >= 0), nbr[d], _PATCH_NONE).reshape(sel.size, K1 * K1)
                over = ((p1[sel] >= 0) & (cnt[d] > PATCH_MAX_PNTS)).any(axis=1)
                p2, c2 = _patch_pack(cand) if sel.size else (np.zeros((0, 1), np.int32), np.zeros(0, np.int64))
                p2 = np.asarray(p2, np.int64)
                try2 = ~over & (c2 >= 6) & (c2 <= PATCH_MAX_PNTS)
                sel, p2 = sel[try2], p2[try2]
                ok, f = _patch_fit(src_xyz, nodes[sel], p2, 6, gnomonic)
                fits[1] = (sel, f)
                att[sel[ok]] = 1
                pat[sel[ok], :p2.shape[1]] = p2[ok]
                todo[sel[ok]] = False
        sel = np.flatnonzero(todo & (c1 >= 3))
        ok, f = _patch_fit(src_xyz, nodes[sel], p1[sel], 3, gnomonic)
        fits[2] = (sel, f)
        att[sel[ok]] = 2
        pat[sel[ok], :K1] = p1[sel[ok]]
        # the shape values of every (row, slot) pair under its node's attempt
        patt = att[inv]
        ppat = pat[inv]
        L = np.zeros((prow.size, PATCH_MAX_PNTS))
        L[patt == 3, 0] = 1.0
        for a, M in ((0, 6), (1, 6), (2, 3)):
            if a not in fits:
                continue
            sel, f = fits[a]
            pairs = np.flatnonzero(patt == a)
            if pairs.size == 0:
                continue
            where = np.full(nodes.size, -1, np.int64)
            where[sel] = np.arange(sel.size)
            L[pairs] = _patch_shape(src_xyz, f, where[inv[pairs]], ppat[pairs], [dst_xyz[c][prow[pairs]] for c in range(3)], M, gnomonic)
        term = pb[:, None] * L
    # the ordered merge: distinct ids ascending per row, the values summed in (slot, patch position) order from 0.0
    live = ppat >= 0
    crow = np.broadcast_to(prow[:, None], ppat.shape)[live]
    cid, cterm = ppat[live], term[live]
    key = crow * np.int64(max(n_src, 1)) + cid
    order = np.argsort(key, kind="stable")
    key, cterm = key[order], cterm[order]
    first = np.ones(key.size, bool)
    first[1:] = key[1:] != key[:-1]
    grp = np.cumsum(first) - 1
    start = np.flatnonzero(first)
    rank = np.arange(key.size) - start[grp] if key.size else np.zeros(0, np.int64)
    val = np.zeros(start.size)
    for t in range(int(rank.max()) + 1 if key.size else 0):
        s_ = np.flatnonzero(rank == t)
        val[grp[s_]] = val[grp[s_]] + cterm[s_]
    col = (key[start] % max(n_src, 1)).astype(np.int32)
    rowlen = np.bincount(key[start] // max(n_src, 1), minlength=n_dst).astype(np.int64)
    rowptr = np.concatenate([[0], np.cumsum(rowlen)]).astype(np.int64)
    stats = [int((rowlen > 0).sum())] + [int((patt == a).sum()) for a in range(4)] + [int(rowlen.max()) if n_dst else 0]
    return rowptr, col, val, stats


def patch_rows(idx, w, src_xyz, dst_xyz, neighbours):
    """The numpy mirror of mpg_handle_patch, written elementwise in the order of mpassit_amd/csrc/patch.h so that it has the device's bits.
    idx, w: the weights() of a fixed bilinear handle, [n_dst][S] with -1 = no entry; src_xyz [3][n_src], dst_xyz [3][n_dst]: the library's
    stored unit vectors (Mesh.xyz / Grid.xyz); neighbours: patch_neighbours_mesh(voc, tri) or patch_neighbours_grid(snx, sny).
    Per source node the attempt ladder of include/mpassit_amd.h -- (A) degree 2 on the ring-1 patch, (B) degree 2 on the ring-2 patch (a
    mesh), (C) degree 1 on ring 1, (D) the node itself; per mapped row the distinct ids of its slots' patches ascending, the values
    acc = acc + b_s * L_(s,k) over (slot, patch position) from 0.0.
    -> (rowptr int64, col int32, val, stats): stats = [rows written, pairs served by A, B, C, D, longest row], mpg_handle_store_stats
    [1..6]."""
    return _patch_rows(idx, w, src_xyz, dst_xyz, neighbours)


REGRIDMETHOD_CONSERVE_2ND = 4
_C2_DET_TOL = 2.0 ** -26
_C2_HALF_TOL = 2.0 ** -10


def _c2_dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _c2_cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _c2_tri_area(a, b, c):
    """c2_tri_area of conserve2nd.h on [..., 3] unit vectors: sph_tri_area's num / den, half-angle steps down to |x| < 2^-10, the series."""
    num = _c2_dot(a, _c2_cross(b - a, c - a))
    den = ((1.0 + _c2_dot(a, b)) + _c2_dot(b, c)) + _c2_dot(c, a)
    ok = den > 0.0
    x = num / np.where(ok, den, 1.0)
    scale = np.full(x.shape, 2.0)
    for _ in range(64):
        big = ~(np.abs(x) < _C2_HALF_TOL)
        if not big.any():
            break
        x = np.where(big, x / (1.0 + np.sqrt(1.0 + x * x)), x)
        scale = np.where(big, scale * 2.0, scale)
    x2 = x * x
    return np.where(ok, scale * (x * (1.0 - x2 * (1.0 / 3.0 - x2 * (1.0 / 5.0 - x2 * (1.0 / 7.0))))), 0.0)


def _c2_fan(xyz, cnt):
    """The fan from slot 0 of the polygons (xyz [n][M][3], cnt [n]): the signed area and the moment [n][3], both from 0.0 in slot order."""
    n, M = xyz.shape[:2]
    area, m = np.zeros(n), np.zeros((n, 3))
    for t in range(1, M - 1):
        on = cnt > t + 1
        if not on.any():
            break
        a = np.where(on, _c2_tri_area(xyz[:, 0], xyz[:, t], xyz[:, t + 1]), 0.0)
        c = ((xyz[:, 0] + xyz[:, t]) + xyz[:, t + 1]) / 3.0
        area = np.where(on, area + a, area)
        m = np.where(on[:, None], m + a[:, None] * c, m)
    return area, m


def _c2_ccw(xyz, cnt, rev):
    out = xyz.copy()
    k = np.arange(xyz.shape[1])[None, :]
    src = np.where(k < cnt[:, None], cnt[:, None] - 1 - k, k)
    out[rev] = np.take_along_axis(xyz[rev], src[rev][:, :, None], axis=1)
    return out


def _c2_clip(subj, n, clip, clip_n):
    """Sutherland-Hodgman of conserve_clip.h over aligned pairs: subject polygons (subj [Np][Ms][3], n [Np]) by the sides of the clip
    polygons in order (both counter-clockwise) -> (polygon [Np][Ms + Mc][3], count)."""
    Np, Ms = subj.shape[:2]
    Mc = clip.shape[1]
    cap = Ms + Mc
    poly = np.zeros((Np, cap, 3))
    poly[:, :Ms] = subj
    n = n.astype(np.int64).copy()
    rows_all = np.arange(Np)
    for e in range(Mc):
        nxt = np.where(e + 1 == clip_n, 0, np.minimum(e + 1, Mc - 1))
        qa, qb = clip[:, e], clip[rows_all, nxt]
        side = qb - qa
        act = (e < clip_n) & (n >= 3) & ~(_c2_dot(side, side) < 1e-24)
        if not act.any():
            continue
        nrm = _c2_cross(qa, side)
        eps = 1e-15 * np.sqrt(_c2_dot(nrm, nrm))
        out = np.zeros_like(poly)
        m = np.zeros(Np, np.int64)
        for i in range(int(n[act].max())):
            r = rows_all[act & (i < n)]
            X1 = poly[r, i]
            X2 = poly[r, np.where(i + 1 == n[r], 0, i + 1)]
            d1, d2 = _c2_dot(nrm[r], X1), _c2_dot(nrm[r], X2)
            in1, in2 = d1 >= -eps[r], d2 >= -eps[r]
            k = r[in1]
            out[k, m[k]] = X1[in1]
            m[k] += 1
            x = in1 != in2
            X = X1[x] * d2[x][:, None] - X2[x] * d1[x][:, None]
            sgn = np.where((d2[x] - d1[x]) > 0.0, 1.0, -1.0)
            nn = np.sqrt(_c2_dot(X, X))
            good = nn > 0.0
            k = r[x][good]
            out[k, m[k]] = X[good] * (sgn[good] / nn[good])[:, None]
            m[k] += 1
        poly[act] = out[act]
        n[act] = m[act]
    return poly, n


def _c2_seq_sum(val, group, ngroups):
    """acc[g] = ((0.0 + v_0) + v_1) + ... over the items of group g in their given order; val [N] or [N][C]."""
    val = np.asarray(val, np.float64)
    acc = np.zeros((ngroups,) + val.shape[1:])
    if val.shape[0] == 0:
        return acc
    order = np.argsort(group, kind="stable")
    g = group[order]
    start = np.searchsorted(g, np.arange(ngroups))
    rank = np.arange(g.size) - start[g]
    for t in range(int(rank.max()) + 1):
        sel = order[rank == t]
        acc[group[sel]] = acc[group[sel]] + val[sel]
    return acc


def conserve2nd_polygons_mesh(voc, vert_xyz, cell_xyz=None):
    """The cells of a mesh for conserve2nd_rows: voc = verticesOnCell [nCells][maxEdges] (1-based, 0 = pad), vert_xyz / cell_xyz [3][n]:
    Mesh.xyz(MESHLOC_NODE) / Mesh.xyz(MESHLOC_ELEMENT) -> (xyz [nCells][maxEdges][3] valid entries first in listed order, cnt, centres)."""
    voc = np.asarray(voc, np.int64)
    v = np.asarray(vert_xyz, np.float64).T
    ok = (voc > 0) & (voc <= v.shape[0])
    cnt = ok.sum(axis=1)
    ids = np.take_along_axis(voc, np.argsort(~ok, axis=1, kind="stable"), axis=1)
    xyz = v[np.clip(ids, 1, max(v.shape[0], 1)) - 1]
    xyz[np.arange(voc.shape[1])[None, :] >= cnt[:, None]] = 0.0
    return xyz, cnt, (None if cell_xyz is None else np.asarray(cell_xyz, np.float64).T)


def conserve2nd_polygons_grid(corner_xyz, nx, ny, center_xyz=None):
    """The cells of a grid for conserve2nd_rows, id = j * nx + i: corner_xyz / center_xyz [3][n]: Grid.xyz(STAGGERLOC_CORNER) /
    Grid.xyz(STAGGERLOC_CENTER) -> corners (i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1) of every cell, 4 each, the centres."""
    c = np.asarray(corner_xyz, np.float64).T.reshape(ny + 1, nx + 1, 3)
    xyz = np.stack([c[:-1, :-1], c[:-1, 1:], c[1:, 1:], c[1:, :-1]], axis=2).reshape(nx * ny, 4, 3)
    return xyz, np.full(nx * ny, 4, np.int64), (None if center_xyz is None else np.asarray(center_xyz, np.float64).T)


def _conserve2nd_rows(rowptr, col, src_polys, dst_polys, neighbours, norm, src_mask=None, first_order=False):
    """conserve2nd_rows with the switch of the tests (first_order True: every stencil fails) -> (rowptr, col, val, info): info holds the
    pieces' areas Aq, area_d, the sources' A_i and the statistics [pairs, passing, failing, stencil entries, longest row]."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64).reshape(-1)
    sx, sn = np.asarray(src_polys[0], np.float64), np.asarray(src_polys[1], np.int64)
    dx, dn = np.asarray(dst_polys[0], np.float64), np.asarray(dst_polys[1], np.int64)
    nS, nD, nnz = sx.shape[0], rowptr.size - 1, col.size
    centre = src_polys[2] if len(src_polys) > 2 and src_polys[2] is not None else np.zeros((nS, 3))
    mask = np.zeros(nS, bool) if src_mask is None else np.asarray(src_mask).reshape(-1) != 0
    with np.errstate(all="ignore"):
        # cells: orientation, area(d), G_i
        fa_s, _ = _c2_fan(sx, sn)
        fa_d, _ = _c2_fan(dx, dn)
        none_s, none_d = (sn < 3) | (fa_s == 0.0), (dn < 3) | (fa_d == 0.0)
        sc, dc = _c2_ccw(sx, sn, fa_s < 0.0), _c2_ccw(dx, dn, fa_d < 0.0)
        area_d = np.where(none_d, 0.0, np.abs(fa_d))
        _, mom = _c2_fan(sc, sn)
        r = np.sqrt(_c2_dot(mom, mom))
        useG = (sn >= 3) & (r > 0.0)
        G = np.where(useG[:, None], mom / np.where(useG, r, 1.0)[:, None], centre)
        e1, e2 = _patch_frame([G[:, 0], G[:, 1], G[:, 2]])
        e1, e2 = np.stack(e1, axis=1), np.stack(e2, axis=1)
        # pieces
        row = np.repeat(np.arange(nD), np.diff(rowptr))
        Aq, mq = np.zeros(nnz), np.zeros((nnz, 3))
        live = np.flatnonzero(~none_s[col] & ~none_d[row])
        for a in range(0, live.size, 1 << 15):                              # bounded memory
            q = live[a:a + (1 << 15)]
            poly, n = _c2_clip(sc[col[q]], sn[col[q]], dc[row[q]], dn[row[q]])
            ar, m = _c2_fan(poly, n)
            keep = n >= 3
            Aq[q] = np.where(keep & (ar > 0.0), ar, 0.0)
            mq[q] = np.where(keep[:, None], m, 0.0)
        rsum = _c2_seq_sum(Aq, row, nD)
        by_src = np.argsort(col, kind="stable")                               # a source's pieces in ascending destination id
        Ai = _c2_seq_sum(Aq[by_src], col[by_src], nS)
        Mi = _c2_seq_sum(mq[by_src], col[by_src], nS)
        # stencils
        nbr, cnt = np.asarray(neighbours[0], np.int64), np.asarray(neighbours[1], np.int64)
        K = nbr.shape[1]
        ids = np.arange(nS)
        safe = np.clip(nbr, 0, max(nS - 1, 0))
        member = (nbr >= 0) & (nbr < nS) & (nbr != ids[:, None]) & ~mask[safe]
        usable = (cnt <= PATCH_MAX_PNTS) & ~mask & (not first_order)
        member &= usable[:, None]
        dxk, dyk = np.zeros((nS, K)), np.zeros((nS, K))
        m00, m01, m11, ns = np.zeros(nS), np.zeros(nS), np.zeros(nS), np.zeros(nS, np.int64)
        for k in range(K):
            d = G[safe[:, k]] - G
            dxk[:, k], dyk[:, k] = _c2_dot(d, e1), _c2_dot(d, e2)
            on = member[:, k]
            m00 = np.where(on, m00 + dxk[:, k] * dxk[:, k], m00)
            m01 = np.where(on, m01 + dxk[:, k] * dyk[:, k], m01)
            m11 = np.where(on, m11 + dyk[:, k] * dyk[:, k], m11)
            ns += on
        p = m00 * m11
        det = p - m01 * m01
        ok = usable & (ns >= 2) & (det > _C2_DET_TOL * p)
        bxk = (m11[:, None] * dxk - m01[:, None] * dyk) / det[:, None]
        byk = (m00[:, None] * dyk - m01[:, None] * dxk) / det[:, None]
        member &= ok[:, None]
        sbx_own, sby_own = np.zeros(nS), np.zeros(nS)
        for k in range(K):
            on = member[:, k]
            sbx_own = np.where(on, sbx_own + bxk[:, k], sbx_own)
            sby_own = np.where(on, sby_own + byk[:, k], sby_own)
        own_bx, own_by = np.where(ok, -sbx_own, 0.0), np.where(ok, -sby_own, 0.0)
        # the stencil CSR: members and the cell itself, ascending
        cand_id = np.concatenate([np.where(member, nbr, _PATCH_NONE), ids[:, None]], axis=1)
        cand_bx = np.concatenate([bxk, own_bx[:, None]], axis=1)
        cand_by = np.concatenate([byk, own_by[:, None]], axis=1)
        order = np.argsort(cand_id, axis=1, kind="stable")
        cand_id = np.take_along_axis(cand_id, order, axis=1)
        cand_bx, cand_by = np.take_along_axis(cand_bx, order, axis=1), np.take_along_axis(cand_by, order, axis=1)
        have = cand_id != _PATCH_NONE
        slen = have.sum(axis=1)
        sptr = np.concatenate([[0], np.cumsum(slen)]).astype(np.int64)
        scol, sbx, sby = cand_id[have], cand_bx[have], cand_by[have]
        # offsets and weights
        okq = (Aq > 0.0) & (Ai[col] > 0.0)
        dq = mq / np.where(okq, Aq, 1.0)[:, None] - Mi[col] / np.where(okq, Ai[col], 1.0)[:, None]
        ex, ey = np.where(okq, _c2_dot(dq, e1[col]), 0.0), np.where(okq, _c2_dot(dq, e2[col]), 0.0)
        div = area_d[row] if norm == NORM_DSTAREA else rsum[row]
        w = np.where(div > 0.0, Aq / np.where(div > 0.0, div, 1.0), 0.0)
        # the rows: every (entry, stencil position) pair in order
        plen = slen[col]
        pair_p = np.repeat(np.arange(nnz), plen)
        first = np.cumsum(plen) - plen
        pair_k = sptr[col][pair_p] + (np.arange(pair_p.size) - first[pair_p])
        key = (row[pair_p] << 32) | scol[pair_k]
        ukey, entry = np.unique(key, return_inverse=True)
        entry = entry.reshape(-1)
        g = (ex[pair_p] * sbx[pair_k]) + (ey[pair_p] * sby[pair_k])
        t = np.where(scol[pair_k] == col[pair_p], 1.0 + g, g)
        val = _c2_seq_sum(w[pair_p] * t, entry, ukey.size)
    out_rowptr = np.searchsorted(ukey >> 32, np.arange(nD + 1)).astype(np.int64)
    out_col = (ukey & 0xFFFFFFFF).astype(np.int32)
    longest = int(np.diff(out_rowptr).max()) if nD else 0
    info = {"Aq": Aq, "area_d": area_d, "Ai": Ai, "pass": ok, "sptr": sptr, "scol": scol,
            "stats": [int(nnz), int(ok.sum()), int(nS - ok.sum()), int(scol.size), longest]}
    return out_rowptr, out_col, val, info


def conserve2nd_rows(rowptr, col, src_polys, dst_polys, neighbours, norm, src_mask=None):
    """The numpy mirror of mpg_handle_conserve2nd, written elementwise in the order of mpassit_amd/csrc/conserve2nd.h and conserve_clip.h so
    that it has the device's bits.  rowptr, col: the csr() pattern of a first-order conservative handle; src_polys / dst_polys: the cells
    of the two sides from conserve2nd_polygons_mesh / _grid fed with the library's own unit vectors (Mesh.xyz(MESHLOC_NODE), Grid.xyz(
    STAGGERLOC_CORNER); the cell centres are the fallback of G_i); neighbours: patch_neighbours_mesh(voc, tri) of the source mesh or
    patch_neighbours_grid(nx, ny) of the source grid's CENTER stagger; norm: the Store's NORM_*; src_mask [n_src]: non-zero = masked.
    Per stored entry the re-clipped piece's area and moment, per source cell the centroid of its covered part and the least-squares
    stencil b over N1 minus itself minus the masked cells (failing: the cell alone, b = 0), per row the ascending union of its sources'
    stencils with acc = acc + w_q * t in stored order from 0.0 (include/mpassit_amd.h states every step).
    -> (rowptr int64, col int32, val)."""
    return _conserve2nd_rows(rowptr, col, src_polys, dst_polys, neighbours, norm, src_mask)[:3]


_COMPOSE_VECTOR_PASSES = 64   # terms of an entry of C summed by vectorised passes; what lies behind them is summed by a plain loop


def compose_csr(a_rowptr, a_col, a_val, b_rowptr, b_col, b_vals):
    """C = A . B of two CSR matrices, the bit-exact mirror of mpg_handle_compose and mpg_compose_weights_dev -> (rowptr int64, col int32,
    vals [K][nnz_C]) for b_vals [K][nnz_B] (a 1-D b_vals is one plane).  Pattern: row i holds the distinct columns reachable from A's row
    i through B's rows, ascending; structural (a value of 0.0 stays); rows that reach nothing are empty.  Values: c[i,e] from 0.0, over
    A's entries p of row i in stored order and within each over B's entries q of row a_col[p] in stored order with b_col[q] == e,
    acc = acc + (a_p * b_q), the product and the sum each rounded (numpy contracts nothing); duplicates are one term per occurrence.
    The (p, q) pairs are laid out in that order once; pass t adds the t-th term of every entry, so no index repeats within a pass and
    each entry sees its terms in order.  Entries with more than _COMPOSE_VECTOR_PASSES terms (long rows, heavy duplicates) finish in a
    plain loop over their remaining pairs, in the same order."""
    a_rowptr, b_rowptr = np.asarray(a_rowptr, dtype=np.int64), np.asarray(b_rowptr, dtype=np.int64)
    a_col, b_col = np.asarray(a_col, dtype=np.int64).reshape(-1), np.asarray(b_col, dtype=np.int64).reshape(-1)
    a_val = np.asarray(a_val, dtype=np.float64).reshape(-1)
    b_vals = np.asarray(b_vals, dtype=np.float64)
    b_vals = b_vals.reshape(1, -1) if b_vals.ndim <= 1 else b_vals
    K, n = b_vals.shape[0], a_rowptr.size - 1
    if a_col.size and (a_col.min() < 0 or a_col.max() >= b_rowptr.size - 1):
        raise ValueError("compose_csr: a column of A lies outside B's rows")
    # every (p, q) pair, p ascending and q ascending inside p: the summation order
    blen = np.diff(b_rowptr)[a_col]
    pair_p = np.repeat(np.arange(a_col.size), blen)
    first = np.cumsum(blen) - blen                                    # of each p among the pairs
    pair_q = b_rowptr[a_col][pair_p] + (np.arange(pair_p.size) - first[pair_p])
    pair_row = np.repeat(np.repeat(np.arange(n), np.diff(a_rowptr)), blen)
    key = (pair_row << 32) | b_col[pair_q]
    ukey, entry = np.unique(key, return_inverse=True)                 # sorted: rows together, columns ascending inside a row
    rowptr = np.searchsorted(ukey >> 32, np.arange(n + 1)).astype(np.int64)
    col = (ukey & 0xFFFFFFFF).astype(np.int32)
    vals = np.zeros((K, ukey.size))
    if pair_p.size == 0:
        return rowptr, col, vals
    entry = entry.reshape(-1)
    order = np.argsort(entry, kind="stable")                          # an entry's pairs, still in summation order
    start = np.searchsorted(entry[order], np.arange(ukey.size))
    rank = np.empty(pair_p.size, np.int64)
    rank[order] = np.arange(pair_p.size) - start[entry[order]]
    term = a_val[pair_p][None, :] * b_vals[:, pair_q]                 # [K][pairs], each product rounded
    for t in range(min(int(rank.max()) + 1, _COMPOSE_VECTOR_PASSES)):
        sel = np.nonzero(rank == t)[0]
        vals[:, entry[sel]] = vals[:, entry[sel]] + term[:, sel]
    for s in np.nonzero(rank >= _COMPOSE_VECTOR_PASSES)[0]:           # ascending pair index: ascending rank inside every entry
        for k in range(K):
            vals[k, entry[s]] = vals[k, entry[s]] + term[k, s]
    return rowptr, col, vals


@dataclass
class TargetGrid:
    """Host copy of what `define_target_grid_params` leaves in the ESMF Grid (all [nj][ni], degrees)."""
    nx: int  # mass points west-east  (= i_target = namelist nx - 1)
    ny: int  # mass points south-north (= j_target)
    proj: Proj
    is_regional: bool
    lat: np.ndarray = None
    lon: np.ndarray = None
    lat_u: np.ndarray = None
    lon_u: np.ndarray = None
    lat_v: np.ndarray = None
    lon_v: np.ndarray = None
    lat_c: np.ndarray = None
    lon_c: np.ndarray = None
    cosa: np.ndarray = None
    sina: np.ndarray = None
    extra: dict = field(default_factory=dict)


def define_target_grid_params(target_grid_type, nx, ny, dx=NAN, dy=NAN, ref_lat=NAN, ref_lon=NAN, ref_x=NAN, ref_y=NAN,
                              truelat1=NAN, truelat2=NAN, stand_lon=NAN, is_regional=True, arrays=True):
    """Namelist (&config, program_setup.F90:103-106) -> TargetGrid.  nx, ny are the namelist's
    STAGGERED counts: the mass grid is (nx-1) x (ny-1) (program_setup.F90:163-164).
    arrays=False stops after the namelist checks and the projection set-up: the coordinate arrays are then
    produced on the device by `regrid.Grid.from_proj(target)`."""
    i_target, j_target = nx - 1, ny - 1
    kind = target_grid_type.upper()
    known_x, known_y, known_lat, known_lon = ref_x, ref_y, ref_lat, ref_lon
    if kind == "LAMBERT":
        if truelat2 == NAN:
            if truelat1 == NAN:
                raise ValueError("No TRUELAT1 specified for Lambert conformal projection.")
            truelat2 = truelat1
    elif kind == "LAT-LON":
        if dx == NAN and dy == NAN:
            if is_regional:
                raise ValueError("For lat-lon projection, if dx/dy are not specified a global grid is assumed.")
            dlondeg, dlatdeg = 360.0 / i_target, 180.0 / j_target
            known_x = known_y = 1.0
            known_lon = stand_lon + dlondeg / 2.0
            known_lat = -90.0 + dlatdeg / 2.0
        else:
            if not is_regional:
                raise ValueError("For lat-lon projection, if dx/dy are specified a regional grid is assumed.")
            dlatdeg, dlondeg = dy, dx
            if known_lat == NAN or known_lon == NAN:
                raise ValueError("For lat-lon projection with dx/dy, ref_lat/ref_lon must be specified")
    elif kind in ("MERCATOR", "POLAR"):
        if truelat1 == NAN:
            raise ValueError("No TRUELAT1 specified for the %s projection." % kind.lower())
    else:
        raise ValueError('In namelist, invalid target_grid_type specified. Valid projections are "lambert", "mercator", "polar", and '
                         '"lat-lon".')
    if known_x == NAN and known_y == NAN:
        known_x, known_y = (i_target + 1) / 2.0, (j_target + 1) / 2.0
    elif known_x == NAN or known_y == NAN:
        raise ValueError("In namelist, neither or both of ref_x, ref_y must be specified.")
    if kind == "LAMBERT":
        proj = Proj.lambert(truelat1, truelat2, stand_lon, known_lat, known_lon, known_x, known_y, dx)
    elif kind == "POLAR":
        proj = Proj.polar(truelat1, stand_lon, known_lat, known_lon, known_x, known_y, dx)
    elif kind == "MERCATOR":
        proj = Proj.mercator(truelat1, known_lat, known_lon, known_x, known_y, dx)
    else:
        proj = Proj.latlon(known_lat, known_lon, known_x, known_y, dlatdeg, dlondeg)
    g = TargetGrid(i_target, j_target, proj, is_regional)
    if not arrays:      # coordinates are generated on the device (regrid.Grid.from_proj -> mpg_grid_create_proj)
        return g
    g.lat, g.lon = proj.lat_lon_fields(i_target, j_target, M)
    g.lat_v, g.lon_v = proj.lat_lon_fields(i_target, j_target + 1, V)
    g.lat_u, g.lon_u = proj.lat_lon_fields(i_target + 1, j_target, U)
    g.lat_c, g.lon_c = proj.lat_lon_fields(i_target + 1, j_target + 1, CORNER)
    if proj.code == PROJ_LC:
        g.cosa, g.sina = get_rotang(g.lat, g.lon)
    return g


def get_cell_corners(lat, lon, dx):
    """CORNER-stagger coordinates of a file-defined target grid, exactly as get_cell_corners computes them
    (model_grid.F90:1902-1972): every corner is the great-circle destination point at distance sqrt(dx^2/2) from a
    mass point, with the bearings AS WRITTEN there -- 135 degrees for the (i, j) block, 225 on the extra column
    (from column i_target), 45 on the extra row (from row j_target), 315 at the far corner -- and its own constants
    pi = 3.14159265359, R = 6370000.  lat, lon: [nj][ni] degrees -> ([nj+1][ni+1], [nj+1][ni+1])."""
    pi, R = 3.14159265359, 6370000.0
    nj, ni = lat.shape
    d = np.sqrt((dx ** 2.0) / 2.0)

    def dest(la, lo, bearing_deg):
        lat1, lon1 = la * (pi / 180.0), lo * (pi / 180.0)
        brng = bearing_deg * (pi / 180.0)
        lat2 = np.arcsin(np.sin(lat1) * np.cos(d / R) + np.cos(lat1) * np.sin(d / R) * np.cos(brng))
        lon2 = lon1 + np.arctan2(np.sin(brng) * np.sin(d / R) * np.cos(lat1), np.cos(d / R) - np.sin(lat1) * np.sin(lat2))
        return lat2 * 180.0 / pi, lon2 * 180.0 / pi
    latc, lonc = np.empty((nj + 1, ni + 1)), np.empty((nj + 1, ni + 1))
    latc[:nj, :ni], lonc[:nj, :ni] = dest(lat, lon, 135.0)
    latc[:nj, ni], lonc[:nj, ni] = dest(lat[:, ni - 1], lon[:, ni - 1], 225.0)
    latc[nj, :ni], lonc[nj, :ni] = dest(lat[nj - 1, :], lon[nj - 1, :], 45.0)
    latc[nj, ni], lonc[nj, ni] = dest(lat[nj - 1, ni - 1], lon[nj - 1, ni - 1], 315.0)
    return latc, lonc


def define_target_grid_file(path):
    """target_grid_type = 'file' (define_target_grid_file, model_grid.F90:1203-1888): the grid comes from a WRF
    geo_em / wrfinput style file -- dimensions west_east / south_north, global attributes DX, CEN_LAT, CEN_LON,
    TRUELAT1/2, MOAD_CEN_LAT, STAND_LON, POLE_LAT/LON, MAP_PROJ, variables XLONG|XLONG_M, XLAT|XLAT_M, XLONG_U, XLAT_U,
    XLONG_V, XLAT_V, MAPFAC_M/U/V, SINALPHA / COSALPHA (Lambert), HGT|HGT_M; corners from get_cell_corners.
    Classic-format files only (ncio).  -> TargetGrid with host arrays (use regrid.Grid.from_target)."""
    from . import ncio
    with ncio.Reader(path) as r:
        ni, nj = r.dims["west_east"], r.dims["south_north"]

        def var(*names):
            for n in names:
                if n in r.vars:
                    v = r.vars[n]
                    return r.get(n, rec=0, dtype=np.float64) if v["record"] else r.get(n, dtype=np.float64)
            raise KeyError("%s: none of %s found" % (path, "/".join(names)))

        def att(name, default=NAN):
            try:
                return float(r.att(name)[0])
            except ncio.NcioError:
                return default
        dx = att("DX")
        code = int(att("MAP_PROJ", PROJ_LC))
        proj = Proj(code, dx=dx, stdlon=att("STAND_LON"), truelat1=att("TRUELAT1"), truelat2=att("TRUELAT2"))
        g = TargetGrid(ni, nj, proj, True)
        g.lon, g.lat = var("XLONG", "XLONG_M"), var("XLAT", "XLAT_M")
        g.lon_u, g.lat_u = var("XLONG_U"), var("XLAT_U")
        g.lon_v, g.lat_v = var("XLONG_V"), var("XLAT_V")
        g.lat_c, g.lon_c = get_cell_corners(g.lat, g.lon, dx)
        # The projection as a CLAIM the library checks on the grid's own points (mpg_grid_attach_proj: the Stores may then search
        # through its inverse instead of the box pyramid): the file's MAP_PROJ / TRUELAT1/2 / STAND_LON / DX with the grid's own first
        # mass point as the known point.  WRF numbers its projections 1 Lambert, 2 polar stereographic, 3 Mercator, 6 lat-lon
        # (a rotated lat-lon grid fails the check and keeps the pyramid).
        proj.lat1, proj.lon1, proj.knowni, proj.knownj = float(g.lat[0, 0]), float(g.lon[0, 0]), 1.0, 1.0
        if code == 6:
            proj.code = PROJ_LATLON
            proj.latinc = float(g.lat[1, 0] - g.lat[0, 0]) if nj > 1 else 0.0
            dlon = float(g.lon[0, 1] - g.lon[0, 0]) if ni > 1 else 0.0
            proj.loninc = dlon + 360.0 if dlon < -180.0 else dlon
        for k, names in (("mapfac_m", ("MAPFAC_M",)), ("mapfac_u", ("MAPFAC_U",)), ("mapfac_v", ("MAPFAC_V",)), ("hgt", ("HGT", "HGT_M"))):
            try:
                g.extra[k] = var(*names)
            except KeyError:
                pass
        if code == PROJ_LC:
            g.sina, g.cosa = var("SINALPHA"), var("COSALPHA")
        g.extra.update(from_file=True, ref_lat=att("MOAD_CEN_LAT", att("CEN_LAT")), ref_lon=att("CEN_LON"), pole_lat=att("POLE_LAT", 90.0),
                       pole_lon=att("POLE_LON", 0.0))
        try:                                                              # model_grid.F90:1288-1295
            mpc = r.att("MAP_PROJ_CHAR")
            g.extra["map_proj_char"] = mpc.strip() if isinstance(mpc, str) else None
        except ncio.NcioError:
            g.extra["map_proj_char"] = None
    return g
