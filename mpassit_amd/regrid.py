"""Host-side mirror of the ESMF verbs MPASSIT's hot path uses, bound to the HIP C-ABI.

Names follow the reference's call sites so that tests read like the reference:
  Mesh            <- ESMF_MeshCreate                 (model_grid.F90:488-497)
  Grid            <- ESMF_GridCreate* + GridAddCoord (model_grid.F90:684-728,736-1038)
  regrid_store    <- ESMF_Field[Bundle]RegridStore   (interp.F90:123,207,...,437)
  RouteHandle.regrid      <- ESMF_Field[Bundle]Regrid (interp.F90:134,219,...,443)
  RouteHandle.release     <- ESMF_FieldBundleRegridRelease (interp.F90:450-463)
Host numpy arrays go through mpg_regrid (H2D + kernel + D2H); torch CUDA tensors go through
mpg_regrid_dev on torch's current stream (device-resident fast path used by bench.py).
"""
import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import (LAYOUT_CELL_FAST, LAYOUT_LEV_FAST, MESHLOC_ELEMENT, MESHLOC_NODE, MESHLOC_EDGE, REGRIDMETHOD_BILINEAR, REGRIDMETHOD_CONSERVE,
                   REGRIDMETHOD_NEAREST_STOD, STAGGERLOC_CENTER, STAGGERLOC_CORNER, STAGGERLOC_EDGE1, STAGGERLOC_EDGE2,
                   NORM_DSTAREA, NORM_FRACAREA, POLEMETHOD_NONE, POLEMETHOD_ALLAVG, EXTRAPMETHOD_NEAREST_STOD, EXTRAPMETHOD_NEAREST_IDAVG,
                   EXTRAP_MAX_PNTS, MASKRULE_AUTO, MASKRULE_ROW, MASKRULE_ENTRY, check)

__all__ = ["MESHLOC_ELEMENT", "MESHLOC_NODE", "Mesh", "Grid", "RouteHandle", "regrid_store", "regrid_store_grid", "regrid_store_begin", "regrid_store_grid_begin", "rotate_winds_cgrid", "wind_destagger", "regrid_autograd",
           "regrid_store_to_mesh", "regrid_to_mesh_autograd", "regrid_store_conserve_to_mesh", "regrid_csr_to_mesh_autograd", "NORM_DSTAREA",
           "NORM_FRACAREA", "regrid_store_mesh", "regrid_rows_autograd", "regrid_store_conserve_mesh", "regrid_csr_rows_autograd",
           "REGRIDMETHOD_BILINEAR", "REGRIDMETHOD_CONSERVE", "REGRIDMETHOD_NEAREST_STOD", "STAGGERLOC_CENTER",
           "STAGGERLOC_EDGE1", "STAGGERLOC_EDGE2", "STAGGERLOC_CORNER", "LAYOUT_CELL_FAST", "LAYOUT_LEV_FAST",
           "regrid_store_periodic_to_mesh", "POLEMETHOD_NONE", "POLEMETHOD_ALLAVG", "regrid_store_grid_to_grid", "regrid_store_conserve_grid_to_grid", "wind_to_mesh", "mesh_rotang", "wind_to_mesh_autograd",
           "MESHLOC_EDGE", "mesh_edge_rotang", "wind_to_edges", "wind_to_edges_autograd",
           "wind_csr_to_mesh", "wind_csr_to_edges", "wind_csr_to_mesh_autograd", "wind_csr_to_edges_autograd",
           "sphere_frames", "wind_vector_weights", "wind_vector", "wind_vector_autograd",
           "reconstruct_store", "reconstruct_weights", "wind_reconstruct", "wind_reconstruct_autograd", "compose", "compose_weights",
           "rotate_winds_cgrid_transpose", "wind_destagger_transpose", "wind_destagger_autograd",
           "regrid_masked_autograd", "extrapolate", "EXTRAPMETHOD_NEAREST_STOD", "EXTRAPMETHOD_NEAREST_IDAVG", "EXTRAP_MAX_PNTS",
           "mask_handle", "extrapolate_masked", "store_masks", "MASKRULE_AUTO", "MASKRULE_ROW", "MASKRULE_ENTRY",
           "patch", "regrid_store_patch", "REGRIDMETHOD_PATCH", "PATCH_MAX_PNTS",
           "conserve_2nd", "regrid_store_conserve_2nd", "REGRIDMETHOD_CONSERVE_2ND",
           "creep", "creep_nearest", "CREEP_ALL_LEVELS",
           "regrid_store_nearest_dtos", "REGRIDMETHOD_NEAREST_DTOS", "DTOS_SUM", "DTOS_MEAN"]


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _dtype_f32(dtype):
    return str(dtype) in ("torch.float32", "float32")


def _stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# Algorithmic-byte accounting of a sequence of device calls (bench.py's `job` leg): while ACCOUNT is a list, every
# device-side Regrid / rotation appends (what, bytes) with the bytes of SURVEY s8(d) -- U*L*e_src + P*L*e_dst per field plus
# the handle's indices and weights once per call (U = the sources the handle references).  Off (None) by default: looking
# up U synchronises.
ACCOUNT = None


def _account_regrid(rh, nlev, nfields, src_elem, dst_elem):
    if ACCOUNT is None:
        return
    if getattr(rh, "_acc_U", None) is None:
        try:
            rh._acc_U = int(rh.unique_sources().size)
        except L.MpgError:                      # handles with pole terms: every source of the grid
            rh._acc_U = int(rh.n_src)
    wbytes = (rh.nnz * 12 + (rh.n_dst + 1) * 4) if rh.nnz_per_row == 0 else rh.n_dst * (4 if rh.nnz_per_row == 1 else 12 * rh.nnz_per_row)
    ACCOUNT.append(("regrid nnz%d L%d x%d" % (rh.nnz_per_row, nlev, nfields), nfields * nlev * (rh._acc_U * src_elem + rh.n_dst * dst_elem) + wbytes))


def _level_stride(out, lead, ny, nx, who):
    """The destination level stride of a device `out` (elements): 0 for a contiguous one (dense), else the stride of a view whose
    level planes lie a uniform `ld` >= ny * nx apart (Handle.empty_pitched: strides (nlev * ld, ld, nx, 1)).  lead: the leading
    sizes, (nfields, nlev) or (nlev,).  Any other layout -- rows not contiguous, transposed, a field stride that is not nlev
    times the level stride -- raises ValueError."""
    if out.is_contiguous():
        return 0
    shape = tuple(lead) + (ny, nx)
    if tuple(out.shape) != shape:
        raise ValueError("%s: a strided out must have the shape %s, not %s" % (who, shape, tuple(out.shape)))
    st = out.stride()
    if (nx > 1 and st[-1] != 1) or (ny > 1 and st[-2] != nx):
        raise ValueError("%s: out's rows must be contiguous (strides %s)" % (who, st))
    ld, inner = None, 1
    for size, stride in reversed(list(zip(lead, st[:len(lead)]))):
        if size == 1:
            continue
        if ld is None:
            ld = stride // inner if stride % inner == 0 else -1
        if ld < 0 or stride != ld * inner:
            raise ValueError("%s: out's level planes must lie one uniform stride apart (strides %s)" % (who, st))
        inner *= size
    if ld is None:        # a single plane: nothing to pitch
        return 0
    if ld < ny * nx:
        raise ValueError("%s: out's level stride %d is below the plane size %d" % (who, ld, ny * nx))
    return ld


def _parse_missing(who, src, missing, src_mask, n_src):
    """(flags, missing_value, mask pointer or None) of mpg_mask_opts from regrid_masked's `missing` ("nan", a number, a tuple of both, or
    None) and `src_mask` (bool / uint8 CUDA tensor of n_src).  With a float32 `src` the number is rounded to float32 first, so that a
    file's sentinel compares equal.  One text for the masked Regrid and its adjoint: both must take the same sources for missing."""
    import torch
    flags, mv = 0, 0.0
    for item in (missing if isinstance(missing, (tuple, list)) else (missing,)):
        if item is None:
            continue
        if isinstance(item, str):
            if item.lower() != "nan":
                raise ValueError("%s: missing must be \"nan\", a number, a tuple of both, or None" % who)
            flags |= L.MISSING_NAN
        elif np.isnan(float(item)):
            flags |= L.MISSING_NAN
        else:
            if flags & L.MISSING_VALUE:
                raise ValueError("%s: one numeric missing value at most" % who)
            flags |= L.MISSING_VALUE
            mv = float(np.float32(item)) if src.dtype == torch.float32 else float(item)
    mask_ptr = None
    if src_mask is not None:
        if not (_is_torch(src_mask) and src_mask.is_cuda and src_mask.is_contiguous() and src_mask.dtype in (torch.bool, torch.uint8)):
            raise ValueError("%s: src_mask must be a contiguous bool/uint8 CUDA tensor" % who)
        if src_mask.numel() != n_src:
            raise ValueError("src_mask has %d elements, handle expects %d" % (src_mask.numel(), n_src))
        mask_ptr = src_mask.data_ptr()
    return flags, mv, mask_ptr


class Mesh:
    """MPAS mesh as the reference hands it to ESMF: elements = cells, nodes = vertices.
    lat/lon in radians (file convention), verticesOnCell [nCells][maxEdges] 1-based, 0-padded."""

    def __init__(self, latCell, lonCell, latVertex, lonVertex, verticesOnCell, window_grid=None):
        """window_grid: a Grid (one rank's row block) -- only the part of the mesh that grid can see is brought to the
        device (mpg_mesh_create_window); ids stay global, Stores onto that grid give the weights of the whole mesh."""
        latCell, lonCell, latVertex, lonVertex = map(_f64, (latCell, lonCell, latVertex, lonVertex))
        voc = np.ascontiguousarray(verticesOnCell, dtype=np.int32)
        if voc.ndim != 2 or voc.shape[0] != latCell.size:
            raise ValueError("verticesOnCell must be [nCells][maxEdges]")
        self.nCells, self.nVertices, self.maxEdges = int(latCell.size), int(latVertex.size), int(voc.shape[1])
        self.nEdges = 0
        self._h = C.c_void_p()
        args = (C.c_int64(self.nCells), C.c_int64(self.nVertices), C.c_int(self.maxEdges), _ptr(latCell), _ptr(lonCell), _ptr(latVertex),
                _ptr(lonVertex), _ptr(voc))
        if window_grid is None:
            check(L.load().mpg_mesh_create(*args, C.byref(self._h)))
        else:
            check(L.load().mpg_mesh_create_window(*args, window_grid._h, C.byref(self._h)))

    @classmethod
    def from_mpas(cls, m, window_grid=None):
        mesh = cls(m.latCell, m.lonCell, m.latVertex, m.lonVertex, m.verticesOnCell, window_grid=window_grid)
        if getattr(m, "latEdge", None) is not None and window_grid is None:     # (a windowed mesh takes no edges)
            mesh.set_edges(m.latEdge, m.lonEdge, getattr(m, "angleEdge", None))
        return mesh

    def set_edges(self, latEdge, lonEdge, angleEdge=None):
        """mpg_mesh_set_edges: the mesh's edge points (radians, as the MPAS file holds latEdge / lonEdge / angleEdge), the destination
        MESHLOC_EDGE of regrid_store_to_mesh.  Once per mesh; without angleEdge, mesh_edge_rotang is refused."""
        latEdge, lonEdge = _f64(latEdge), _f64(lonEdge)
        if latEdge.ndim != 1 or latEdge.shape != lonEdge.shape:
            raise ValueError("set_edges: latEdge and lonEdge must be 1-D arrays of one size")
        if angleEdge is not None:
            angleEdge = _f64(angleEdge)
            if angleEdge.shape != latEdge.shape:
                raise ValueError("set_edges: angleEdge must have latEdge's size")
        check(L.mesh_set_edges(self._h, int(latEdge.size), _ptr(latEdge), _ptr(lonEdge), _ptr(angleEdge)))
        n = C.c_int64()
        check(L.mesh_edge_count(self._h, C.byref(n)))
        self.nEdges = int(n.value)

    def window_info(self):
        """(cell_first, cell_count, vertex_first, vertex_count, margin): the resident part of the geometry (the whole mesh
        unless it was made with window_grid) and the chord distance from the grid within which every cell is present."""
        a, b, c, d, mg = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
        check(L.load().mpg_mesh_window_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(mg)))
        return a.value, b.value, c.value, d.value, mg.value

    def set_source_window(self, first, count, meshloc=MESHLOC_ELEMENT):
        """Every handle of this mesh and location (existing and future) indexes its sources relative to `first`; Regrid
        then reads slabs of `count` ids (mpg_mesh_set_source_window).  Route handle objects made earlier: call
        RouteHandle._refresh() (n_src changes)."""
        check(L.load().mpg_mesh_set_source_window(self._h, C.c_int(meshloc), C.c_int64(first), C.c_int64(count)))

    def triangles(self):
        tri = np.empty((self.nVertices, 3), np.int32)
        check(L.load().mpg_mesh_get_triangles(self._h, _ptr(tri)))
        return tri

    def xyz(self, meshloc=MESHLOC_ELEMENT):
        """mpg_mesh_get_xyz: the stored unit vectors of the cells, vertices or edges, [3][n] float64 -- the bits the searches use."""
        n = {MESHLOC_ELEMENT: self.nCells, MESHLOC_NODE: self.nVertices, MESHLOC_EDGE: self.nEdges}[meshloc]
        xyz = np.empty((3, n))
        check(L.mesh_get_xyz(self._h, int(meshloc), _ptr(xyz)))
        return xyz

    def destroy(self):
        if self._h:
            check(L.load().mpg_mesh_destroy(self._h))
            self._h = C.c_void_p()


class _Proj(C.Structure):
    """struct mpg_proj (include/mpassit_amd.h)."""
    _fields_ = [("code", C.c_int), ("known_lat", C.c_double), ("known_lon", C.c_double), ("known_x", C.c_double),
                ("known_y", C.c_double), ("dx_m", C.c_double), ("stand_lon", C.c_double), ("truelat1", C.c_double),
                ("truelat2", C.c_double), ("dlat_deg", C.c_double), ("dlon_deg", C.c_double)]


class Grid:
    """Structured target grid with its four staggers (degrees, arrays [nj][ni], i fastest)."""

    def __init__(self, lon, lat, lon_corner=None, lat_corner=None, lon_u=None, lat_u=None, lon_v=None, lat_v=None,
                 periodic=False):
        lon, lat = _f64(lon), _f64(lat)
        self.ny, self.nx = lat.shape
        arrs = [None if a is None else _f64(a) for a in (lon_corner, lat_corner, lon_u, lat_u, lon_v, lat_v)]
        shapes = [(self.ny + 1, self.nx + 1)] * 2 + [(self.ny, self.nx + 1)] * 2 + [(self.ny + 1, self.nx)] * 2
        for a, s in zip(arrs, shapes):
            if a is not None and a.shape != s:
                raise ValueError("stagger coordinate array has shape %s, expected %s" % (a.shape, s))
        self._h = C.c_void_p()
        check(L.load().mpg_grid_create(C.c_int(self.nx), C.c_int(self.ny), C.c_int(int(periodic)), _ptr(lon), _ptr(lat),
                                       *[_ptr(a) for a in arrs], C.byref(self._h)))

    @classmethod
    def from_target(cls, g, rows=None, attach_proj=True):
        """From target_grid.TargetGrid; rows=(j0, j1) keeps only mass rows [j0, j1) (multi-GPU row shard,
        mirrors the reference's regDecomp=(/1,npets/) split along j, model_grid.F90:693).  A global grid
        (is_regional=.false.) is periodic in i with monopole caps (model_grid.F90:685-694); a row block keeps only
        the caps it touches."""
        flags = 0 if g.is_regional else L.GRID_PERIODIC_I
        if rows is None:
            self = cls(g.lon, g.lat, g.lon_c, g.lat_c, g.lon_u, g.lat_u, g.lon_v, g.lat_v, periodic=flags)
            j0 = 0
        else:
            j0, j1 = rows
            if flags:
                flags |= (L.GRID_NO_SOUTH_POLE if j0 > 0 else 0) | (L.GRID_NO_NORTH_POLE if j1 < g.ny else 0)
            self = cls(g.lon[j0:j1], g.lat[j0:j1], g.lon_c[j0:j1 + 1], g.lat_c[j0:j1 + 1], g.lon_u[j0:j1], g.lat_u[j0:j1],
                       g.lon_v[j0:j1 + 1], g.lat_v[j0:j1 + 1], periodic=flags)
        if attach_proj and getattr(g, "proj", None) is not None:
            try:                               # the arrays came from this projection: the Stores may search through its inverse.
                self.attach_proj(g.proj, j0)   # The library checks the claim on the grid's own points; a projection that does not
            except L.MpgError:                 # reproduce them (a grid read from a file, whose Proj is incomplete) is refused and
                pass                           # the grid keeps the pyramid search
        return self

    def attach_proj(self, p, row0=0):
        """mpg_grid_attach_proj: the coordinate arrays of this grid are rows row0 .. of projection `p` (target_grid.Proj)."""
        c = _Proj(code=p.code, known_lat=p.lat1, known_lon=p.lon1, known_x=p.knowni, known_y=p.knownj, dx_m=p.dx,
                  stand_lon=p.stdlon, truelat1=p.truelat1, truelat2=p.truelat2, dlat_deg=p.latinc, dlon_deg=p.loninc)
        check(L.load().mpg_grid_attach_proj(self._h, C.byref(c), C.c_int(int(row0))))

    @classmethod
    def from_proj(cls, g, fill_target=True):
        """Device-side target grid (mpg_grid_create_proj): all four staggers, map factors and cos/sin(alpha) are
        computed on the GPU from the projection of target_grid.TargetGrid `g` (built with arrays=False or not).
        fill_target: copy cos/sin(alpha) back into `g` (interp's wind rotation reads them from there)."""
        p = g.proj
        c = _Proj(code=p.code, known_lat=p.lat1, known_lon=p.lon1, known_x=p.knowni, known_y=p.knownj, dx_m=p.dx,
                  stand_lon=p.stdlon, truelat1=p.truelat1, truelat2=p.truelat2, dlat_deg=p.latinc, dlon_deg=p.loninc)
        self = cls.__new__(cls)
        self.nx, self.ny = g.nx, g.ny
        self._h = C.c_void_p()
        check(L.load().mpg_grid_create_proj(C.byref(c), C.c_int(g.nx), C.c_int(g.ny),
                                            C.c_int(0 if g.is_regional else L.GRID_PERIODIC_I), C.byref(self._h)))
        self.built_from_proj = True
        if fill_target and p.code == 1:
            g.cosa, g.sina = self.rotang()
        return self

    def coords(self, staggerloc):
        """(lon, lat) in degrees of a projection-built grid, [nj][ni] of that stagger (XLONG/XLAT[_U,_V] of the file)."""
        lon, lat = np.empty(self.stagger_shape(staggerloc)), np.empty(self.stagger_shape(staggerloc))
        check(L.load().mpg_grid_get_coords(self._h, C.c_int(staggerloc), _ptr(lon), _ptr(lat)))
        return lon, lat

    def rotang_dev(self):
        """(cosalpha, sinalpha) as they sit in device memory, owned by the grid (mpg_grid_rotang_dev): DevArray views for rotate_winds_cgrid /
        wind_destagger -- no download and upload of 2 x ny x nx doubles (configuration 4: 30 MB through pageable memory, 1.5 ms of a cold job)."""
        c, s = C.c_void_p(), C.c_void_p()
        check(L.load().mpg_grid_rotang_dev(self._h, C.byref(c), C.byref(s)))
        return DevArray(c.value, self.ny * self.nx), DevArray(s.value, self.ny * self.nx)

    def rotang(self):
        """(cosalpha, sinalpha) [ny][nx] (get_rotang, model_grid.F90:2450-2507); Lambert grids only."""
        cosa, sina = np.empty((self.ny, self.nx)), np.empty((self.ny, self.nx))
        check(L.load().mpg_grid_get_rotang(self._h, _ptr(cosa), _ptr(sina)))
        return cosa, sina

    def mapfac(self, staggerloc):
        """MAPFAC_M / _U / _V (get_map_factor, model_grid.F90:2229-2365)."""
        mf = np.empty(self.stagger_shape(staggerloc))
        check(L.load().mpg_grid_get_mapfac(self._h, C.c_int(staggerloc), _ptr(mf)))
        return mf

    def xyz(self, staggerloc=STAGGERLOC_CENTER):
        """mpg_grid_get_xyz: the stored unit vectors of a stagger's points, [3][snx * sny] float64 (point j * snx + i) -- the bits the
        searches use."""
        ny, nx = self.stagger_shape(staggerloc)
        xyz = np.empty((3, ny * nx))
        check(L.grid_get_xyz(self._h, int(staggerloc), _ptr(xyz)))
        return xyz

    def stagger_shape(self, staggerloc):
        return {STAGGERLOC_CENTER: (self.ny, self.nx), STAGGERLOC_EDGE1: (self.ny, self.nx + 1),
                STAGGERLOC_EDGE2: (self.ny + 1, self.nx), STAGGERLOC_CORNER: (self.ny + 1, self.nx + 1)}[staggerloc]

    def destroy(self):
        if self._h:
            check(L.load().mpg_grid_destroy(self._h))
            self._h = C.c_void_p()


class DevArray:
    """A device array the LIBRARY owns, as far as the wrappers need one (address + element count); valid while its owner lives."""

    def __init__(self, ptr, n):
        self._ptr, self._n = int(ptr), int(n)

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return self._n


class RouteHandle:
    def __init__(self, h):
        self._h = h
        n_src, n_dst, nnz = C.c_int64(), C.c_int64(), C.c_int64()
        nx, ny, npr = C.c_int(), C.c_int(), C.c_int()
        check(L.load().mpg_handle_info(h, C.byref(n_src), C.byref(n_dst), C.byref(nx), C.byref(ny), C.byref(npr), C.byref(nnz)))
        self.n_src, self.n_dst, self.nx_dst, self.ny_dst = n_src.value, n_dst.value, nx.value, ny.value
        self.nnz_per_row, self.nnz = npr.value, nnz.value

    @property
    def store_ms(self):
        ms = C.c_float()
        check(L.load().mpg_handle_store_ms(self._h, C.byref(ms)))
        return ms.value

    @property
    def store_path(self):
        """0 hierarchical candidate search, 1 through the grid's index space, 2 index space + BVH for the rest (nearest)."""
        v = C.c_int()
        check(L.load().mpg_handle_store_path(self._h, C.byref(v)))
        return v.value

    @property
    def store_stats(self):
        """mpg_handle_store_stats: which data-dependent branches the Store took (layout by method: include/mpassit_amd.h)."""
        v = (C.c_int64 * 8)()
        check(L.load().mpg_handle_store_stats(self._h, v, C.c_int(8)))
        return [int(x) for x in v]

    def _refresh(self):
        self.__init__(self._h)

    # -- pitched destinations ---------------------------------------------------------------------------
    def level_stride(self, dtype):
        """mpg_dst_level_stride: the smallest level stride (elements) >= ny_dst * nx_dst at which every level plane of this
        handle's results in `dtype` (torch / numpy float32 or float64) starts on a 128-byte line."""
        ld = C.c_int64()
        check(L.load().mpg_dst_level_stride(C.c_int64(self.n_dst), C.c_int(1 if _dtype_f32(dtype) else 0), C.byref(ld)))
        return ld.value

    def empty_pitched(self, nlev, nfields=1, dtype=None, device=None):
        """An uninitialised device result (nfields, nlev, ny_dst, nx_dst) whose level planes lie level_stride(dtype) elements apart:
        strides (nlev * ld, ld, nx_dst, 1).  Every device regrid / wind call takes it as `out`; the pad of each plane is never written."""
        import torch
        dtype = dtype or torch.float64
        ld = self.level_stride(dtype)
        buf = torch.empty(nfields * nlev * ld, dtype=dtype, device=device or "cuda")
        return buf.as_strided((nfields, nlev, self.ny_dst, self.nx_dst), (nlev * ld, ld, self.nx_dst, 1))

    # -- ESMF_FieldRegrid / ESMF_FieldBundleRegrid ---------------------------------------------------
    def regrid(self, src, nlev=1, nfields=1, layout=LAYOUT_CELL_FAST, out=None, src_be=False):
        """src: nfields slabs of nlev*n_src float64 (numpy on host or torch on the GPU).
        Returns dst [nfields][nlev][ny_dst][nx_dst] (squeezing nfields == 1 and nlev == 1 is left to the caller).
        src_be: the CUDA tensor holds the big-endian bytes of a NetCDF classic variable (io_nc device flow)."""
        shape = (nfields, nlev, self.ny_dst, self.nx_dst)
        need = nfields * nlev * self.n_src
        if _is_torch(src):
            import torch
            if src.is_cuda and (src.dtype == torch.float32 or src_be) and src.is_contiguous():
                # a field still in the file's NF90_FLOAT type (and byte order): widened inside the kernel's loads (same
                # result as widening first, nf90_get_var -> r8 in input_data.F90), float64 out
                return self.regrid_typed(src, nlev=nlev, nfields=nfields, layout=layout, out_dtype=torch.float64, out=out, src_be=src_be)
            if not src.is_cuda or src.dtype != torch.float64 or not src.is_contiguous():
                raise ValueError("device regrid needs a contiguous float32/float64 CUDA tensor")
            if src.numel() != need:
                raise ValueError("source has %d elements, handle expects %d" % (src.numel(), need))
            if out is None:
                out = torch.empty(shape, dtype=torch.float64, device=src.device)
            ld = _level_stride(out, (nfields, nlev), self.ny_dst, self.nx_dst, "regrid")
            _account_regrid(self, nlev, nfields, 8, 8)
            check(L.load().mpg_regrid_pitched_dev(self._h, C.c_void_p(src.data_ptr()), C.c_int(layout), C.c_int(nlev), C.c_int(nfields),
                                                  C.c_void_p(out.data_ptr()), C.c_int64(ld), _stream_ptr()))
            return out
        if isinstance(src, np.ndarray) and src.dtype == np.float32:
            return self.regrid_typed_host(src, nlev=nlev, nfields=nfields, layout=layout, out_dtype=np.float64, out=out)
        src = _f64(src)
        if src.size != need:
            raise ValueError("source has %d elements, handle expects %d" % (src.size, need))
        if out is None:
            out = np.empty(shape)
        check(L.load().mpg_regrid(self._h, _ptr(src), C.c_int(layout), C.c_int(nlev), C.c_int(nfields), _ptr(out)))
        return out

    def regrid_typed(self, src, nlev=1, nfields=1, layout=LAYOUT_CELL_FAST, out_dtype=None, scale=1.0, offset=0.0, out=None,
                     src_be=False, dst_be=False):
        """Fused ingest/egress Regrid on device tensors: float32 or float64 source (as in the MPAS file), float32 or
        float64 destination (as in the output file), float64 arithmetic, dst = cast(regrid(src)*scale + offset).
        src_be / dst_be: that side holds big-endian values (the bytes of a NetCDF classic variable; MPG_TYPE_BE)."""
        import torch
        if not (src.is_cuda and src.is_contiguous() and src.dtype in (torch.float32, torch.float64)):
            raise ValueError("regrid_typed needs a contiguous float32/float64 CUDA tensor")
        if src.numel() != nfields * nlev * self.n_src:
            raise ValueError("source has %d elements, handle expects %d" % (src.numel(), nfields * nlev * self.n_src))
        out_dtype = out_dtype or src.dtype
        if out is None:
            out = torch.empty((nfields, nlev, self.ny_dst, self.nx_dst), dtype=out_dtype, device=src.device)
        ld = _level_stride(out, (nfields, nlev), self.ny_dst, self.nx_dst, "regrid_typed")
        _account_regrid(self, nlev, nfields, src.element_size(), out.element_size())
        check(L.load().mpg_regrid_typed_pitched_dev(self._h, C.c_void_p(src.data_ptr()), C.c_int(int(src.dtype == torch.float32) | (2 if src_be else 0)),
                                                    C.c_int(layout), C.c_int(nlev), C.c_int(nfields), C.c_void_p(out.data_ptr()),
                                                    C.c_int(int(out.dtype == torch.float32) | (2 if dst_be else 0)), C.c_double(scale), C.c_double(offset),
                                                    C.c_int64(ld), _stream_ptr()))
        return out

    def regrid_bundle(self, srcs, nlev=1, layout=LAYOUT_CELL_FAST, out_dtype=None, scale=1.0, offsets=None, outs=None, src_be=False, dst_be=False):
        """ESMF_FieldBundleRegrid over SEPARATE field arrays (interp.F90:240-254; mpg_regrid_bundle_typed_dev): srcs = device
        tensors of nlev * n_src elements each, one dtype; one launch for all of them, per-field epilogue offsets.  Returns the
        list of results [nlev][ny][nx] (outs: tensors to write into)."""
        import torch
        nf = len(srcs)
        if nf == 0:
            return []
        dt = srcs[0].dtype
        for t in srcs:
            if not (t.is_cuda and t.is_contiguous() and t.dtype == dt and dt in (torch.float32, torch.float64)):
                raise ValueError("regrid_bundle needs contiguous CUDA tensors of one float32 / float64 dtype")
            if t.numel() != nlev * self.n_src:
                raise ValueError("a source has %d elements, handle expects %d" % (t.numel(), nlev * self.n_src))
        out_dtype = out_dtype or dt
        if outs is None:
            outs = [torch.empty((nlev, self.ny_dst, self.nx_dst), dtype=out_dtype, device=srcs[0].device) for _ in range(nf)]
        lds = set()
        for t in outs:
            if not (t.is_cuda and t.dtype == outs[0].dtype and t.numel() == nlev * self.n_dst):
                raise ValueError("regrid_bundle: bad destination tensor")
            if t.is_contiguous():
                lds.add(0)
            else:   # a pitched result, (nlev, ny, nx) or empty_pitched's (1, nlev, ny, nx)
                lead = tuple(t.shape[:-2]) if t.dim() == 4 else (nlev,)
                lds.add(_level_stride(t, lead, self.ny_dst, self.nx_dst, "regrid_bundle"))
        if len(lds) > 1:
            raise ValueError("regrid_bundle: the destinations must share one level stride (or all be dense)")
        ld = lds.pop()
        _account_regrid(self, nlev, nf, srcs[0].element_size(), outs[0].element_size())
        sp = (C.c_void_p * nf)(*[t.data_ptr() for t in srcs])
        dp = (C.c_void_p * nf)(*[t.data_ptr() for t in outs])
        op = None if offsets is None else (C.c_double * nf)(*[float(o) for o in offsets])
        check(L.load().mpg_regrid_bundle_typed_pitched_dev(self._h, C.c_int(nf), sp, C.c_int(int(dt == torch.float32) | (2 if src_be else 0)),
                                                           C.c_int(layout), C.c_int(nlev), dp,
                                                           C.c_int(int(outs[0].dtype == torch.float32) | (2 if dst_be else 0)),
                                                           C.c_double(scale), op, C.c_int64(ld), _stream_ptr()))
        return outs

    def regrid_typed_host(self, src, nlev=1, nfields=1, layout=LAYOUT_CELL_FAST, out_dtype=None, scale=1.0, offset=0.0, out=None):
        """The same on numpy arrays (mpg_regrid_typed): float32 / float64 host buffers cross PCIe as they are, chunks of
        levels are uploaded, regridded and downloaded concurrently.  Returns [nfields][nlev][ny][nx] of out_dtype."""
        src = np.ascontiguousarray(src)
        if src.dtype not in (np.float32, np.float64):
            src = src.astype(np.float64)
        if src.size != nfields * nlev * self.n_src:
            raise ValueError("source has %d elements, handle expects %d" % (src.size, nfields * nlev * self.n_src))
        out_dtype = np.dtype(out_dtype or src.dtype)
        if out is None:
            out = np.empty((nfields, nlev, self.ny_dst, self.nx_dst), out_dtype)
        check(L.load().mpg_regrid_typed(self._h, src.ctypes.data_as(C.c_void_p), C.c_int(int(src.dtype == np.float32)), C.c_int(layout),
                                        C.c_int(nlev), C.c_int(nfields), out.ctypes.data_as(C.c_void_p),
                                        C.c_int(int(out.dtype == np.float32)), C.c_double(scale), C.c_double(offset)))
        return out

    def regrid_bundle_host(self, srcs, nlev=1, layout=LAYOUT_CELL_FAST, out_dtype=None, scale=1.0, offsets=None, outs=None):
        """mpg_regrid_bundle_typed: the fields of a bundle as separate numpy arrays (float32 or float64, one dtype), all through
        ONE upload / Regrid / download pipeline.  Returns the list of results [nlev][ny][nx] of out_dtype."""
        nf = len(srcs)
        if nf == 0:
            return []
        srcs = [np.ascontiguousarray(a) for a in srcs]
        dt = srcs[0].dtype
        if dt not in (np.float32, np.float64) or any(a.dtype != dt for a in srcs):
            raise ValueError("regrid_bundle_host needs float32 or float64 arrays of one dtype")
        for a in srcs:
            if a.size != nlev * self.n_src:
                raise ValueError("a source has %d elements, handle expects %d" % (a.size, nlev * self.n_src))
        out_dtype = np.dtype(out_dtype or dt)
        if outs is None:
            outs = [np.empty((nlev, self.ny_dst, self.nx_dst), out_dtype) for _ in range(nf)]
        sp = (C.c_void_p * nf)(*[a.ctypes.data for a in srcs])
        dp = (C.c_void_p * nf)(*[o.ctypes.data for o in outs])
        op = None if offsets is None else (C.c_double * nf)(*[float(o) for o in offsets])
        check(L.load().mpg_regrid_bundle_typed(self._h, C.c_int(nf), sp, C.c_int(int(dt == np.float32)), C.c_int(layout), C.c_int(nlev), dp,
                                               C.c_int(int(out_dtype == np.float32)), C.c_double(scale), op))
        return outs

    # -- transposeRoutehandle: the adjoint A^T (not an inverse) ------------------------------------------
    def regrid_transpose(self, src, nlev=1, nfields=1, layout=LAYOUT_CELL_FAST, out_dtype=None, out=None):
        """mpg_regrid_transpose_dev: mesh_out = A^T grid_in with the operator regrid() applies (ESMF's transposeRoutehandle).  The
        ADJOINT of the Regrid, not an inverse (A^T A != I): it takes gradients, increments and residuals back to the mesh.
        src: grid values [nfields][nlev][ny_dst][nx_dst], float32 / float64, a CUDA tensor (contiguous, or a plane-pitched view as
        empty_pitched makes) or a numpy array (uploaded, and the result comes back as numpy).  Returns nfields slabs of nlev * n_src
        values of out_dtype (default: src's): (nfields, nlev, n_src) for LAYOUT_CELL_FAST, (nfields, n_src, nlev) for LAYOUT_LEV_FAST.
        Sources no entry references are exactly 0."""
        import torch
        host = isinstance(src, np.ndarray)
        if host:
            src = torch.from_numpy(np.ascontiguousarray(src)).cuda()
        if not (_is_torch(src) and src.is_cuda and src.dtype in (torch.float32, torch.float64)):
            raise ValueError("regrid_transpose needs a float32/float64 CUDA tensor or numpy array")
        if src.is_contiguous():
            if src.numel() != nfields * nlev * self.n_dst:
                raise ValueError("source has %d elements, handle expects %d" % (src.numel(), nfields * nlev * self.n_dst))
            ld = 0
        else:
            lead = (nfields, nlev) if src.dim() == 4 else (nlev,)
            if src.dim() not in (3, 4) or (src.dim() == 3 and nfields != 1):
                raise ValueError("regrid_transpose: a strided source must be (nfields, nlev, ny, nx) or (nlev, ny, nx) with plane-pitched levels")
            ld = _level_stride(src, lead, self.ny_dst, self.nx_dst, "regrid_transpose")
        out_dtype = out_dtype or src.dtype
        if isinstance(out_dtype, np.dtype) or out_dtype in (np.float32, np.float64):
            out_dtype = torch.float32 if np.dtype(out_dtype) == np.float32 else torch.float64
        shape = (nfields, nlev, self.n_src) if layout == LAYOUT_CELL_FAST else (nfields, self.n_src, nlev)
        if out is None:
            out = torch.empty(shape, dtype=out_dtype, device=src.device)
        elif not (out.is_cuda and out.is_contiguous() and out.dtype in (torch.float32, torch.float64) and out.numel() == nfields * nlev * self.n_src):
            raise ValueError("regrid_transpose: out must be a contiguous float32/float64 CUDA tensor of %d elements" % (nfields * nlev * self.n_src))
        check(L.load().mpg_regrid_transpose_dev(self._h, C.c_void_p(src.data_ptr()), C.c_int(int(src.dtype == torch.float32)), C.c_int64(ld),
                                                C.c_int(nlev), C.c_int(nfields), C.c_void_p(out.data_ptr()),
                                                C.c_int(int(out.dtype == torch.float32)), C.c_int(layout), _stream_ptr()))
        return out.cpu().numpy() if host else out

    # -- Grid -> Mesh: the mesh's own memory orders ---------------------------------------------------
    def regrid_to_mesh(self, src, nlev=1, nfields=1, layout=LAYOUT_CELL_FAST, out_dtype=None, scale=1.0, offset=0.0, out=None):
        """mpg_regrid_to_mesh_dev: Regrid of a fixed-nnz handle (regrid_store_to_mesh's, but any 4-, 3- or 1-slot handle) onto its
        n_dst points in either memory order of a mesh field.  `layout` is the DESTINATION layout: LAYOUT_CELL_FAST returns
        (nfields, nlev, n_dst) with the bytes of regrid_typed, LAYOUT_LEV_FAST (nfields, n_dst, nlev) -- MPAS file order -- with the
        same bits transposed.  src: grid values [nfields][nlev][plane of n_src], float32 / float64, a contiguous CUDA tensor or a
        plane-pitched view (nfields, nlev, ny, nx) / (nlev, ny, nx) as empty_pitched of the handle that produced it makes.
        dst = cast(regrid(src) * scale + offset), float64 arithmetic."""
        return self._to_mesh(L.regrid_to_mesh_dev, "regrid_to_mesh", src, nlev, nfields, layout, out_dtype, scale, offset, out)

    def regrid_csr_to_mesh(self, src, nlev=1, nfields=1, layout=LAYOUT_CELL_FAST, out_dtype=None, scale=1.0, offset=0.0, out=None):
        """mpg_regrid_csr_to_mesh_dev: regrid_to_mesh for CSR handles -- regrid_store_conserve_to_mesh's, a Mesh -> Grid conservative
        one, a from_weights one.  Same source rules (contiguous, or a plane-pitched view), same layouts and epilogue; LAYOUT_CELL_FAST
        has the bytes of regrid_typed on the same handle, LAYOUT_LEV_FAST the same bits transposed."""
        return self._to_mesh(L.regrid_csr_to_mesh_dev, "regrid_csr_to_mesh", src, nlev, nfields, layout, out_dtype, scale, offset, out)

    def _to_mesh(self, fn, who, src, nlev, nfields, layout, out_dtype, scale, offset, out):
        import torch
        if not (_is_torch(src) and src.is_cuda and src.dtype in (torch.float32, torch.float64)):
            raise ValueError(who + " needs a float32/float64 CUDA tensor")
        if src.is_contiguous():
            if src.numel() != nfields * nlev * self.n_src:
                raise ValueError("source has %d elements, handle expects %d" % (src.numel(), nfields * nlev * self.n_src))
            ld = 0
        else:
            if src.dim() not in (3, 4) or (src.dim() == 3 and nfields != 1):
                raise ValueError(who + ": a strided source must be (nfields, nlev, ny, nx) or (nlev, ny, nx) with plane-pitched levels")
            ny, nx = int(src.shape[-2]), int(src.shape[-1])
            if ny * nx != self.n_src:
                raise ValueError("source planes have %d points, handle expects %d" % (ny * nx, self.n_src))
            ld = _level_stride(src, (nfields, nlev) if src.dim() == 4 else (nlev,), ny, nx, who)
        out_dtype = out_dtype or src.dtype
        if isinstance(out_dtype, np.dtype) or out_dtype in (np.float32, np.float64):
            out_dtype = torch.float32 if np.dtype(out_dtype) == np.float32 else torch.float64
        shape = (nfields, nlev, self.n_dst) if layout == LAYOUT_CELL_FAST else (nfields, self.n_dst, nlev)
        if out is None:
            out = torch.empty(shape, dtype=out_dtype, device=src.device)
        elif not (out.is_cuda and out.is_contiguous() and out.dtype in (torch.float32, torch.float64) and out.numel() == nfields * nlev * self.n_dst):
            raise ValueError(who + ": out must be a contiguous float32/float64 CUDA tensor of %d elements" % (nfields * nlev * self.n_dst))
        _account_regrid(self, nlev, nfields, src.element_size(), out.element_size())
        check(fn(self._h, src.data_ptr(), int(src.dtype == torch.float32), ld, int(nlev), int(nfields), out.data_ptr(),
                                   int(out.dtype == torch.float32), int(layout), float(scale), float(offset),
                                   torch.cuda.current_stream().cuda_stream))
        return out

    # -- rows to rows: MPAS file order in and out (the Regrid of a Mesh -> Mesh job) -----------------------
    def regrid_rows(self, src, nlev=1, nfields=1, out_dtype=None, scale=1.0, offset=0.0, out=None):
        """mpg_regrid_rows_dev: Regrid of a fixed-nnz handle (regrid_store_mesh's, but any 1-, 3- or 4-slot handle without pole caps)
        from [n_src][nlev] rows onto [n_dst][nlev] rows -- MPAS file order on both sides.  src: nfields slabs of (n_src, nlev), a
        contiguous float32 / float64 CUDA tensor.  Returns (nfields, n_dst, nlev) of out_dtype (default: src's) whose element [p][k] has
        the bits of element [k][p] of regrid_typed(layout=LAYOUT_LEV_FAST).  dst = cast(regrid(src) * scale + offset), float64
        arithmetic; an unmapped point gets cast(0.0 * scale + offset)."""
        return self._rows(L.regrid_rows_dev, "regrid_rows", src, nlev, nfields, out_dtype, scale, offset, out)

    def regrid_csr_rows(self, src, nlev=1, nfields=1, out_dtype=None, scale=1.0, offset=0.0, out=None):
        """mpg_regrid_csr_rows_dev: regrid_rows for CSR handles (regrid_store_conserve_mesh's, but any CSR handle without pole caps:
        both other conservative Stores', from_weights') -- [n_src][nlev] rows in, [n_dst][nlev] rows out, MPAS file order on both sides.
        Same arguments and result shape as regrid_rows; element [p][k] has the bits of element [k][p] of
        regrid_typed(layout=LAYOUT_LEV_FAST), an empty row gives cast(0.0 * scale + offset)."""
        return self._rows(L.regrid_csr_rows_dev, "regrid_csr_rows", src, nlev, nfields, out_dtype, scale, offset, out)

    def _rows(self, fn, who, src, nlev, nfields, out_dtype, scale, offset, out):
        import torch
        if not (_is_torch(src) and src.is_cuda and src.dtype in (torch.float32, torch.float64)):
            raise ValueError(who + " needs a float32/float64 CUDA tensor")
        if int(nlev) < 1 or int(nfields) < 1:
            raise ValueError(who + ": nlev and nfields must be >= 1")
        if not src.is_contiguous():
            raise ValueError(who + ": the source must be contiguous, nfields slabs of (n_src, nlev)")
        if src.numel() != nfields * nlev * self.n_src:
            raise ValueError("source has %d elements, handle expects %d" % (src.numel(), nfields * nlev * self.n_src))
        out_dtype = out_dtype or src.dtype
        if isinstance(out_dtype, np.dtype) or out_dtype in (np.float32, np.float64):
            out_dtype = torch.float32 if np.dtype(out_dtype) == np.float32 else torch.float64
        if out_dtype not in (torch.float32, torch.float64):
            raise ValueError(who + ": out_dtype must be float32 or float64")
        if out is None:
            out = torch.empty((nfields, self.n_dst, nlev), dtype=out_dtype, device=src.device)
        elif not (_is_torch(out) and out.is_cuda and out.is_contiguous() and out.dtype in (torch.float32, torch.float64) and
                  out.numel() == nfields * nlev * self.n_dst):
            raise ValueError("%s: out must be a contiguous float32/float64 CUDA tensor of %d elements" % (who, nfields * nlev * self.n_dst))
        _account_regrid(self, nlev, nfields, src.element_size(), out.element_size())
        check(fn(self._h, src.data_ptr(), int(src.dtype == torch.float32), int(nlev), int(nfields), out.data_ptr(),
                 int(out.dtype == torch.float32), float(scale), float(offset), torch.cuda.current_stream().cuda_stream))
        return out

    def dst_frac(self):
        """mpg_handle_get_dst_frac: the covered fraction of every destination cell, [n_dst] float64 (conservative Grid -> Mesh and Mesh -> Mesh handles)."""
        frac = np.empty(self.n_dst, np.float64)
        check(L.handle_get_dst_frac(self._h, _ptr(frac)))
        return frac

    def src_nearest(self):
        """mpg_handle_get_src_nearest: the destination every source chose, [n_src] int32 with -1 for none -- the binning index of a
        regrid_store_nearest_dtos handle (any other handle is refused)."""
        nearest = np.empty(self.n_src, np.int32)
        check(L.handle_get_src_nearest(self._h, _ptr(nearest)))
        return nearest

    def transpose_stats(self):
        """(n_referenced, max_per_source): sources with at least one entry and the longest transposed row
        (mpg_handle_transpose_stats; builds the transposed index if needed)."""
        a, b = C.c_int64(), C.c_int64()
        check(L.load().mpg_handle_transpose_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def transpose_build_ms(self):
        """GPU time of the transposed index build (mpg_handle_transpose_build_ms); 0.0 while none is built."""
        ms = C.c_float()
        check(L.load().mpg_handle_transpose_build_ms(self._h, C.byref(ms)))
        return ms.value

    # -- masked Regrid: dynamic masking / skipna + na_thres on the unmasked Store's weights ----------------
    def regrid_masked(self, src, nlev=1, nfields=1, layout=LAYOUT_CELL_FAST, missing="nan", src_mask=None, min_valid_frac=0.5,
                      fill_value=float("nan"), out_dtype=None, scale=1.0, offset=0.0, out=None):
        """mpg_regrid_masked_dev: Regrid from the valid sources only.  A source is invalid when it is statically masked (src_mask:
        bool / uint8 CUDA tensor of n_src, non-zero = never use) or its value is missing: missing = "nan", a number (a sentinel such
        as a file's _FillValue), a tuple of both, or None.  With a float32 source a numeric `missing` is rounded to float32 first,
        so that the file's sentinel compares equal.  A point whose valid weight Wv reaches min_valid_frac of its total weight Wt gets
        regrid_valid * Wt / Wv (then * scale + offset); every other point, unmapped ones included, gets fill_value.  With nothing
        missing the result equals regrid_typed's bit for bit on mapped points.
        src: contiguous float32 / float64 CUDA tensor of nfields * nlev * n_src elements; out may come from empty_pitched."""
        import torch
        if not (_is_torch(src) and src.is_cuda and src.is_contiguous() and src.dtype in (torch.float32, torch.float64)):
            raise ValueError("regrid_masked needs a contiguous float32/float64 CUDA tensor")
        if src.numel() != nfields * nlev * self.n_src:
            raise ValueError("source has %d elements, handle expects %d" % (src.numel(), nfields * nlev * self.n_src))
        flags, mv, mask_ptr = _parse_missing("regrid_masked", src, missing, src_mask, self.n_src)
        out_dtype = out_dtype or src.dtype
        if out is None:
            out = torch.empty((nfields, nlev, self.ny_dst, self.nx_dst), dtype=out_dtype, device=src.device)
        elif not (out.is_cuda and out.dtype in (torch.float32, torch.float64)):
            raise ValueError("regrid_masked: out must be a float32/float64 CUDA tensor")
        ld = _level_stride(out, (nfields, nlev), self.ny_dst, self.nx_dst, "regrid_masked")
        if ld == 0 and out.numel() != nfields * nlev * self.n_dst:
            raise ValueError("out has %d elements, handle produces %d" % (out.numel(), nfields * nlev * self.n_dst))
        opts = L.MaskOpts(flags, mv, mask_ptr, float(min_valid_frac), float(fill_value), float(scale), float(offset))
        _account_regrid(self, nlev, nfields, src.element_size(), out.element_size())
        check(L.regrid_masked_dev(self._h, src.data_ptr(), int(src.dtype == torch.float32), int(layout), int(nlev), int(nfields),
                                  out.data_ptr(), int(out.dtype == torch.float32), ld, C.byref(opts), torch.cuda.current_stream().cuda_stream))
        return out

    def regrid_masked_transpose(self, grad, src, nlev=1, nfields=1, layout=LAYOUT_CELL_FAST, missing="nan", src_mask=None, min_valid_frac=0.5,
                                scale=1.0, out_dtype=None, out=None, work=None):
        """mpg_regrid_masked_transpose_dev: the adjoint of regrid_masked -- the gradient with respect to `src` from `grad`, the gradient
        with respect to regrid_masked's result.  `src`, `layout`, `missing`, `src_mask`, `min_valid_frac` and `scale` are the forward
        call's (missing is parsed as regrid_masked parses it); `src` is read only to decide which elements are valid.  The gradient
        at a missing or statically masked source is exactly 0 (never NaN), and `grad` at filled outputs -- undefined and unmapped points
        -- is ignored, NaN included.  With nothing missing and scale 1 the result equals regrid_transpose(grad) bit for bit on a
        handle that maps every point.
        grad: [nfields][nlev][ny_dst][nx_dst] float32 / float64 CUDA tensor, contiguous or a plane-pitched view as empty_pitched makes.
        work: float64 CUDA workspace of nfields * nlev * n_dst elements (allocated when None); on return it holds the scaled gradient
        grad * scale * Wt / Wv, 0 at filled outputs.  Returns nfields slabs of nlev * n_src values of out_dtype (default: src's) in
        `layout`: (nfields, nlev, n_src) for LAYOUT_CELL_FAST, (nfields, n_src, nlev) for LAYOUT_LEV_FAST."""
        import torch
        who = "regrid_masked_transpose"
        if not (_is_torch(src) and src.is_cuda and src.is_contiguous() and src.dtype in (torch.float32, torch.float64)):
            raise ValueError(who + " needs a contiguous float32/float64 CUDA tensor as src")
        if src.numel() != nfields * nlev * self.n_src:
            raise ValueError("source has %d elements, handle expects %d" % (src.numel(), nfields * nlev * self.n_src))
        if not (_is_torch(grad) and grad.is_cuda and grad.dtype in (torch.float32, torch.float64)):
            raise ValueError(who + " needs a float32/float64 CUDA tensor as grad")
        if grad.is_contiguous():
            if grad.numel() != nfields * nlev * self.n_dst:
                raise ValueError("grad has %d elements, handle expects %d" % (grad.numel(), nfields * nlev * self.n_dst))
            ld = 0
        else:
            lead = (nfields, nlev) if grad.dim() == 4 else (nlev,)
            if grad.dim() not in (3, 4) or (grad.dim() == 3 and nfields != 1):
                raise ValueError(who + ": a strided grad must be (nfields, nlev, ny, nx) or (nlev, ny, nx) with plane-pitched levels")
            ld = _level_stride(grad, lead, self.ny_dst, self.nx_dst, who)
        flags, mv, mask_ptr = _parse_missing(who, src, missing, src_mask, self.n_src)
        out_dtype = out_dtype or src.dtype
        if isinstance(out_dtype, np.dtype) or out_dtype in (np.float32, np.float64):
            out_dtype = torch.float32 if np.dtype(out_dtype) == np.float32 else torch.float64
        shape = (nfields, nlev, self.n_src) if layout == LAYOUT_CELL_FAST else (nfields, self.n_src, nlev)
        if out is None:
            out = torch.empty(shape, dtype=out_dtype, device=src.device)
        elif not (out.is_cuda and out.is_contiguous() and out.dtype in (torch.float32, torch.float64) and out.numel() == nfields * nlev * self.n_src):
            raise ValueError(who + ": out must be a contiguous float32/float64 CUDA tensor of %d elements" % (nfields * nlev * self.n_src))
        if work is None:
            work = torch.empty((nfields, nlev, self.n_dst), dtype=torch.float64, device=src.device)
        elif not (_is_torch(work) and work.is_cuda and work.is_contiguous() and work.dtype == torch.float64 and work.numel() == nfields * nlev * self.n_dst):
            raise ValueError(who + ": work must be a contiguous float64 CUDA tensor of %d elements" % (nfields * nlev * self.n_dst))
        opts = L.MaskOpts(flags, mv, mask_ptr, float(min_valid_frac), 0.0, float(scale), 0.0)
        check(L.regrid_masked_transpose_dev(self._h, grad.data_ptr(), int(grad.dtype == torch.float32), ld, src.data_ptr(),
                                            int(src.dtype == torch.float32), int(layout), int(nlev), int(nfields), out.data_ptr(),
                                            int(out.dtype == torch.float32), C.byref(opts), work.data_ptr(), torch.cuda.current_stream().cuda_stream))
        return out

    @classmethod
    def from_weights(cls, n_src, nx_dst, ny_dst, row, col, S):
        """Route handle from externally computed weights in ESMF's factorList / factorIndexList form (1-based
        row = destination j*nx+i, col = source), e.g. the S/row/col of an ESMF_RegridWeightGen file."""
        row = np.ascontiguousarray(row, np.int32)
        col = np.ascontiguousarray(col, np.int32)
        S = _f64(S)
        if not (row.size == col.size == S.size):
            raise ValueError("row, col and S must have the same length")
        h = C.c_void_p()
        check(L.load().mpg_handle_from_weights(C.c_int64(n_src), C.c_int(nx_dst), C.c_int(ny_dst), C.c_int64(S.size), _ptr(row), _ptr(col),
                                               _ptr(S), C.byref(h)))
        return cls(h)

    def to_esmf_weights(self):
        """(row, col, S), 1-based, unmapped destination points omitted: what ESMF would return as factorIndexList /
        factorList for the same regrid (nearest: S = 1)."""
        if self.nnz_per_row == 0:
            rowptr, col, val = self.csr()
            row = np.repeat(np.arange(1, self.n_dst + 1, dtype=np.int32), np.diff(rowptr).astype(np.int64))
            return row, (col + 1).astype(np.int32), val
        idx, w = self.weights()
        keep = idx >= 0
        row = np.broadcast_to(np.arange(1, self.n_dst + 1, dtype=np.int32)[:, None], idx.shape)[keep]
        row, col, S = np.ascontiguousarray(row), (idx[keep] + 1).astype(np.int32), np.ascontiguousarray(w[keep])
        dst, src0, wp, row_len = self.pole()
        if len(dst):
            # a pole node's value is the mean of one CENTER row: row_len factors of w_pole / row_len each
            nz = wp != 0.0
            prow = np.repeat(dst[nz] + 1, row_len).astype(np.int32)
            pcol = (src0[nz][:, None] + np.arange(1, row_len + 1, dtype=np.int32)[None, :]).reshape(-1).astype(np.int32)
            row, col, S = np.concatenate([row, prow]), np.concatenate([col, pcol]), np.concatenate([S, np.repeat(wp[nz] / row_len, row_len)])
            keep = S != 0.0                                      # the cap points' zero-weight filler slots
            row, col, S = row[keep], col[keep], S[keep]
        return row, col, S

    def kernel_choice(self):
        """(cell_fast, lev_fast, max_unique): which Regrid kernel serves this handle (mpg_handle_kernel_choice)."""
        cf, lf, mu = C.c_int(), C.c_int(), C.c_int()
        check(L.load().mpg_handle_kernel_choice(self._h, C.byref(cf), C.byref(lf), C.byref(mu)))
        return cf.value, lf.value, mu.value

    def tile_stats(self):
        """(tile_nx, tile_ny, reuse, line_fill) of the tile lists in use (mpg_handle_tile_stats); None before the first
        staged Regrid of the handle."""
        tx, ty, reuse, fill = C.c_int(), C.c_int(), C.c_double(), C.c_double()
        if L.load().mpg_handle_tile_stats(self._h, C.byref(tx), C.byref(ty), C.byref(reuse), C.byref(fill)) != L.MPG_SUCCESS:
            return None
        return tx.value, ty.value, reuse.value, fill.value

    def pole(self):
        """Pole terms of a Grid -> Grid handle on a periodic grid: (dst_id, src_row_start, w_pole, row_len);
        empty arrays for every other handle (mpg_handle_get_pole)."""
        n, row_len = C.c_int64(), C.c_int()
        check(L.load().mpg_handle_pole_count(self._h, C.byref(n), C.byref(row_len)))
        dst, src0, wp = np.empty(n.value, np.int32), np.empty(n.value, np.int32), np.empty(n.value)
        if n.value:
            check(L.load().mpg_handle_get_pole(self._h, _ptr(dst), _ptr(src0), _ptr(wp)))
        return dst, src0, wp, row_len.value

    def weights(self):
        """(idx [n_dst][nnz_per_row] int32 with -1 = unmapped, w [n_dst][nnz_per_row])."""
        idx = np.empty((self.n_dst, self.nnz_per_row), np.int32)
        w = np.empty((self.n_dst, self.nnz_per_row))
        check(L.load().mpg_handle_get_weights(self._h, _ptr(idx), _ptr(w)))
        return idx, w

    def csr(self):
        rowptr = np.empty(self.n_dst + 1, np.int64)
        col, val = np.empty(self.nnz, np.int32), np.empty(self.nnz)
        check(L.load().mpg_handle_get_csr(self._h, _ptr(rowptr), _ptr(col), _ptr(val)))
        return rowptr, col, val

    def unique_sources(self):
        n = C.c_int64()
        check(L.load().mpg_handle_unique_sources(self._h, C.byref(n), None))
        ids = np.empty(n.value, np.int32)
        if n.value:
            check(L.load().mpg_handle_unique_sources(self._h, C.byref(n), _ptr(ids)))
        return ids

    def source_range(self):
        """(first, end): the global source ids this Mesh -> Grid handle references (mpg_handle_source_range)."""
        a, b = C.c_int64(), C.c_int64()
        check(L.load().mpg_handle_source_range(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def localize(self):
        ids = self.unique_sources()
        check(L.load().mpg_handle_localize(self._h))
        self._refresh()
        return ids

    def rebase(self, base, n_local):
        check(L.load().mpg_handle_rebase(self._h, C.c_int64(base), C.c_int64(n_local)))
        self._refresh()

    def release(self):
        if self._h:
            check(L.load().mpg_handle_release(self._h))
            self._h = None


try:   # the differentiable Regrid needs torch; the rest of this module does not
    import torch as _torch
except ImportError:
    _torch = None

if _torch is not None:
    class RegridFunction(_torch.autograd.Function):
        """Regrid with a gradient: forward is regrid_typed (scale 1, offset 0) in src's dtype, backward is regrid_transpose into
        src's layout and dtype.  Use regrid_autograd()."""

        @staticmethod
        def forward(ctx, src, rh, nlev, nfields, layout):
            ctx.rh, ctx.nlev, ctx.nfields, ctx.layout = rh, nlev, nfields, layout
            ctx.src_shape, ctx.src_dtype = src.shape, src.dtype
            return rh.regrid_typed(src.contiguous(), nlev=nlev, nfields=nfields, layout=layout, out_dtype=src.dtype)

        @staticmethod
        def backward(ctx, grad):
            g = ctx.rh.regrid_transpose(grad.contiguous(), nlev=ctx.nlev, nfields=ctx.nfields, layout=ctx.layout, out_dtype=ctx.src_dtype)
            return g.reshape(ctx.src_shape), None, None, None, None


def regrid_autograd(rh, src, nlev=1, nfields=1, layout=LAYOUT_CELL_FAST):
    """rh.regrid_typed(src) (float32 or float64 CUDA tensor, scale 1, offset 0) as a differentiable torch op: the gradient with
    respect to src is rh.regrid_transpose of the incoming gradient, in src's layout and dtype."""
    return RegridFunction.apply(src, rh, nlev, nfields, layout)


if _torch is not None:
    class RegridMaskedFunction(_torch.autograd.Function):
        """regrid_masked with a gradient: forward is regrid_masked (scale 1, offset 0) in src's dtype, backward is
        regrid_masked_transpose of the same handle, source and options into src's layout and dtype.  Use regrid_masked_autograd()."""

        @staticmethod
        def forward(ctx, src, rh, nlev, nfields, layout, missing, src_mask, min_valid_frac, fill_value):
            ctx.rh, ctx.nlev, ctx.nfields, ctx.layout = rh, nlev, nfields, layout
            ctx.missing, ctx.src_mask, ctx.min_valid_frac = missing, src_mask, min_valid_frac
            ctx.src_shape = src.shape
            data = src.detach().contiguous()
            ctx.save_for_backward(data)         # read again only to decide which elements were valid
            return rh.regrid_masked(data, nlev=nlev, nfields=nfields, layout=layout, missing=missing, src_mask=src_mask,
                                    min_valid_frac=min_valid_frac, fill_value=fill_value, out_dtype=src.dtype)

        @staticmethod
        def backward(ctx, grad):
            data, = ctx.saved_tensors
            g = ctx.rh.regrid_masked_transpose(grad.contiguous(), data, nlev=ctx.nlev, nfields=ctx.nfields, layout=ctx.layout, missing=ctx.missing,
                                               src_mask=ctx.src_mask, min_valid_frac=ctx.min_valid_frac, out_dtype=data.dtype)
            return (g.reshape(ctx.src_shape),) + (None,) * 8


def regrid_masked_autograd(rh, src, nlev=1, nfields=1, layout=LAYOUT_CELL_FAST, missing="nan", src_mask=None, min_valid_frac=0.5,
                           fill_value=float("nan")):
    """rh.regrid_masked(src) (float32 or float64 CUDA tensor, scale 1, offset 0) as a differentiable torch op; `layout`, `missing`,
    `src_mask`, `min_valid_frac` and `fill_value` as regrid_masked takes them.  The gradient with respect to src is
    rh.regrid_masked_transpose of the incoming gradient, in src's layout and dtype: the exact derivative at every valid source element.
    The gradient at a missing or statically masked source is 0, not NaN (such an element never entered the result), and the incoming
    gradient at filled outputs -- undefined and unmapped points, whose value is the constant fill_value -- is ignored, a NaN there
    included.  The first backward on a handle builds its transposed index."""
    return RegridMaskedFunction.apply(src, rh, nlev, nfields, layout, missing, src_mask, min_valid_frac, fill_value)


if _torch is not None:
    class RegridToMeshFunction(_torch.autograd.Function):
        """regrid_to_mesh with a gradient: forward is regrid_to_mesh (scale 1, offset 0) in src's dtype, backward is regrid_transpose
        of the same handle, fed the incoming gradient in the forward's destination layout.  Use regrid_to_mesh_autograd()."""

        @staticmethod
        def forward(ctx, src, rh, nlev, nfields, layout):
            ctx.rh, ctx.nlev, ctx.nfields, ctx.layout = rh, nlev, nfields, layout
            ctx.src_shape, ctx.src_dtype = src.shape, src.dtype
            return rh.regrid_to_mesh(src.contiguous(), nlev=nlev, nfields=nfields, layout=layout, out_dtype=src.dtype)

        @staticmethod
        def backward(ctx, grad):
            # regrid_transpose reads [nfields][nlev][n_dst] planes: a gradient in [cell][lev] order goes back to [lev][cell] first
            if ctx.layout == LAYOUT_LEV_FAST:
                grad = grad.reshape(ctx.nfields, ctx.rh.n_dst, ctx.nlev).transpose(1, 2)
            g = ctx.rh.regrid_transpose(grad.contiguous(), nlev=ctx.nlev, nfields=ctx.nfields, layout=LAYOUT_CELL_FAST, out_dtype=ctx.src_dtype)
            return g.reshape(ctx.src_shape), None, None, None, None


def regrid_to_mesh_autograd(rh, src, nlev=1, nfields=1, layout=LAYOUT_CELL_FAST):
    """rh.regrid_to_mesh(src) (float32 or float64 CUDA tensor of [nfields][nlev][n_src] grid values, scale 1, offset 0) as a
    differentiable torch op; `layout` is the destination layout.  The gradient with respect to src is rh.regrid_transpose of the
    incoming gradient, in src's shape and dtype."""
    return RegridToMeshFunction.apply(src, rh, nlev, nfields, layout)


if _torch is not None:
    class RegridCsrToMeshFunction(_torch.autograd.Function):
        """regrid_csr_to_mesh with a gradient: RegridToMeshFunction for CSR handles.  Use regrid_csr_to_mesh_autograd()."""

        @staticmethod
        def forward(ctx, src, rh, nlev, nfields, layout):
            ctx.rh, ctx.nlev, ctx.nfields, ctx.layout = rh, nlev, nfields, layout
            ctx.src_shape, ctx.src_dtype = src.shape, src.dtype
            return rh.regrid_csr_to_mesh(src.contiguous(), nlev=nlev, nfields=nfields, layout=layout, out_dtype=src.dtype)

        backward = RegridToMeshFunction.backward


def regrid_csr_to_mesh_autograd(rh, src, nlev=1, nfields=1, layout=LAYOUT_CELL_FAST):
    """rh.regrid_csr_to_mesh(src) (scale 1, offset 0) as a differentiable torch op; `layout` is the destination layout.  The gradient
    with respect to src is rh.regrid_transpose of the same handle applied to the incoming gradient, in src's shape and dtype."""
    return RegridCsrToMeshFunction.apply(src, rh, nlev, nfields, layout)


if _torch is not None:
    class RegridRowsFunction(_torch.autograd.Function):
        """regrid_rows with a gradient: forward is regrid_rows (scale 1, offset 0) in src's dtype, backward is regrid_transpose of the
        same handle with layout=LAYOUT_LEV_FAST, so the gradient comes back as [n_src][nlev] rows.  Use regrid_rows_autograd()."""

        @staticmethod
        def forward(ctx, src, rh, nlev, nfields):
            ctx.rh, ctx.nlev, ctx.nfields = rh, nlev, nfields
            ctx.src_shape, ctx.src_dtype = src.shape, src.dtype
            return rh.regrid_rows(src.contiguous(), nlev=nlev, nfields=nfields, out_dtype=src.dtype)

        @staticmethod
        def backward(ctx, grad):
            # regrid_transpose reads [nfields][nlev][n_dst] planes: the incoming [cell][lev] gradient goes to [lev][cell] first
            grad = grad.reshape(ctx.nfields, ctx.rh.n_dst, ctx.nlev).transpose(1, 2)
            g = ctx.rh.regrid_transpose(grad.contiguous(), nlev=ctx.nlev, nfields=ctx.nfields, layout=LAYOUT_LEV_FAST, out_dtype=ctx.src_dtype)
            return g.reshape(ctx.src_shape), None, None, None


def regrid_rows_autograd(rh, src, nlev=1, nfields=1):
    """rh.regrid_rows(src) (float32 or float64 CUDA tensor of nfields slabs of (n_src, nlev), scale 1, offset 0) as a differentiable
    torch op.  The gradient with respect to src is rh.regrid_transpose(..., layout=LAYOUT_LEV_FAST) of the incoming gradient, in src's
    shape and dtype."""
    return RegridRowsFunction.apply(src, rh, nlev, nfields)


if _torch is not None:
    class RegridCsrRowsFunction(_torch.autograd.Function):
        """regrid_csr_rows with a gradient: RegridRowsFunction for CSR handles.  Use regrid_csr_rows_autograd()."""

        @staticmethod
        def forward(ctx, src, rh, nlev, nfields):
            ctx.rh, ctx.nlev, ctx.nfields = rh, nlev, nfields
            ctx.src_shape, ctx.src_dtype = src.shape, src.dtype
            return rh.regrid_csr_rows(src.contiguous(), nlev=nlev, nfields=nfields, out_dtype=src.dtype)

        backward = RegridRowsFunction.backward


def regrid_csr_rows_autograd(rh, src, nlev=1, nfields=1):
    """rh.regrid_csr_rows(src) (scale 1, offset 0) as a differentiable torch op.  The gradient with respect to src is
    rh.regrid_transpose(..., layout=LAYOUT_LEV_FAST) of the same handle applied to the incoming gradient, in src's shape and dtype."""
    return RegridCsrRowsFunction.apply(src, rh, nlev, nfields)


def regrid_store_conserve_mesh(src_mesh, dst_mesh, norm=NORM_DSTAREA):
    """ESMF_FieldRegridStore(mesh field -> mesh field, regridmethod=CONSERVE, normType=norm): the source mesh's Voronoi cells onto the
    destination mesh's, first-order conservative.  NORM_DSTAREA: w = I / area(cell); NORM_FRACAREA: w = I / covered area.  A CSR handle
    (n_src = the source nCells, n_dst = the destination nCells): regrid_typed, regrid_masked, regrid_transpose, csr() and dst_frac()
    work on it, regrid_csr_rows reads and writes MPAS file order.  Meshes made with window_grid= are refused by the library."""
    if not (isinstance(src_mesh, Mesh) and isinstance(dst_mesh, Mesh)):
        raise TypeError("regrid_store_conserve_mesh: src_mesh and dst_mesh must be Mesh objects")
    if norm not in (NORM_DSTAREA, NORM_FRACAREA):
        raise ValueError("regrid_store_conserve_mesh: norm must be NORM_DSTAREA or NORM_FRACAREA, not %r" % (norm,))
    h = C.c_void_p()
    check(L.regrid_store_conserve_mesh(src_mesh._h, dst_mesh._h, int(norm), C.byref(h)))
    return RouteHandle(h)


def regrid_store_mesh(src_mesh, dst_mesh, regridmethod=REGRIDMETHOD_BILINEAR, src_meshloc=MESHLOC_ELEMENT, dst_meshloc=MESHLOC_ELEMENT):
    """ESMF_FieldRegridStore(mesh field -> mesh field): the source mesh's cell centres onto the destination mesh's cells
    (MESHLOC_ELEMENT) or vertices (MESHLOC_NODE), bilinear (the source mesh's dual triangles, the lowest passing triangle id) or
    nearest.  The handle is an ordinary fixed one (n_src = the source nCells, n_dst = the destination count): regrid_typed,
    regrid_masked, regrid_transpose, regrid_to_mesh and the getters work on it; regrid_rows reads and writes MPAS file order.
    Conservative (regrid_store_conserve_mesh is that Store), node-located sources and meshes made with window_grid= are refused by the
    library (MpgError, rc 4)."""
    if not (isinstance(src_mesh, Mesh) and isinstance(dst_mesh, Mesh)):
        raise TypeError("regrid_store_mesh: src_mesh and dst_mesh must be Mesh objects")
    if regridmethod not in (REGRIDMETHOD_BILINEAR, REGRIDMETHOD_CONSERVE, REGRIDMETHOD_NEAREST_STOD):
        raise ValueError("regrid_store_mesh: unknown regridmethod %r" % (regridmethod,))
    for loc in (src_meshloc, dst_meshloc):
        if loc not in (MESHLOC_ELEMENT, MESHLOC_NODE):
            raise ValueError("regrid_store_mesh: unknown mesh location %r" % (loc,))
    h = C.c_void_p()
    check(L.regrid_store_mesh(src_mesh._h, int(src_meshloc), dst_mesh._h, int(dst_meshloc), int(regridmethod), C.byref(h)))
    return RouteHandle(h)


def regrid_store_conserve_to_mesh(src_grid, dst_mesh, norm=NORM_DSTAREA):
    """ESMF_FieldRegridStore(grid field -> mesh field, regridmethod=CONSERVE, normType=norm): the grid's cells (CORNER polygons) onto the
    mesh's Voronoi cells, first-order conservative.  NORM_DSTAREA: w = I / area(cell); NORM_FRACAREA: w = I / covered area.  A CSR
    handle (n_dst = nCells): regrid_typed, regrid_masked, regrid_transpose, csr() and dst_frac() work on it, regrid_csr_to_mesh writes
    the mesh's own memory orders."""
    h = C.c_void_p()
    check(L.regrid_store_conserve_to_mesh(src_grid._h, dst_mesh._h, int(norm), C.byref(h)))
    return RouteHandle(h)


def regrid_store_to_mesh(src_grid, dst_mesh, regridmethod=REGRIDMETHOD_BILINEAR, staggerloc=STAGGERLOC_CENTER, meshloc=MESHLOC_ELEMENT):
    """ESMF_FieldRegridStore(grid field -> mesh field): the grid's `staggerloc` points onto the mesh's cells (MESHLOC_ELEMENT) or
    vertices (MESHLOC_NODE), bilinear or nearest -- or, on a mesh with edges (Mesh.set_edges), onto its edge points (MESHLOC_EDGE).  The
    handle is an ordinary fixed one (n_dst = the mesh count): regrid_typed,
    regrid_masked, regrid_transpose and the getters work on it, regrid_to_mesh writes the mesh's own memory orders."""
    h = C.c_void_p()
    check(L.regrid_store_to_mesh(src_grid._h, int(staggerloc), dst_mesh._h, int(meshloc), int(regridmethod), C.byref(h)))
    return RouteHandle(h)


def regrid_store_periodic_to_mesh(src_grid, dst_mesh, meshloc=MESHLOC_ELEMENT, pole_method=POLEMETHOD_ALLAVG):
    """ESMF_FieldRegridStore(grid field -> mesh field, regridmethod=BILINEAR, polemethod=pole_method) from a grid that is periodic in i
    (Grid(..., periodic=True), a global Grid.from_target / from_proj): the CENTER points onto the mesh's cells (MESHLOC_ELEMENT) or vertices
    (MESHLOC_NODE) or, on a mesh with edges (Mesh.set_edges; without them rc 2), its edge points (MESHLOC_EDGE: the handle
    wind_csr_to_edges takes), the seam column between i = nx - 1 and i = 0 and -- under POLEMETHOD_ALLAVG -- the pole caps included; POLEMETHOD_NONE
    leaves the points poleward of the first and last row unmapped.  Each end row closes on the pole of its own hemisphere (the sign of the
    row's mean z), so the rows may be numbered south to north or north to south (GRIB, ERA5, the Gaussian grids); GRID_NO_SOUTH_POLE /
    GRID_NO_NORTH_POLE name the row-0 / row-(ny-1) end of a row block, and two live ends in one hemisphere are refused (rc 2).  A CSR handle without pole terms (n_dst = the mesh count; quad rows of 4
    entries, cap rows of nx): regrid_csr_to_mesh writes the mesh's own memory orders, regrid_csr_rows, regrid_typed, regrid_masked,
    regrid_transpose, csr() and to_esmf_weights() work on it.  A non-periodic grid is refused (MpgError, rc 4): regrid_store_to_mesh is
    its Store."""
    if not (isinstance(src_grid, Grid) and isinstance(dst_mesh, Mesh)):
        raise TypeError("regrid_store_periodic_to_mesh: src_grid must be a Grid and dst_mesh a Mesh")
    h = C.c_void_p()
    check(L.regrid_store_periodic_to_mesh(src_grid._h, dst_mesh._h, int(meshloc), int(pole_method), C.byref(h)))
    return RouteHandle(h)


def regrid_store_grid_to_grid(src_grid, dst_grid, regridmethod=REGRIDMETHOD_BILINEAR, src_staggerloc=STAGGERLOC_CENTER,
                              dst_staggerloc=STAGGERLOC_CENTER, pole_method=POLEMETHOD_ALLAVG):
    """ESMF_FieldRegridStore(grid field -> grid field) between two grids (or two staggers of one): the `src_staggerloc` points of src_grid
    onto the `dst_staggerloc` points of dst_grid, bilinear or nearest -- a lat-lon analysis onto the target grid, a parent domain onto its
    nest and back, results onto a verification grid.  From a non-periodic grid the handle is fixed (4 slots bilinear, unmapped points idx
    -1; 1 slot nearest, every point mapped); bilinear from a grid periodic in i (CENTER points only) gives the CSR handle of
    regrid_store_periodic_to_mesh with the seam column and, under POLEMETHOD_ALLAVG, the pole caps; pole_method is ignored otherwise.
    n_dst = dnx * dny and every Regrid writes [lev][dny][dnx].  Conservative is refused (MpgError, rc 4):
    regrid_store_conserve_grid_to_grid is that Store."""
    if not (isinstance(src_grid, Grid) and isinstance(dst_grid, Grid)):
        raise TypeError("regrid_store_grid_to_grid: src_grid and dst_grid must be Grid objects")
    h = C.c_void_p()
    check(L.regrid_store_grid_to_grid(src_grid._h, int(src_staggerloc), dst_grid._h, int(dst_staggerloc), int(regridmethod), int(pole_method),
                                      C.byref(h)))
    return RouteHandle(h)


def regrid_store_conserve_grid_to_grid(src_grid, dst_grid, norm=NORM_DSTAREA):
    """ESMF_FieldRegridStore(grid field -> grid field, regridmethod=CONSERVE, normType=norm): the cells of src_grid (CORNER quadrilaterals)
    onto the cells of dst_grid, first-order conservative.  NORM_DSTAREA: w = I / area(cell); NORM_FRACAREA: w = I / covered area.  A CSR
    handle (n_src = snx * sny, n_dst = dnx * dny, results [lev][dny][dnx]): regrid_typed, regrid_masked, regrid_transpose, csr() and
    dst_frac() work on it.  Both grids need CORNER coordinates (rc 2 without)."""
    if not (isinstance(src_grid, Grid) and isinstance(dst_grid, Grid)):
        raise TypeError("regrid_store_conserve_grid_to_grid: src_grid and dst_grid must be Grid objects")
    if norm not in (NORM_DSTAREA, NORM_FRACAREA):
        raise ValueError("regrid_store_conserve_grid_to_grid: norm must be NORM_DSTAREA or NORM_FRACAREA, not %r" % (norm,))
    h = C.c_void_p()
    check(L.regrid_store_conserve_grid_to_grid(src_grid._h, dst_grid._h, int(norm), C.byref(h)))
    return RouteHandle(h)


def regrid_store(src_mesh, dst_grid, regridmethod=REGRIDMETHOD_BILINEAR, staggerloc=STAGGERLOC_CENTER,
                 meshloc=MESHLOC_ELEMENT):
    """ESMF_FieldRegridStore(mesh field -> grid field); srcTermProcessing=1, unmappedaction=IGNORE."""
    h = C.c_void_p()
    check(L.load().mpg_regrid_store(src_mesh._h, C.c_int(meshloc), dst_grid._h, C.c_int(staggerloc), C.c_int(regridmethod), C.byref(h)))
    return RouteHandle(h)


def regrid_store_grid(grid, dst_staggerloc, src_staggerloc=STAGGERLOC_CENTER, regridmethod=REGRIDMETHOD_BILINEAR):
    """ESMF_FieldRegridStore(u_target_grid_nostag -> u_target_grid) (interp.F90:298,316)."""
    h = C.c_void_p()
    check(L.load().mpg_regrid_store_grid(grid._h, C.c_int(src_staggerloc), C.c_int(dst_staggerloc), C.c_int(regridmethod), C.byref(h)))
    return RouteHandle(h)


def regrid_store_begin(src_mesh, dst_grid, regridmethod=REGRIDMETHOD_BILINEAR, staggerloc=STAGGERLOC_CENTER, meshloc=MESHLOC_ELEMENT):
    """mpg_regrid_store_begin: the Store of regrid_store(same arguments) STARTED on the library's worker thread; returns at once.  The later
    regrid_store returns the finished handle (waiting for what is left of it)."""
    check(L.load().mpg_regrid_store_begin(src_mesh._h, C.c_int(meshloc), dst_grid._h, C.c_int(staggerloc), C.c_int(regridmethod)))


def regrid_store_grid_begin(grid, dst_staggerloc, src_staggerloc=STAGGERLOC_CENTER, regridmethod=REGRIDMETHOD_BILINEAR):
    """mpg_regrid_store_grid_begin: regrid_store_grid(same arguments) started in the background."""
    check(L.load().mpg_regrid_store_grid_begin(grid._h, C.c_int(src_staggerloc), C.c_int(dst_staggerloc), C.c_int(regridmethod)))


def rotate_winds_cgrid(cosa, sina, u, v):
    """rotate_winds_cgrid (interp.F90:689-749), in place.  u, v: [nlev][ny][nx] (or [ny][nx]); numpy or torch."""
    if _is_torch(u):
        npts = cosa.numel()
        nlev = u.numel() // npts
        if ACCOUNT is not None:                 # u, v read and written once, cos / sin(alpha) read once
            ACCOUNT.append(("rotate L%d" % nlev, npts * (nlev * 32 + 16)))
        check(L.load().mpg_rotate_winds_dev(C.c_int64(npts), C.c_int(nlev), C.c_void_p(cosa.data_ptr()), C.c_void_p(sina.data_ptr()),
                                            C.c_void_p(u.data_ptr()), C.c_void_p(v.data_ptr()), _stream_ptr()))
        return u, v
    cosa, sina = _f64(cosa), _f64(sina)
    if not (u.flags.c_contiguous and v.flags.c_contiguous and u.dtype == np.float64 and v.dtype == np.float64):
        raise ValueError("u, v must be contiguous float64 (rotated in place)")
    npts = cosa.size
    nlev = u.size // npts
    check(L.load().mpg_rotate_winds(C.c_int64(npts), C.c_int(nlev), _ptr(cosa), _ptr(sina), _ptr(u), _ptr(v)))
    return u, v


def wind_destagger(rh_u, rh_v, cosa, sina, umass, vmass, nlev, out_dtype=None, dst_be=False, keep_mass=False, outs=None):
    """interp.F90:291-328 in one pass (mpg_wind_destagger_dev; numpy arrays: mpg_wind_destagger): rotate_winds_cgrid on the CENTER-stagger winds (cosa / sina
    None: no rotation) + UMASS -> U(EDGE1) + VMASS -> V(EDGE2).  rh_u / rh_v: the regrid_store_grid handles of ONE grid (either
    may be None); umass / vmass: float64 CUDA tensors (or numpy arrays) [nlev][ny][nx], not modified.  Returns (U, V, UMASS', VMASS'): U
    [nlev][ny][nx+1], V [nlev][ny+1][nx] of out_dtype (float64), the rotated mass winds only with keep_mass (else None).
    Bit-identical to rotate_winds_cgrid followed by the two handles' regrid().  Raises MpgError(rc = MPG_ERR_UNSUPPORTED) for
    handles that are not such a pair (re-indexed ones).  outs=(U, V) (device only): tensors to write into, dense or plane-pitched
    (rh_u.empty_pitched / rh_v.empty_pitched) with ONE level stride for both (at least the larger plane: use the larger of the two
    handles' level_stride)."""
    ref = umass if umass is not None else vmass
    rot = cosa is not None
    if not _is_torch(ref):
        if outs is not None:
            raise ValueError("wind_destagger: outs= takes device tensors; the host-array chain returns new arrays")
        # HOST arrays (mpg_wind_destagger): the mass winds cross the link once, U and V come back -- 2 fields up, 2 down, where
        # rotate_winds_cgrid + two regrid() calls move 4 up and 4 down.  keep_mass: the rotated mass winds are returned as new arrays.
        out_np = np.dtype(out_dtype or np.float64)
        if out_np not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError("wind_destagger: out_dtype must be float64 or float32")
        um = _f64(umass) if umass is not None else None
        vm = _f64(vmass) if vmass is not None else None
        ca, sa = (_f64(cosa), _f64(sina)) if rot else (None, None)
        u = np.empty((nlev, rh_u.ny_dst, rh_u.nx_dst), dtype=out_np) if rh_u is not None else None
        v = np.empty((nlev, rh_v.ny_dst, rh_v.nx_dst), dtype=out_np) if rh_v is not None else None
        ur = np.empty_like(um) if (keep_mass and rot) else None
        vr = np.empty_like(vm) if (keep_mass and rot) else None

        def hp(a):
            return _ptr(a) if a is not None else None
        check(L.load().mpg_wind_destagger(rh_u._h if rh_u is not None else None, rh_v._h if rh_v is not None else None, hp(ca), hp(sa), hp(um), hp(vm),
                                          C.c_int(nlev), hp(u), hp(v), C.c_int(int(out_np == np.dtype(np.float32)) | (2 if dst_be else 0)), hp(ur), hp(vr)))
        return u, v, ur, vr
    import torch
    given = [t for t in (outs or ()) if t is not None]
    out_dtype = out_dtype or (given[0].dtype if given else torch.float64)
    for t in (umass, vmass):
        if t is not None and not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float64):
            raise ValueError("wind_destagger needs contiguous float64 CUDA tensors")
    u, v = outs if outs is not None else (None, None)
    if u is None and rh_u is not None:
        u = torch.empty((nlev, rh_u.ny_dst, rh_u.nx_dst), dtype=out_dtype, device=ref.device)
    if v is None and rh_v is not None:
        v = torch.empty((nlev, rh_v.ny_dst, rh_v.nx_dst), dtype=out_dtype, device=ref.device)
    lds = set()
    for t, rh in ((u, rh_u), (v, rh_v)):
        if t is None or rh is None:
            continue
        if not (t.is_cuda and t.dtype == out_dtype and t.numel() == nlev * rh.n_dst):
            raise ValueError("wind_destagger: bad destination tensor")
        lead = tuple(t.shape[:-2]) if t.dim() == 4 else (nlev,)
        lds.add(_level_stride(t, lead, rh.ny_dst, rh.nx_dst, "wind_destagger"))
    if len(lds) > 1:
        raise ValueError("wind_destagger: U and V must share one level stride (or both be dense)")
    ld = lds.pop() if lds else 0
    ur = torch.empty_like(umass) if (keep_mass and rot) else None
    vr = torch.empty_like(vmass) if (keep_mass and rot) else None
    if ACCOUNT is not None:     # both mass fields read once, U and V written once, indices + weights of both handles and the angles once
        npts = ref.numel() // nlev
        es = 4 if out_dtype == torch.float32 else 8
        by = 0
        if rh_u is not None:
            by += nlev * (npts * 8 + rh_u.n_dst * es) + rh_u.n_dst * 48
        if rh_v is not None:
            by += nlev * (npts * 8 + rh_v.n_dst * es) + rh_v.n_dst * 48
        ACCOUNT.append(("wind_destagger L%d" % nlev, by + (npts * 16 if rot else 0)))

    def p(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None
    check(L.load().mpg_wind_destagger_pitched_dev(rh_u._h if rh_u is not None else None, rh_v._h if rh_v is not None else None, p(cosa), p(sina),
                                                  p(umass), p(vmass), C.c_int(nlev), p(u), p(v),
                                                  C.c_int(int(out_dtype == torch.float32) | (2 if dst_be else 0)), p(ur), p(vr), C.c_int64(ld),
                                                  _stream_ptr()))
    return u, v, ur, vr


def rotate_winds_cgrid_transpose(cosa, sina, gu, gv):
    """mpg_rotate_winds_transpose_dev: the adjoint of rotate_winds_cgrid, in place on the gradients gu, gv -- contiguous float64 CUDA
    tensors [nlev][ny][nx] (or [ny][nx]); cosa / sina [ny][nx] float64 CUDA tensors, reused over the levels.  The same bits as
    target_grid.rotate_winds_transpose_at.  Returns (gu, gv)."""
    import torch
    for t in (cosa, sina, gu, gv):
        if not (_is_torch(t) and t.is_cuda and t.is_contiguous() and t.dtype == torch.float64):
            raise ValueError("rotate_winds_cgrid_transpose needs contiguous float64 CUDA tensors (the gradients are rotated in place)")
    npts = cosa.numel()
    if sina.numel() != npts or npts == 0 or gu.numel() % npts or gu.numel() == 0 or gv.numel() != gu.numel():
        raise ValueError("rotate_winds_cgrid_transpose: gu and gv must hold the same whole number of [ny][nx] planes as cosa / sina have points")
    nlev = gu.numel() // npts
    check(L.rotate_winds_transpose_dev(C.c_int64(npts), C.c_int(nlev), C.c_void_p(cosa.data_ptr()), C.c_void_p(sina.data_ptr()),
                                       C.c_void_p(gu.data_ptr()), C.c_void_p(gv.data_ptr()), _stream_ptr()))
    return gu, gv


def wind_destagger_transpose(rh_u, rh_v, cosa, sina, gu, gv, nlev, g_umass_rot=None, g_vmass_rot=None, outs=None):
    """mpg_wind_destagger_transpose_dev: the adjoint of wind_destagger in one pass -- the gradients gu [nlev][ny][nx+1] and gv
    [nlev][ny+1][nx] of U and V (float32 or float64 CUDA tensors of ONE dtype, dense or plane-pitched with one level stride for both, as
    wind_destagger's outs) back to the gradients (g_umass, g_vmass) of the mass-point winds, float64 [nlev][ny][nx]; an entry is None
    for a component that is not produced (its handle is None).  cosa / sina None: no rotation, and either handle may be None.
    g_umass_rot / g_vmass_rot: the gradients of wind_destagger's keep_mass results (float64, rotation only), added before the rotation's
    adjoint.  Bit-identical to rh_u.regrid_transpose(gu) and rh_v.regrid_transpose(gv) into float64, the adds, and
    rotate_winds_cgrid_transpose.  outs=(g_umass, g_vmass): contiguous float64 CUDA tensors to write into."""
    import torch
    if (cosa is None) != (sina is None):
        raise ValueError("wind_destagger_transpose: cosa and sina come together")
    if rh_u is None and rh_v is None:
        raise ValueError("wind_destagger_transpose: no handle")
    rot = cosa is not None
    nx, ny = (rh_v.nx_dst, rh_v.ny_dst - 1) if rh_v is not None else (rh_u.nx_dst - 1, rh_u.ny_dst)
    pitched, dense, dts = set(), [], set()
    for t, rh in ((gu, rh_u), (gv, rh_v)):
        if rh is None:
            continue
        if not (_is_torch(t) and t.is_cuda and t.dtype in (torch.float32, torch.float64)):
            raise ValueError("wind_destagger_transpose needs float32/float64 CUDA tensors")
        dts.add(t.dtype)
        if t.is_contiguous():
            if t.numel() != nlev * rh.n_dst:
                raise ValueError("wind_destagger_transpose: a gradient has %d elements, its handle expects %d" % (t.numel(), nlev * rh.n_dst))
            dense.append(rh.n_dst)
        else:
            if t.dim() != 3:
                raise ValueError("wind_destagger_transpose: a strided gradient must be (nlev, ny, nx) with plane-pitched levels")
            pitched.add(_level_stride(t, (nlev,), rh.ny_dst, rh.nx_dst, "wind_destagger_transpose"))
    if len(dts) > 1:
        raise ValueError("wind_destagger_transpose: gu and gv must have one dtype")
    # one stride for both: a contiguous tensor beside a pitched one has the stride of its own plane
    if len(pitched) > 1 or (pitched and nlev > 1 and any(n != max(pitched) for n in dense)):
        raise ValueError("wind_destagger_transpose: gu and gv must share one level stride (or both be dense)")
    ld = pitched.pop() if pitched else 0
    for t in (cosa, sina, g_umass_rot, g_vmass_rot):
        if t is None:
            continue
        if not (_is_torch(t) and t.is_cuda and t.is_contiguous() and t.dtype == torch.float64):
            raise ValueError("wind_destagger_transpose: the angles and the mass-wind gradients must be contiguous float64 CUDA tensors")
    if rot and (cosa.numel() != nx * ny or sina.numel() != nx * ny):
        raise ValueError("wind_destagger_transpose: cosa / sina must have %d points" % (nx * ny))
    for t in (g_umass_rot, g_vmass_rot):
        if t is not None and t.numel() != nlev * nx * ny:
            raise ValueError("wind_destagger_transpose: a mass-wind gradient must have %d elements" % (nlev * nx * ny))
    ref = gu if rh_u is not None else gv
    og, ov = outs if outs is not None else (None, None)
    if og is None and rh_u is not None:
        og = torch.empty((nlev, ny, nx), dtype=torch.float64, device=ref.device)
    if ov is None and rh_v is not None:
        ov = torch.empty((nlev, ny, nx), dtype=torch.float64, device=ref.device)
    for t, rh in ((og, rh_u), (ov, rh_v)):
        if rh is not None and not (_is_torch(t) and t.is_cuda and t.is_contiguous() and t.dtype == torch.float64 and t.numel() == nlev * nx * ny):
            raise ValueError("wind_destagger_transpose: outs must be contiguous float64 CUDA tensors of %d elements" % (nlev * nx * ny))

    def p(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None
    check(L.wind_destagger_transpose_dev(rh_u._h if rh_u is not None else None, rh_v._h if rh_v is not None else None, p(cosa), p(sina),
                                         p(gu) if rh_u is not None else None, p(gv) if rh_v is not None else None,
                                         C.c_int(int(dts.pop() == torch.float32)), C.c_int64(ld), C.c_int(nlev), p(g_umass_rot), p(g_vmass_rot),
                                         p(og) if rh_u is not None else None, p(ov) if rh_v is not None else None, _stream_ptr()))
    return (og if rh_u is not None else None), (ov if rh_v is not None else None)


if _torch is not None:
    class WindDestaggerFunction(_torch.autograd.Function):
        """wind_destagger with a gradient: forward is wind_destagger, backward ONE wind_destagger_transpose call.  Returns the tensors
        among (U, V, UMASS', VMASS') only; use wind_destagger_autograd()."""

        @staticmethod
        def forward(ctx, umass, vmass, rh_u, rh_v, cosa, sina, nlev, out_dtype, keep_mass):
            ctx.rh_u, ctx.rh_v, ctx.cosa, ctx.sina, ctx.nlev = rh_u, rh_v, cosa, sina, nlev
            ctx.given = (umass is not None, vmass is not None)
            res = wind_destagger(rh_u, rh_v, cosa, sina, umass, vmass, nlev, out_dtype=out_dtype, keep_mass=keep_mass)
            ctx.which = tuple(i for i, r in enumerate(res) if r is not None)
            return tuple(res[i] for i in ctx.which)

        @staticmethod
        def backward(ctx, *grads):
            g = dict(zip(ctx.which, grads))

            def c(t):
                return t.contiguous() if t is not None else None
            gum, gvm = wind_destagger_transpose(ctx.rh_u, ctx.rh_v, ctx.cosa, ctx.sina, c(g.get(0)), c(g.get(1)), ctx.nlev,
                                                g_umass_rot=c(g.get(2)), g_vmass_rot=c(g.get(3)))
            return (gum if ctx.given[0] else None, gvm if ctx.given[1] else None) + (None,) * 7


def wind_destagger_autograd(rh_u, rh_v, cosa, sina, umass, vmass, nlev, out_dtype=None, keep_mass=False):
    """wind_destagger(rh_u, rh_v, cosa, sina, umass, vmass, nlev, out_dtype=out_dtype, keep_mass=keep_mass) on float64 CUDA tensors as a
    differentiable torch op: the same bits and the same 4-tuple (U, V, UMASS', VMASS').  The backward is one wind_destagger_transpose
    call on the incoming gradients (float32 or float64, as out_dtype) -- with keep_mass the gradients of the rotated mass winds go in as
    g_umass_rot / g_vmass_rot -- and the gradients with respect to umass and vmass are always float64; None for an input that was not
    given.  The angles are constants."""
    res = WindDestaggerFunction.apply(umass, vmass, rh_u, rh_v, cosa, sina, nlev, out_dtype, keep_mass)
    out = [None, None, None, None]
    slots = [i for i, have in enumerate((rh_u is not None, rh_v is not None, keep_mass and cosa is not None, keep_mass and cosa is not None)) if have]
    for i, r in zip(slots, res):
        out[i] = r
    return tuple(out)


def _wind_source(t, rh, nlev, who):
    """The level stride (elements, 0 = dense) of one wind component for wind_to_mesh, after the checks RouteHandle._to_mesh makes of its source."""
    import torch
    if not (_is_torch(t) and t.is_cuda and t.dtype in (torch.float32, torch.float64)):
        raise ValueError(who + " needs float32/float64 CUDA tensors")
    if t.is_contiguous():
        if t.numel() != nlev * rh.n_src:
            raise ValueError("%s: a source has %d elements, its handle expects %d" % (who, t.numel(), nlev * rh.n_src))
        return 0
    if t.dim() not in (3, 4) or (t.dim() == 4 and t.shape[0] != 1):
        raise ValueError(who + ": a strided source must be (nlev, ny, nx) or (1, nlev, ny, nx) with plane-pitched levels")
    ny, nx = int(t.shape[-2]), int(t.shape[-1])
    if ny * nx != rh.n_src:
        raise ValueError("%s: source planes have %d points, the handle expects %d" % (who, ny * nx, rh.n_src))
    return _level_stride(t, (1, nlev) if t.dim() == 4 else (nlev,), ny, nx, who)


def _wind_pair(who, call, rh_u, rh_v, angles, names, need_angles, u, v, nlev, layout, out_dtype, outs, nout, label=""):
    """The body of wind_to_mesh and wind_to_edges: the checks of the sources, the two angle arrays `names` (need_angles False: both may be
    None) and the nout results (outs: a sequence of nout tensors or None each), the allocation, the ACCOUNT entry and the call.  Returns
    the tuple of results."""
    import torch
    ldu, ldv = _wind_source(u, rh_u, nlev, who), _wind_source(v, rh_v, nlev, who)
    if u.dtype != v.dtype:
        raise ValueError(who + ": u and v must have one dtype")
    if not need_angles and (angles[0] is None) != (angles[1] is None):
        raise ValueError("%s: %s come together (both None: no rotation)" % (who, names.replace(" / ", " and ")))
    for t in angles:
        if (need_angles or t is not None) and not (t is not None and _is_torch(t) and t.is_cuda and t.is_contiguous() and t.dtype == torch.float64
                                                   and t.numel() == rh_u.n_dst):
            raise ValueError("%s: %s must be contiguous float64 CUDA tensors of n_dst = %d elements" % (who, names, rh_u.n_dst))
    outs = tuple(outs) if outs is not None else (None,) * nout
    if len(outs) != nout:
        raise ValueError(who + ": outs must hold %d tensor(s)" % nout)
    given = [t for t in outs if t is not None]
    out_dtype = out_dtype or (given[0].dtype if given else u.dtype)
    if isinstance(out_dtype, np.dtype) or out_dtype in (np.float32, np.float64):
        out_dtype = torch.float32 if np.dtype(out_dtype) == np.float32 else torch.float64
    shape = (nlev, rh_u.n_dst) if layout == LAYOUT_CELL_FAST else (rh_u.n_dst, nlev)
    res = [t if t is not None else torch.empty(shape, dtype=out_dtype, device=u.device) for t in outs]
    for t in res:
        if not (t.is_cuda and t.is_contiguous() and t.dtype == out_dtype and t.dtype in (torch.float32, torch.float64) and t.numel() == nlev * rh_u.n_dst):
            raise ValueError(who + ": outs must be contiguous float32/float64 CUDA tensors of %d elements and one dtype" % (nlev * rh_u.n_dst))
    if ACCOUNT is not None:     # L (U_u + U_v) e_s + n_out P L e_d + P (2 NNZ 12 + 16): both sources read once, every result written once,
        for rh in (rh_u, rh_v):  # the indices and weights of both handles and the angles (when given) once
            if getattr(rh, "_acc_U", None) is None:
                rh._acc_U = int(rh.unique_sources().size)
        if rh_u.nnz_per_row == 0:   # CSR handles: 12 nnz + 4 (P + 1) per DISTINCT handle (one handle given twice is staged once)
            wbytes = sum(12 * rh.nnz + 4 * (rh.n_dst + 1) for rh in ((rh_u,) if rh_v is rh_u else (rh_u, rh_v)))
        else:
            wbytes = rh_u.n_dst * 2 * rh_u.nnz_per_row * 12
        ACCOUNT.append(("%s nnz%d L%d%s" % (who, rh_u.nnz_per_row, nlev, label),
                        nlev * (rh_u._acc_U + rh_v._acc_U) * u.element_size() + nout * rh_u.n_dst * nlev * res[0].element_size()
                        + wbytes + rh_u.n_dst * (16 if angles[0] is not None else 0)))

    def p(t):
        return t.data_ptr() if t is not None else None
    check(call(rh_u._h, rh_v._h, p(angles[0]), p(angles[1]), u.data_ptr(), v.data_ptr(), int(u.dtype == torch.float32), ldu, ldv, int(nlev),
               res[0].data_ptr(), p(res[1] if nout == 2 else None), int(out_dtype == torch.float32), int(layout),
               torch.cuda.current_stream().cuda_stream))
    return tuple(res)


def wind_to_mesh(rh_u, rh_v, cosa, sina, u, v, nlev, layout=LAYOUT_CELL_FAST, out_dtype=None, outs=None):
    """mpg_wind_to_mesh_dev: the wind chain turned round, in one pass -- U through rh_u and V through rh_v onto the SAME mesh points (the
    typical pair: regrid_store_to_mesh(grid, mesh, staggerloc=STAGGERLOC_EDGE1 / STAGGERLOC_EDGE2); rh_u is rh_v is allowed), then the
    rotation from grid-relative to earth-relative winds with cosa / sina at the mesh points (mesh_rotang; both None: no rotation) and the
    cast: ue = a ca - b sa, ve = a sa + b ca with a, b the float64 results of rh_u.regrid_to_mesh(u) and rh_v.regrid_to_mesh(v), the
    inverse of rotate_winds_cgrid.  u, v: float32 / float64 CUDA tensors of one dtype, [nlev][n_src of their handle], contiguous or
    plane-pitched views (nlev, ny, nx) as empty_pitched and wind_destagger(outs=) make.  Returns (ue, ve) of out_dtype (default: u's):
    (nlev, n_dst) for LAYOUT_CELL_FAST, (n_dst, nlev) for LAYOUT_LEV_FAST -- MPAS file order; a point either handle leaves unmapped is
    +0.0 in both.  outs=(ue, ve): contiguous CUDA tensors of nlev * n_dst elements to write into.  Bit-identical to the separate calls."""
    return _wind_pair("wind_to_mesh", L.wind_to_mesh_dev, rh_u, rh_v, (cosa, sina), "cosa / sina", False, u, v, nlev, layout, out_dtype, outs, 2)


def mesh_rotang(grid, mesh, meshloc=MESHLOC_ELEMENT):
    """mpg_mesh_rotang_dev: (cosa, sina) of a Lambert grid's rotation angle at the mesh's cells (MESHLOC_ELEMENT) or vertices
    (MESHLOC_NODE), float64 CUDA tensors for wind_to_mesh; target_grid.rotang_at is the numpy mirror.  MpgError (rc 4) for a grid that
    is not Lambert or carries no projection -- the forward chain does not rotate there: pass None angles -- and for a windowed mesh."""
    import torch
    if meshloc not in (MESHLOC_ELEMENT, MESHLOC_NODE):
        raise ValueError("mesh_rotang: meshloc must be MESHLOC_ELEMENT or MESHLOC_NODE")
    n = mesh.nCells if meshloc == MESHLOC_ELEMENT else mesh.nVertices
    cosa = torch.empty(n, dtype=torch.float64, device="cuda")
    sina = torch.empty(n, dtype=torch.float64, device="cuda")
    check(L.mesh_rotang_dev(grid._h, mesh._h, int(meshloc), cosa.data_ptr(), sina.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return cosa, sina


def _unmapped_mask(rh):
    """The points a handle leaves unmapped -- a fixed one: idx[0] < 0; a CSR one: the row is empty -- as a bool CUDA tensor [n_dst],
    downloaded once per handle object."""
    if getattr(rh, "_unmapped_dev", None) is None:
        un = np.diff(rh.csr()[0]) == 0 if rh.nnz_per_row == 0 else rh.weights()[0][:, 0] < 0
        rh._unmapped_dev = _torch.as_tensor(un, device="cuda")
    return rh._unmapped_dev


def _wind_pair_backward(ctx, grads, turn):
    """The backward both wind ops share: the incoming gradients back to [lev][point] planes, zeroed where either handle leaves the point
    unmapped, turned by the op's transposed rotation `turn` into (g_a, g_b), and each handle's regrid_transpose in its input's shape."""
    n, nlev = ctx.rh_u.n_dst, ctx.nlev

    def planes(g):            # regrid_transpose reads [nlev][n_dst] planes
        if ctx.layout == LAYOUT_LEV_FAST:
            g = g.reshape(n, nlev).t()
        return g.reshape(nlev, n)
    # a point unmapped in EITHER handle is a constant of the forward: without this a point mapped in one handle only would send
    # its gradient through that handle's transpose, a term the forward does not have
    un = _unmapped_mask(ctx.rh_u)
    if ctx.rh_v is not ctx.rh_u:
        un = un | _unmapped_mask(ctx.rh_v)
    g_a, g_b = turn(*[planes(g).masked_fill(un, 0.0) for g in grads])
    # two separate gradients even when rh_u is rh_v: one of u, one of v
    gu = ctx.rh_u.regrid_transpose(g_a.contiguous(), nlev=nlev, layout=LAYOUT_CELL_FAST, out_dtype=ctx.dtypes[0])
    gv = ctx.rh_v.regrid_transpose(g_b.contiguous(), nlev=nlev, layout=LAYOUT_CELL_FAST, out_dtype=ctx.dtypes[1])
    return gu.reshape(ctx.shapes[0]), gv.reshape(ctx.shapes[1])


if _torch is not None:
    class WindToMeshFunction(_torch.autograd.Function):
        """wind_to_mesh with a gradient: forward is wind_to_mesh in u's dtype; backward takes (g_ue, g_ve) back to [lev][cell], zeroes
        them where either handle leaves the point unmapped (the forward stores a constant +0.0 in both results there), turns them by the
        transposed rotation in torch and applies each handle's regrid_transpose.  Use wind_to_mesh_autograd()."""

        @staticmethod
        def forward(ctx, u, v, rh_u, rh_v, cosa, sina, nlev, layout):
            ctx.rh_u, ctx.rh_v, ctx.cosa, ctx.sina, ctx.nlev, ctx.layout = rh_u, rh_v, cosa, sina, nlev, layout
            ctx.shapes, ctx.dtypes = (u.shape, v.shape), (u.dtype, v.dtype)
            return wind_to_mesh(rh_u, rh_v, cosa, sina, u.contiguous(), v.contiguous(), nlev, layout=layout, out_dtype=u.dtype)

        @staticmethod
        def backward(ctx, g_ue, g_ve):
            def turn(g_ue, g_ve):
                if ctx.cosa is None:
                    return g_ue, g_ve
                ca, sa = ctx.cosa.to(g_ue.dtype), ctx.sina.to(g_ue.dtype)
                return g_ue * ca + g_ve * sa, g_ve * ca - g_ue * sa
            return _wind_pair_backward(ctx, (g_ue, g_ve), turn) + (None,) * 6


def wind_to_mesh_autograd(rh_u, rh_v, cosa, sina, u, v, nlev, layout=LAYOUT_CELL_FAST):
    """wind_to_mesh(rh_u, rh_v, cosa, sina, u, v, nlev, layout) in u's dtype as a differentiable torch op.  The gradients with respect
    to u and v: the incoming (g_ue, g_ve), taken back to [lev][cell] and set to zero where either handle leaves the point unmapped (the
    forward's +0.0 there depends on neither u nor v), give g_a = g_ue ca + g_ve sa and g_b = -g_ue sa + g_ve ca, and
    rh_u.regrid_transpose(g_a), rh_v.regrid_transpose(g_b) are returned in u's and v's shapes and dtypes: the exact adjoint of the
    forward.  The first backward on a handle downloads its indices once for the mask."""
    return WindToMeshFunction.apply(u, v, rh_u, rh_v, cosa, sina, nlev, layout)


def mesh_edge_rotang(grid, mesh):
    """mpg_mesh_edge_rotang_dev: (cn, sn) = cos / sin of phi = angleEdge - alpha at the mesh's edges, float64 CUDA tensors [nEdges] for
    wind_to_edges -- the rotation from a Lambert grid's grid-relative winds to earth-relative ones (alpha, as mesh_rotang) and the
    projection onto the edge normal (angleEdge) composed into one rotation; target_grid.edge_rotang_at is the numpy mirror.  grid=None:
    alpha = 0, winds that are earth-relative already (a lat-lon or Mercator source).  MpgError (rc 4) for a grid that is not Lambert or
    carries no projection -- pass None there -- and (rc 2) for a mesh without edges or without angleEdge (Mesh.set_edges)."""
    import torch
    n = int(mesh.nEdges)          # (0: the library refuses a mesh without edges before it looks at the outputs)
    cn = torch.empty(n, dtype=torch.float64, device="cuda")
    sn = torch.empty(n, dtype=torch.float64, device="cuda")
    check(L.mesh_edge_rotang_dev(grid._h if grid is not None else None, mesh._h, cn.data_ptr(), sn.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream))
    return cn, sn


def wind_to_edges(rh_u, rh_v, cn, sn, u, v, nlev, layout=LAYOUT_CELL_FAST, out_dtype=None, tangential=False, outs=None):
    """mpg_wind_to_edges_dev: winds onto mesh EDGES in one pass -- U through rh_u and V through rh_v onto the SAME points (the typical
    pair: regrid_store_to_mesh(grid, mesh, staggerloc=STAGGERLOC_EDGE1 / STAGGERLOC_EDGE2, meshloc=MESHLOC_EDGE); rh_u is rh_v is
    allowed), then ONE rotation by phi = angleEdge - alpha with cn / sn = cos / sin(phi) at the points (mesh_edge_rotang; required) and
    the cast: un = a cn + b sn, the edge-normal wind `u` MPAS carries, and with tangential=True ut = b cn - a sn, with a, b the float64
    results of rh_u.regrid_to_mesh(u) and rh_v.regrid_to_mesh(v).  u, v: float32 / float64 CUDA tensors of one dtype,
    [nlev][n_src of their handle], contiguous or plane-pitched views (nlev, ny, nx).  Returns un, or (un, ut), of out_dtype (default:
    u's): (nlev, n_dst) for LAYOUT_CELL_FAST, (n_dst, nlev) for LAYOUT_LEV_FAST -- the file order of u(nEdges, nVertLevels); a point
    either handle leaves unmapped is +0.0.  outs: the tensor (tangential: the pair) to write into, contiguous, nlev * n_dst elements.
    Bit-identical to the separate calls."""
    nout = 2 if tangential else 1
    if _is_torch(outs):
        outs = (outs,)
    res = _wind_pair("wind_to_edges", L.wind_to_edges_dev, rh_u, rh_v, (cn, sn), "cn / sn", True, u, v, nlev, layout, out_dtype, outs, nout,
                     label=" x%d" % nout)
    return res if tangential else res[0]


if _torch is not None:
    class WindToEdgesFunction(_torch.autograd.Function):
        """wind_to_edges with a gradient: forward is wind_to_edges in u's dtype; backward takes g_un (and g_ut) back to [lev][edge],
        zeroes them where either handle leaves the point unmapped (the forward stores a constant +0.0 there), turns them by the
        transposed rotation in torch and applies each handle's regrid_transpose.  Use wind_to_edges_autograd()."""

        @staticmethod
        def forward(ctx, u, v, rh_u, rh_v, cn, sn, nlev, layout, tangential):
            ctx.rh_u, ctx.rh_v, ctx.cn, ctx.sn, ctx.nlev, ctx.layout, ctx.tangential = rh_u, rh_v, cn, sn, nlev, layout, tangential
            ctx.shapes, ctx.dtypes = (u.shape, v.shape), (u.dtype, v.dtype)
            return wind_to_edges(rh_u, rh_v, cn, sn, u.contiguous(), v.contiguous(), nlev, layout=layout, out_dtype=u.dtype, tangential=tangential)

        @staticmethod
        def backward(ctx, g_un, g_ut=None):
            def turn(g_un, g_ut=None):
                cn, sn = ctx.cn.to(g_un.dtype), ctx.sn.to(g_un.dtype)
                if g_ut is None:
                    return g_un * cn, g_un * sn
                return g_un * cn - g_ut * sn, g_un * sn + g_ut * cn
            return _wind_pair_backward(ctx, (g_un, g_ut) if ctx.tangential else (g_un,), turn) + (None,) * 7


def wind_to_edges_autograd(rh_u, rh_v, cn, sn, u, v, nlev, layout=LAYOUT_CELL_FAST, tangential=False):
    """wind_to_edges(rh_u, rh_v, cn, sn, u, v, nlev, layout, tangential=tangential) in u's dtype as a differentiable torch op.  The
    gradients with respect to u and v: the incoming g_un (and g_ut), taken back to [lev][edge] and set to zero where either handle
    leaves the point unmapped, give g_a = g_un cn - g_ut sn and g_b = g_un sn + g_ut cn, and rh_u.regrid_transpose(g_a),
    rh_v.regrid_transpose(g_b) are returned in u's and v's shapes and dtypes: the exact adjoint of the forward.  The first backward on a
    handle downloads its indices once for the mask."""
    return WindToEdgesFunction.apply(u, v, rh_u, rh_v, cn, sn, nlev, layout, tangential)


def wind_csr_to_mesh(rh_u, rh_v, cosa, sina, u, v, nlev, layout=LAYOUT_CELL_FAST, out_dtype=None, outs=None):
    """mpg_wind_csr_to_mesh_dev: wind_to_mesh for CSR handles -- regrid_store_periodic_to_mesh (U and V of a global lat-lon or Gaussian
    analysis), regrid_store_conserve_to_mesh, regrid_store_conserve_mesh, RouteHandle.from_weights -- in one pass: ue = a ca - b sa,
    ve = a sa + b ca with a, b the float64 results of rh_u.regrid_csr_to_mesh(u) and rh_v.regrid_csr_to_mesh(v); cosa / sina both None:
    no rotation (ue = a, ve = b).  rh_u is rh_v is the main case (a collocated analysis): the handle is staged once.  The arguments and
    results are wind_to_mesh's; a point whose row is empty in either handle is +0.0 in both results.  Bit-identical to the separate
    calls.  Under POLEMETHOD_ALLAVG a cap point gets the row mean of each COMPONENT, which is not a wind (include/mpassit_amd.h)."""
    return _wind_pair("wind_csr_to_mesh", L.wind_csr_to_mesh_dev, rh_u, rh_v, (cosa, sina), "cosa / sina", False, u, v, nlev, layout, out_dtype, outs, 2)


def wind_csr_to_edges(rh_u, rh_v, cn, sn, u, v, nlev, layout=LAYOUT_CELL_FAST, out_dtype=None, tangential=False, outs=None):
    """mpg_wind_csr_to_edges_dev: wind_to_edges for CSR handles onto the mesh's edges (the typical one:
    regrid_store_periodic_to_mesh(grid, mesh, meshloc=MESHLOC_EDGE), given as rh_u and rh_v), in one pass: un = a cn + b sn, the
    edge-normal wind `u` MPAS carries, and with tangential=True ut = b cn - a sn, with a, b the float64 results of
    rh_u.regrid_csr_to_mesh(u) and rh_v.regrid_csr_to_mesh(v) and cn / sn of mesh_edge_rotang (grid=None for the earth-relative winds of
    a lat-lon analysis; required).  The arguments and results are wind_to_edges'; a point whose row is empty in either handle is +0.0.
    Bit-identical to the separate calls.  The cap caveat of wind_csr_to_mesh holds here too."""
    nout = 2 if tangential else 1
    if _is_torch(outs):
        outs = (outs,)
    res = _wind_pair("wind_csr_to_edges", L.wind_csr_to_edges_dev, rh_u, rh_v, (cn, sn), "cn / sn", True, u, v, nlev, layout, out_dtype, outs, nout,
                     label=" x%d" % nout)
    return res if tangential else res[0]


if _torch is not None:
    class WindCsrToMeshFunction(WindToMeshFunction):
        """wind_csr_to_mesh with a gradient: WindToMeshFunction's backward (the mask of a CSR handle is "row empty") behind the CSR
        forward.  Use wind_csr_to_mesh_autograd()."""

        @staticmethod
        def forward(ctx, u, v, rh_u, rh_v, cosa, sina, nlev, layout):
            ctx.rh_u, ctx.rh_v, ctx.cosa, ctx.sina, ctx.nlev, ctx.layout = rh_u, rh_v, cosa, sina, nlev, layout
            ctx.shapes, ctx.dtypes = (u.shape, v.shape), (u.dtype, v.dtype)
            return wind_csr_to_mesh(rh_u, rh_v, cosa, sina, u.contiguous(), v.contiguous(), nlev, layout=layout, out_dtype=u.dtype)

    class WindCsrToEdgesFunction(WindToEdgesFunction):
        """wind_csr_to_edges with a gradient: WindToEdgesFunction's backward behind the CSR forward.  Use wind_csr_to_edges_autograd()."""

        @staticmethod
        def forward(ctx, u, v, rh_u, rh_v, cn, sn, nlev, layout, tangential):
            ctx.rh_u, ctx.rh_v, ctx.cn, ctx.sn, ctx.nlev, ctx.layout, ctx.tangential = rh_u, rh_v, cn, sn, nlev, layout, tangential
            ctx.shapes, ctx.dtypes = (u.shape, v.shape), (u.dtype, v.dtype)
            return wind_csr_to_edges(rh_u, rh_v, cn, sn, u.contiguous(), v.contiguous(), nlev, layout=layout, out_dtype=u.dtype, tangential=tangential)


def wind_csr_to_mesh_autograd(rh_u, rh_v, cosa, sina, u, v, nlev, layout=LAYOUT_CELL_FAST):
    """wind_csr_to_mesh(rh_u, rh_v, cosa, sina, u, v, nlev, layout) in u's dtype as a differentiable torch op: the gradients of
    wind_to_mesh_autograd, with "unmapped" read as "the row is empty" (the first backward on a handle downloads its row pointers once)
    and each handle's regrid_transpose, which serves CSR handles."""
    return WindCsrToMeshFunction.apply(u, v, rh_u, rh_v, cosa, sina, nlev, layout)


def wind_csr_to_edges_autograd(rh_u, rh_v, cn, sn, u, v, nlev, layout=LAYOUT_CELL_FAST, tangential=False):
    """wind_csr_to_edges(rh_u, rh_v, cn, sn, u, v, nlev, layout, tangential=tangential) in u's dtype as a differentiable torch op: the
    gradients of wind_to_edges_autograd, with "unmapped" read as "the row is empty" and each handle's regrid_transpose."""
    return WindCsrToEdgesFunction.apply(u, v, rh_u, rh_v, cn, sn, nlev, layout, tangential)


# ---- a wind as a vector through one CSR handle (ESMF 8.6's vectorRegrid) --------------------------------------------------------------
def sphere_frames(lon, lat, c=None, s=None):
    """mpg_sphere_frames_dev: the local frames of n points (lon, lat: float64 CUDA tensors or numpy arrays, RADIANS) as a [6][n] float64
    CUDA tensor, the planes D0x D0y D0z D1x D1y D1z.  c, s both None: D0 = east, D1 = north (earth-relative winds); else D0 = c east +
    s north, D1 = c north - s east: mesh_rotang's (cosa, sina) for the grid-relative winds of a Lambert grid, cos / sin of angleEdge for
    (normal, tangent) at mesh edges, mesh_edge_rotang's (cn, sn) for both at once.  target_grid.sphere_frames_at is the numpy mirror."""
    import torch
    if (c is None) != (s is None):
        raise ValueError("sphere_frames: c and s come together (both None: east and north)")

    def dev(x):
        return x if x is None or _is_torch(x) else torch.as_tensor(_f64(x).reshape(-1), device="cuda")
    lon, lat, c, s = (dev(x) for x in (lon, lat, c, s))
    n = lon.numel()
    for t in (lon, lat, c, s):
        if t is not None and not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float64 and t.numel() == n):
            raise ValueError("sphere_frames: lon, lat, c and s must be contiguous float64 CUDA tensors (or numpy arrays) of one length")
    frames = torch.empty((6, n), dtype=torch.float64, device="cuda")
    check(L.sphere_frames_dev(n, lon.data_ptr(), lat.data_ptr(), c.data_ptr() if c is not None else None, s.data_ptr() if s is not None else None,
                              frames.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return frames


def _frames_ok(t, n):
    import torch
    return _is_torch(t) and t.is_cuda and t.is_contiguous() and t.dtype == torch.float64 and t.numel() == 6 * n


def wind_vector_weights(rh, src_frames, dst_frames):
    """mpg_wind_vector_weights_dev: the 2 x 2 blocks of (rh, frames) as a [4][nnz] float64 CUDA tensor, the planes m00 m01 m10 m11 in the
    order of rh.csr()'s entries -- computed once, applied by wind_vector to any number of levels and fields.  rh: a CSR handle without
    pole terms; src_frames [6][n_src], dst_frames [6][n_dst] as sphere_frames makes.  The bits of target_grid.wind_vector_blocks."""
    import torch
    if not (_frames_ok(src_frames, rh.n_src) and _frames_ok(dst_frames, rh.n_dst)):
        raise ValueError("wind_vector_weights: the frames must be contiguous float64 CUDA tensors [6][n_src = %d] and [6][n_dst = %d]"
                         % (rh.n_src, rh.n_dst))
    m = torch.empty((4, rh.nnz), dtype=torch.float64, device="cuda")
    check(L.wind_vector_weights_dev(rh._h, src_frames.data_ptr(), dst_frames.data_ptr(), m.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return m


def wind_vector(rh, m, u, v, nlev, layout=LAYOUT_CELL_FAST, out_dtype=None, second=True, outs=None):
    """mpg_wind_vector_dev: (u, v) through the CSR handle rh as a VECTOR, in one pass -- per point r0 = sum_q m00 u[col] + m01 v[col],
    r1 = sum_q m10 u[col] + m11 v[col] with the blocks m of wind_vector_weights(rh, src_frames, dst_frames): with (east, north) frames on
    both sides (r0, r1) = (ue, ve); with (normal, tangent) frames at mesh edges (un, ut).  Under POLEMETHOD_ALLAVG a cap point gets the
    mean of the row's vectors, which is a wind (wind_csr_to_mesh gives the mean of each component there, which is not).  u, v: float32 /
    float64 CUDA tensors of one dtype, [nlev][n_src], contiguous or plane-pitched views (nlev, ny, nx).  Returns (r0, r1), or r0 alone
    with second=False (only m00, m01 are read), of out_dtype (default: u's): (nlev, n_dst) for LAYOUT_CELL_FAST, (n_dst, nlev) for
    LAYOUT_LEV_FAST; an empty row is +0.0.  outs: the pair (second=False: the tensor) to write into, contiguous, nlev * n_dst elements.
    Bit-identical to four regrid_csr_to_mesh calls of from-weights handles with the values m[k], added in float64 and cast once."""
    import torch
    who = "wind_vector"
    ldu, ldv = _wind_source(u, rh, nlev, who), _wind_source(v, rh, nlev, who)
    if u.dtype != v.dtype:
        raise ValueError(who + ": u and v must have one dtype")
    if not (_is_torch(m) and m.is_cuda and m.is_contiguous() and m.dtype == torch.float64 and m.numel() == 4 * rh.nnz):
        raise ValueError("%s: m must be a contiguous float64 CUDA tensor [4][nnz = %d] (wind_vector_weights)" % (who, rh.nnz))
    nout = 2 if second else 1
    if _is_torch(outs):
        outs = (outs,)
    outs = tuple(outs) if outs is not None else (None,) * nout
    if len(outs) != nout:
        raise ValueError(who + ": outs must hold %d tensor(s)" % nout)
    given = [t for t in outs if t is not None]
    out_dtype = out_dtype or (given[0].dtype if given else u.dtype)
    if isinstance(out_dtype, np.dtype) or out_dtype in (np.float32, np.float64):
        out_dtype = torch.float32 if np.dtype(out_dtype) == np.float32 else torch.float64
    shape = (nlev, rh.n_dst) if layout == LAYOUT_CELL_FAST else (rh.n_dst, nlev)
    res = [t if t is not None else torch.empty(shape, dtype=out_dtype, device=u.device) for t in outs]
    for t in res:
        if not (t.is_cuda and t.is_contiguous() and t.dtype == out_dtype and t.dtype in (torch.float32, torch.float64) and t.numel() == nlev * rh.n_dst):
            raise ValueError(who + ": outs must be contiguous float32/float64 CUDA tensors of %d elements and one dtype" % (nlev * rh.n_dst))
    if ACCOUNT is not None:     # 2 L U e_s + n_out P L e_d + (4 + 16 n_out) nnz + 4 (P + 1): both sources, every result, col and the blocks once
        if getattr(rh, "_acc_U", None) is None:
            rh._acc_U = int(rh.unique_sources().size)
        ACCOUNT.append(("%s L%d x%d" % (who, nlev, nout), 2 * nlev * rh._acc_U * u.element_size() + nout * rh.n_dst * nlev * res[0].element_size()
                        + (4 + 16 * nout) * rh.nnz + 4 * (rh.n_dst + 1)))
    check(L.wind_vector_dev(rh._h, m.data_ptr(), u.data_ptr(), v.data_ptr(), int(u.dtype == torch.float32), ldu, ldv, int(nlev), res[0].data_ptr(),
                            res[1].data_ptr() if second else None, int(out_dtype == torch.float32), int(layout),
                            torch.cuda.current_stream().cuda_stream))
    return tuple(res) if second else res[0]


class _VectorAdjoint:
    """The four from-weights handles A_kl of one (rh, m), values m[k] on rh's pattern: what wind_vector's backward applies the transposes
    of.  Built on the first backward, kept on the tensor m, rebuilt when m has been written since; releases its handles with itself."""

    def __init__(self, rh, m, nplanes):
        rowptr, col, _ = rh.csr()
        row = np.repeat(np.arange(1, rh.n_dst + 1, dtype=np.int32), np.diff(rowptr).astype(np.int64))
        mh = m.detach().cpu().numpy()
        self.key = (rh._h.value if hasattr(rh._h, "value") else rh._h, m.data_ptr(), m._version, nplanes)
        self.handles = [RouteHandle.from_weights(rh.n_src, rh.n_dst, 1, row, (col + 1).astype(np.int32), mh[k]) for k in range(nplanes)]

    def __del__(self):
        for h in self.handles:
            try:
                h.release()
            except Exception:     # the library may be gone at interpreter exit
                pass

    @classmethod
    def of(cls, rh, m, nplanes):
        held = getattr(m, "_mpg_vector_adjoint", None)
        key = (rh._h.value if hasattr(rh._h, "value") else rh._h, m.data_ptr(), m._version)
        if held is None or held.key[:3] != key or held.key[3] < nplanes:
            held = cls(rh, m, nplanes)
            m._mpg_vector_adjoint = held
        return held.handles


if _torch is not None:
    class WindVectorFunction(_torch.autograd.Function):
        """wind_vector with a gradient with respect to u and v (m is a constant): forward is wind_vector in u's dtype; backward takes the
        incoming gradients back to [lev][point] planes and applies regrid_transpose of the from-weights handles A_kl (values m[k]):
        gu = A00^T g0 + A10^T g1, gv = A01^T g0 + A11^T g1.  Use wind_vector_autograd()."""

        @staticmethod
        def forward(ctx, u, v, rh, m, nlev, layout, second):
            ctx.rh, ctx.m, ctx.nlev, ctx.layout, ctx.second = rh, m, nlev, layout, second
            ctx.shapes, ctx.dtypes = (u.shape, v.shape), (u.dtype, v.dtype)
            return wind_vector(rh, m, u.contiguous(), v.contiguous(), nlev, layout=layout, out_dtype=u.dtype, second=second)

        @staticmethod
        def backward(ctx, g0, g1=None):
            n, nlev = ctx.rh.n_dst, ctx.nlev
            A = _VectorAdjoint.of(ctx.rh, ctx.m, 4 if ctx.second else 2)
            grads = []
            for g in ((g0, g1) if ctx.second else (g0,)):     # regrid_transpose reads [nlev][n_dst] planes
                if ctx.layout == LAYOUT_LEV_FAST:
                    g = g.reshape(n, nlev).t()
                grads.append(g.reshape(nlev, n).contiguous())
            out = []
            for l in range(2):                                 # l = 0: u, 1: v
                g = A[l].regrid_transpose(grads[0], nlev=nlev, layout=LAYOUT_CELL_FAST, out_dtype=ctx.dtypes[l])
                if ctx.second:
                    g = g + A[2 + l].regrid_transpose(grads[1], nlev=nlev, layout=LAYOUT_CELL_FAST, out_dtype=ctx.dtypes[l])
                out.append(g.reshape(ctx.shapes[l]))
            return tuple(out) + (None,) * 5


def wind_vector_autograd(rh, m, u, v, nlev, layout=LAYOUT_CELL_FAST, second=True):
    """wind_vector(rh, m, u, v, nlev, layout, second=second) in u's dtype as a differentiable torch op.  The gradients with respect to u
    and v (m is a constant of the op): gu = A00^T g0 + A10^T g1 and gv = A01^T g0 + A11^T g1 with A_kl the handle's pattern with the values
    m[k], through regrid_transpose of four from-weights handles (two with second=False) that the first backward builds from a download
    of rh.csr() and m and that stay with m; returned in u's and v's shapes and dtypes: the exact adjoint of the forward."""
    return WindVectorFunction.apply(u, v, rh, m, nlev, layout, second)


# ---- winds from the edge-normal u a mesh carries (MPAS's mpas_reconstruct) -------------------------------------------------------------
def reconstruct_store(nEdgesOnCell, edgesOnCell, nEdges):
    """mpg_reconstruct_store: the pattern of edgesOnCell as a from-weights CSR RouteHandle, n_src = nEdges, n_dst = nCells.  nEdgesOnCell
    [nCells] and edgesOnCell [nCells][maxEdges] as an MPAS file holds them (1-based ids; slots past the count are not read): row c is the
    first nEdgesOnCell[c] slots of cell c in the file's order, which is the summation order; every value is 1.0.  Not cached: release()
    it.  Every CSR consumer takes the handle (csr(), regrid_csr_to_mesh, regrid_csr_rows, regrid_transpose)."""
    n_on = np.ascontiguousarray(nEdgesOnCell, np.int32).reshape(-1)
    eoc = np.ascontiguousarray(edgesOnCell, np.int32)
    if eoc.ndim != 2 or eoc.shape[0] != n_on.size:
        raise ValueError("reconstruct_store: edgesOnCell must be [nCells = %d][maxEdges]" % n_on.size)
    h = C.c_void_p()
    check(L.reconstruct_store(n_on.size, int(nEdges), int(eoc.shape[1]), _ptr(n_on), _ptr(eoc), C.byref(h)))
    return RouteHandle(h)


def reconstruct_weights(rh, coeffs, dst_frames=None):
    """mpg_reconstruct_weights_dev: the values of (rh, coeffs, frames) as a [nout][nnz] float64 CUDA tensor in the order of rh.csr()'s
    entries -- computed once, applied by wind_reconstruct to any number of levels and time levels.  coeffs: the file's coeffs_reconstruct
    [nCells][maxEdges][3] (a float64 CUDA tensor or a numpy array), padding included.  dst_frames [6][nCells] as sphere_frames makes:
    nout = 2, (lonCell, latCell) unturned for uReconstructZonal / uReconstructMeridional, turned by mesh_rotang's (cosa, sina) for
    grid-relative winds; None: nout = 3, uReconstructX / Y / Z.  The bits of target_grid.reconstruct_blocks."""
    import torch
    if not _is_torch(coeffs):
        coeffs = torch.as_tensor(_f64(coeffs), device="cuda")
    if not (coeffs.is_cuda and coeffs.is_contiguous() and coeffs.dtype == torch.float64 and coeffs.dim() == 3 and coeffs.shape[0] == rh.n_dst
            and coeffs.shape[2] == 3):
        raise ValueError("reconstruct_weights: coeffs must be a contiguous float64 [nCells = %d][maxEdges][3]" % rh.n_dst)
    if dst_frames is not None and not _frames_ok(dst_frames, rh.n_dst):
        raise ValueError("reconstruct_weights: dst_frames must be a contiguous float64 CUDA tensor [6][nCells = %d]" % rh.n_dst)
    m = torch.empty((2 if dst_frames is not None else 3, rh.nnz), dtype=torch.float64, device="cuda")
    check(L.reconstruct_weights_dev(rh._h, int(coeffs.shape[1]), coeffs.data_ptr(), dst_frames.data_ptr() if dst_frames is not None else None,
                                    m.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return m


def wind_reconstruct(rh, m, u, nlev, src_layout=LAYOUT_LEV_FAST, layout=LAYOUT_CELL_FAST, out_dtype=None, outs=None):
    """mpg_wind_reconstruct_dev: the winds at the cells from the edge-normal u, in one pass -- per cell and level r_k = sum_q m_k[q]
    u[col[q]] with the values m [nout][nnz] of reconstruct_weights (nout = 2: the frame's two components, 3: X, Y, Z).  u: a float32 /
    float64 CUDA tensor; src_layout LAYOUT_LEV_FAST: [nEdges][nlev], MPAS file order, contiguous; LAYOUT_CELL_FAST: [nlev][nEdges],
    contiguous or a plane-pitched view (nlev, ny, nx).  Returns nout tensors of out_dtype (default: u's): (nlev, nCells) for layout
    LAYOUT_CELL_FAST, (nCells, nlev) for LAYOUT_LEV_FAST; an empty row is +0.0.  outs: the nout tensors to write into, contiguous, nlev *
    nCells elements each.  Bit-identical to nout regrid_csr_to_mesh calls of from-weights handles with the values m[k]."""
    import torch
    who = "wind_reconstruct"
    if not (_is_torch(m) and m.is_cuda and m.is_contiguous() and m.dtype == torch.float64 and m.dim() == 2 and m.shape[1] == rh.nnz):
        raise ValueError("%s: m must be a contiguous float64 CUDA tensor [nout][nnz = %d] (reconstruct_weights)" % (who, rh.nnz))
    nout = int(m.shape[0])
    if src_layout == LAYOUT_LEV_FAST:
        if not (_is_torch(u) and u.is_cuda and u.dtype in (torch.float32, torch.float64) and u.is_contiguous() and u.numel() == nlev * rh.n_src):
            raise ValueError("%s: a LAYOUT_LEV_FAST source is a contiguous float32/float64 CUDA tensor [nEdges = %d][nlev = %d]" % (who, rh.n_src, nlev))
        ldu = 0
    else:
        ldu = _wind_source(u, rh, nlev, who)
    outs = tuple(outs) if outs is not None else (None,) * nout
    if len(outs) != nout:
        raise ValueError(who + ": outs must hold %d tensors" % nout)
    given = [t for t in outs if t is not None]
    out_dtype = out_dtype or (given[0].dtype if given else u.dtype)
    if isinstance(out_dtype, np.dtype) or out_dtype in (np.float32, np.float64):
        out_dtype = torch.float32 if np.dtype(out_dtype) == np.float32 else torch.float64
    shape = (nlev, rh.n_dst) if layout == LAYOUT_CELL_FAST else (rh.n_dst, nlev)
    res = [t if t is not None else torch.empty(shape, dtype=out_dtype, device=u.device) for t in outs]
    for t in res:
        if not (t.is_cuda and t.is_contiguous() and t.dtype == out_dtype and t.dtype in (torch.float32, torch.float64) and t.numel() == nlev * rh.n_dst):
            raise ValueError(who + ": outs must be contiguous float32/float64 CUDA tensors of %d elements and one dtype" % (nlev * rh.n_dst))
    if ACCOUNT is not None:     # nEdges L e_s + nout nCells L e_d + (4 + 8 nout) nnz: the source, every result, col and the values once
        ACCOUNT.append(("%s L%d x%d" % (who, nlev, nout), nlev * rh.n_src * u.element_size() + nout * rh.n_dst * nlev * res[0].element_size()
                        + (4 + 8 * nout) * rh.nnz))
    check(L.wind_reconstruct_dev(rh._h, m.data_ptr(), nout, u.data_ptr(), int(u.dtype == torch.float32), int(src_layout), ldu, int(nlev),
                                 res[0].data_ptr(), res[1].data_ptr() if nout > 1 else None, res[2].data_ptr() if nout > 2 else None,
                                 int(out_dtype == torch.float32), int(layout), torch.cuda.current_stream().cuda_stream))
    return tuple(res)


if _torch is not None:
    class WindReconstructFunction(_torch.autograd.Function):
        """wind_reconstruct with a gradient with respect to u (m is a constant): forward is wind_reconstruct in u's dtype; backward takes
        the incoming gradients back to [lev][cell] planes and applies regrid_transpose of the from-weights handles A_k (values m[k],
        _VectorAdjoint): gu = sum_k A_k^T g_k, returned in u's layout.  Use wind_reconstruct_autograd()."""

        @staticmethod
        def forward(ctx, u, rh, m, nlev, src_layout, layout):
            ctx.rh, ctx.m, ctx.nlev, ctx.src_layout, ctx.layout = rh, m, nlev, src_layout, layout
            ctx.shape, ctx.dtype = u.shape, u.dtype
            return wind_reconstruct(rh, m, u.contiguous(), nlev, src_layout=src_layout, layout=layout, out_dtype=u.dtype)

        @staticmethod
        def backward(ctx, *gs):
            n, ns, nlev = ctx.rh.n_dst, ctx.rh.n_src, ctx.nlev
            A = _VectorAdjoint.of(ctx.rh, ctx.m, len(gs))
            gu = None
            for k, g in enumerate(gs):                          # regrid_transpose reads [nlev][n_dst] planes
                if g is None:
                    continue
                if ctx.layout == LAYOUT_LEV_FAST:
                    g = g.reshape(n, nlev).t()
                t = A[k].regrid_transpose(g.reshape(nlev, n).contiguous(), nlev=nlev, layout=LAYOUT_CELL_FAST, out_dtype=ctx.dtype)
                gu = t if gu is None else gu + t
            if gu is None:
                return (None,) * 6
            gu = gu.reshape(nlev, ns)
            if ctx.src_layout == LAYOUT_LEV_FAST:
                gu = gu.t().contiguous()
            return (gu.reshape(ctx.shape),) + (None,) * 5


def wind_reconstruct_autograd(rh, m, u, nlev, src_layout=LAYOUT_LEV_FAST, layout=LAYOUT_CELL_FAST):
    """wind_reconstruct(rh, m, u, nlev, src_layout, layout) in u's dtype as a differentiable torch op.  The gradient with respect to u (m
    is a constant of the op): gu = sum_k A_k^T g_k with A_k the handle's pattern with the values m[k], through regrid_transpose of nout
    from-weights handles that the first backward builds from a download of rh.csr() and m and that stay with m; returned in u's shape,
    layout and dtype: the exact adjoint of the forward."""
    return WindReconstructFunction.apply(u, rh, m, nlev, src_layout, layout)


# ---- handle composition: two Regrids folded into one CSR handle ---------------------------------------------------------------------------
def compose(outer, inner):
    """mpg_handle_compose: C = outer . inner as ONE CSR RouteHandle -- "outer after inner" without the intermediate array.  n_src is
    inner's, n_dst / nx_dst / ny_dst are outer's; inner.n_dst must equal outer.n_src.  Either operand may be fixed or CSR (no pole terms).
    Row i holds the distinct sources reachable from outer's row i through inner's rows, ascending; the values are the ordered sums of
    target_grid.compose_csr, bit for bit.  The handle owns its arrays (outer and inner may be released), is not cached -- release() it --
    and every CSR consumer takes it: regrid_typed, regrid_csr_to_mesh, regrid_csr_rows, regrid_masked, regrid_transpose, the autograd
    ops, wind_vector_weights, wind_reconstruct, csr() and to_esmf_weights()."""
    h = C.c_void_p()
    check(L.handle_compose(outer._h if outer is not None else None, inner._h if inner is not None else None, C.byref(h)))
    return RouteHandle(h)


def compose_weights(composed, outer, inner, m_inner):
    """mpg_compose_weights_dev: caller-owned value planes of inner taken through the composition -- m_inner [K][inner.nnz] (K in 1..4, a
    float64 CUDA tensor in the order of inner.csr()'s entries, e.g. reconstruct_weights' or wind_vector_weights' blocks) -> [K][composed.nnz]
    float64 CUDA tensor in the order of composed.csr()'s entries, by compose's value rule with b_q = m_inner[k][q].  inner must be a CSR
    handle.  Neither allocates on the device side nor synchronises: capturable in a graph.  The bits of target_grid.compose_csr."""
    import torch
    if not (_is_torch(m_inner) and m_inner.is_cuda and m_inner.is_contiguous() and m_inner.dtype == torch.float64 and m_inner.dim() == 2
            and m_inner.shape[1] == inner.nnz):
        raise ValueError("compose_weights: m_inner must be a contiguous float64 CUDA tensor [K][nnz of inner = %d]" % inner.nnz)
    m = torch.empty((int(m_inner.shape[0]), composed.nnz), dtype=torch.float64, device=m_inner.device)
    check(L.compose_weights_dev(composed._h, outer._h, inner._h, int(m_inner.shape[0]), m_inner.data_ptr(), m.data_ptr(),
                                torch.cuda.current_stream().cuda_stream))
    return m


# ---- extrapolation: the unmapped rows of a handle filled from the nearest source points -----------------------------------------------------
def _points(obj, loc, who):
    if isinstance(obj, Mesh):
        return L.Points(mesh=obj._h, meshloc=int(MESHLOC_ELEMENT if loc is None else loc), grid=None, staggerloc=0)
    if isinstance(obj, Grid):
        return L.Points(mesh=None, meshloc=0, grid=obj._h, staggerloc=int(STAGGERLOC_CENTER if loc is None else loc))
    raise ValueError("extrapolate: %s must be a Mesh or a Grid" % who)


def extrapolate(rh, src, dst, method=EXTRAPMETHOD_NEAREST_STOD, num_src_pnts=8, dist_exponent=2.0, src_loc=None, dst_loc=None):
    """mpg_handle_extrapolate (ESMF's extrapMethod / extrapNumSrcPnts / extrapDistExponent): a new RouteHandle of rh's shape whose unmapped
    rows -- idx -1 in slot 0, or an empty CSR row -- are filled from the nearest points of `src`, every other row copied.  src / dst: the
    Mesh or Grid objects rh was stored on; src_loc / dst_loc: a mesh location or a stagger (default MESHLOC_ELEMENT / STAGGERLOC_CENTER;
    a source mesh is searched through its cells only).  EXTRAPMETHOD_NEAREST_STOD: the nearest source with weight 1.
    EXTRAPMETHOD_NEAREST_IDAVG: the num_src_pnts (1..EXTRAP_MAX_PNTS) nearest, weighted by distance ** -dist_exponent and normalised.  A
    fixed rh stays fixed when the new rows fit its slots (STOD; IDAVG with num_src_pnts <= nnz_per_row), otherwise the result is CSR.  The
    bits of target_grid.extrapolate_rows fed with src.xyz() / dst.xyz().  Not cached: release() it; rh may be released."""
    ps, pd = _points(src, src_loc, "src"), _points(dst, dst_loc, "dst")
    opts = L.ExtrapOpts(method=int(method), num_src_pnts=int(num_src_pnts), dist_exponent=float(dist_exponent))
    h = C.c_void_p()
    check(L.handle_extrapolate(rh._h if rh is not None else None, C.byref(ps), C.byref(pd), C.byref(opts), C.byref(h)))
    return RouteHandle(h)


# ---- Store-time masks: ESMF's srcMaskValues / dstMaskValues as handle-to-handle calls ------------------------------------------------------
def _mask_dev(m, n, who, name):
    """A byte mask of n elements on the device (non-zero = masked) from numpy or torch, bool or uint8; a host mask is uploaded.  None stays
    None.  -> the tensor (keep it alive over the call)."""
    if m is None:
        return None
    import torch
    if not _is_torch(m):
        m = np.asarray(m)
        if m.dtype not in (np.bool_, np.uint8):
            raise ValueError("%s: %s must be bool or uint8" % (who, name))
        m = torch.from_numpy(np.ascontiguousarray(m.reshape(-1)).astype(np.uint8))
    if m.dtype not in (torch.bool, torch.uint8):
        raise ValueError("%s: %s must be bool or uint8" % (who, name))
    m = m.reshape(-1).contiguous()
    if m.numel() != n:
        raise ValueError("%s: %s has %d elements, the handle expects %d" % (who, name, m.numel(), n))
    return m if m.is_cuda else m.cuda()


def _mask_ptr(m):
    return None if m is None or m.numel() == 0 else m.data_ptr()


def mask_handle(rh, src_mask=None, dst_mask=None, rule=MASKRULE_AUTO, norm_type=NORM_DSTAREA):
    """mpg_handle_mask (ESMF's srcMaskValues / dstMaskValues on a finished handle): a new RouteHandle of rh's shape and kind with static
    masks applied to its pattern.  src_mask [n_src] / dst_mask [n_dst]: numpy or torch, bool or uint8, non-zero = masked (a host mask is
    uploaded); None = no mask on that side.  A masked destination row becomes unmapped.  MASKRULE_ROW (bilinear, nearest): a row with a
    stored entry on a masked source becomes unmapped.  MASKRULE_ENTRY (conservative, CSR only): the entries of masked sources are removed,
    the rest renormalised by norm_type -- the one the Store was called with -- and dst_frac follows.  MASKRULE_AUTO picks by rh's method.
    The bits of target_grid.mask_rows.  Not cached: release() it; rh may be released."""
    ms = _mask_dev(src_mask, rh.n_src, "mask_handle", "src_mask")
    md = _mask_dev(dst_mask, rh.n_dst, "mask_handle", "dst_mask")
    opts = L.StoreMaskOpts(src_mask_dev=_mask_ptr(ms), dst_mask_dev=_mask_ptr(md), rule=int(rule), norm_type=int(norm_type))
    h = C.c_void_p()
    check(L.handle_mask(rh._h, C.byref(opts), C.byref(h)))
    return RouteHandle(h)


def extrapolate_masked(rh, src, dst, src_mask=None, dst_skip=None, method=EXTRAPMETHOD_NEAREST_STOD, num_src_pnts=8, dist_exponent=2.0,
                       src_loc=None, dst_loc=None):
    """mpg_handle_extrapolate_masked: extrapolate() with the candidates restricted to the sources whose src_mask is 0 -- K = min(N, unmasked
    sources), ties to the lower unmasked id -- and the unmapped rows whose dst_skip is non-zero left unmapped.  Masks as in mask_handle.
    With both masks None the bytes of extrapolate(); with every source masked nothing is filled.  The bits of
    target_grid.extrapolate_rows_masked fed with src.xyz() / dst.xyz().  Not cached: release() it; rh may be released."""
    ps, pd = _points(src, src_loc, "src"), _points(dst, dst_loc, "dst")
    ms = _mask_dev(src_mask, rh.n_src, "extrapolate_masked", "src_mask")
    md = _mask_dev(dst_skip, rh.n_dst, "extrapolate_masked", "dst_skip")
    opts = L.ExtrapOpts(method=int(method), num_src_pnts=int(num_src_pnts), dist_exponent=float(dist_exponent))
    h = C.c_void_p()
    check(L.handle_extrapolate_masked(rh._h, C.byref(ps), C.byref(pd), C.byref(opts), _mask_ptr(ms), _mask_ptr(md), C.byref(h)))
    return RouteHandle(h)


def store_masks(rh, src, dst, src_mask=None, dst_mask=None, norm_type=NORM_DSTAREA, extrap_method=None, num_src_pnts=8, dist_exponent=2.0,
                src_loc=None, dst_loc=None):
    """ESMF_FieldRegridStore(srcMaskValues, dstMaskValues, extrapMethod, normType) on a finished handle: mask_handle (rule by rh's method),
    then extrapolate_masked with the same source mask and dst_skip = dst_mask.  A NEAREST_STOD handle is always refilled with
    EXTRAPMETHOD_NEAREST_STOD -- every unmasked destination takes the nearest UNMASKED source, which is ESMF's result; the other methods
    are refilled with extrap_method only when it is set.  The intermediate handle is released.  Not cached: release() the result."""
    masked = mask_handle(rh, src_mask, dst_mask, MASKRULE_AUTO, norm_type)
    nearest = rh.nnz_per_row == 1        # one slot per row: the nearest Stores' handles and no others (mpg_handle_info)
    if not nearest and extrap_method is None:
        return masked
    try:
        return extrapolate_masked(masked, src, dst, src_mask, dst_mask, EXTRAPMETHOD_NEAREST_STOD if nearest else extrap_method, num_src_pnts,
                                  dist_exponent, src_loc, dst_loc)
    finally:
        masked.release()


# ---- patch regridding: second-degree patch recovery as a CSR handle -------------------------------------------------------------------------
REGRIDMETHOD_PATCH, PATCH_MAX_PNTS = L.REGRIDMETHOD_PATCH, L.PATCH_MAX_PNTS


def patch(rh, src, dst, src_loc=None, dst_loc=None):
    """mpg_handle_patch (ESMF_REGRIDMETHOD_PATCH): a new CSR RouteHandle of rh's shape in which every source node of a bilinear row is
    replaced by the second-degree least-squares polynomial through its neighbours, blended with the row's bilinear weights.  rh: a fixed
    bilinear handle of 3 or 4 slots; src / dst: the Mesh or Grid objects rh was stored between; src_loc / dst_loc: a mesh location or a
    stagger (default MESHLOC_ELEMENT / STAGGERLOC_CENTER; a source mesh takes part with its cells only).  store_stats: [1] rows written,
    [2..5] (row, slot) pairs served by attempts A, B, C, D, [6] the longest row.  The bits of target_grid.patch_rows fed with
    rh.weights(), src.xyz() / dst.xyz() and patch_neighbours_mesh / _grid.  Patch first, then mask_handle / extrapolate.  Not cached:
    release() it; rh may be released."""
    ps, pd = _points(src, src_loc, "src"), _points(dst, dst_loc, "dst")
    h = C.c_void_p()
    check(L.handle_patch(rh._h if rh is not None else None, C.byref(ps), C.byref(pd), C.byref(h)))
    return RouteHandle(h)


def regrid_store_patch(src, dst, src_loc=None, dst_loc=None):
    """Store bilinear, patch, release: the patch handle between src and dst (Mesh or Grid each; src is dst for the CENTER -> EDGE1 / EDGE2
    handles of one grid, with dst_loc the destination stagger; two different grids go through regrid_store_grid_to_grid).  The bilinear handle goes back to the Store cache.  Not cached itself:
    release() the result."""
    if isinstance(src, Mesh) and isinstance(dst, Grid):
        rh = regrid_store(src, dst, REGRIDMETHOD_BILINEAR, STAGGERLOC_CENTER if dst_loc is None else dst_loc)
    elif isinstance(src, Mesh) and isinstance(dst, Mesh):
        rh = regrid_store_mesh(src, dst, REGRIDMETHOD_BILINEAR, MESHLOC_ELEMENT, MESHLOC_ELEMENT if dst_loc is None else dst_loc)
    elif isinstance(src, Grid) and isinstance(dst, Mesh):
        rh = regrid_store_to_mesh(src, dst, REGRIDMETHOD_BILINEAR, STAGGERLOC_CENTER if src_loc is None else src_loc,
                                  MESHLOC_ELEMENT if dst_loc is None else dst_loc)
    elif isinstance(src, Grid) and src is dst:
        rh = regrid_store_grid(src, STAGGERLOC_EDGE1 if dst_loc is None else dst_loc, STAGGERLOC_CENTER if src_loc is None else src_loc)
    elif isinstance(src, Grid) and isinstance(dst, Grid):
        rh = regrid_store_grid_to_grid(src, dst, REGRIDMETHOD_BILINEAR, STAGGERLOC_CENTER if src_loc is None else src_loc,
                                       STAGGERLOC_CENTER if dst_loc is None else dst_loc)
    else:
        raise ValueError("regrid_store_patch: src and dst must be Mesh or Grid objects")
    try:
        return patch(rh, src, dst, src_loc, dst_loc)
    finally:
        rh.release()


# ---- second-order conservative regridding: a linear reconstruction inside every source cell, as a CSR handle -------------------------------
REGRIDMETHOD_CONSERVE_2ND = L.REGRIDMETHOD_CONSERVE_2ND


def conserve_2nd(rh, src, dst, norm=NORM_DSTAREA, src_mask=None, src_loc=None, dst_loc=None):
    """mpg_handle_conserve2nd (ESMF_REGRIDMETHOD_CONSERVE_2ND): a new CSR RouteHandle of rh's shape in which every source cell carries a
    least-squares gradient over its neighbours' means and every stored piece is evaluated at its own centroid.  rh: a first-order
    conservative CSR handle (regrid_store with REGRIDMETHOD_CONSERVE, regrid_store_conserve_to_mesh, regrid_store_conserve_mesh), also
    after mask_handle(rule=MASKRULE_ENTRY); src / dst: the Mesh or Grid objects rh was stored between (cells on both sides: MESHLOC_ELEMENT
    / STAGGERLOC_CENTER, the defaults of src_loc / dst_loc); norm: the one the Store was called with; src_mask [n_src]: numpy or torch,
    bool or uint8, non-zero = masked -- masked cells take no part in a gradient (mask rh with the same mask first).  The integral is kept
    as rh keeps it and the row sums are rh's; weights may be negative (no limiter).  store_stats: [1] pairs clipped, [2] sources with a
    passing stencil, [3] sources without one, [4] stencil entries, [6] the longest row.  The bits of target_grid.conserve2nd_rows.  Not
    cached: release() it; rh may be released."""
    ps, pd = _points(src, src_loc, "src"), _points(dst, dst_loc, "dst")
    ms = _mask_dev(src_mask, rh.n_src, "conserve_2nd", "src_mask") if rh is not None else None
    opts = L.Conserve2ndOpts(norm_type=int(norm), src_mask_dev=_mask_ptr(ms))
    h = C.c_void_p()
    check(L.handle_conserve2nd(rh._h if rh is not None else None, C.byref(ps), C.byref(pd), C.byref(opts), C.byref(h)))
    return RouteHandle(h)


def regrid_store_conserve_2nd(src, dst, norm=NORM_DSTAREA):
    """Store first-order conservative, convert, release: the second-order conservative handle between the cells of src and dst (Mesh ->
    Grid, Grid -> Mesh, Mesh -> Mesh or Grid -> Grid between two different grids, picked by the operand types).  The first-order handle goes back to the Store cache.  Not cached
    itself: release() the result."""
    if isinstance(src, Mesh) and isinstance(dst, Grid):
        if norm != NORM_DSTAREA:
            raise ValueError("regrid_store_conserve_2nd: the Mesh -> Grid conservative Store normalises by the destination area (NORM_DSTAREA) only")
        rh = regrid_store(src, dst, REGRIDMETHOD_CONSERVE)
    elif isinstance(src, Grid) and isinstance(dst, Mesh):
        rh = regrid_store_conserve_to_mesh(src, dst, norm)
    elif isinstance(src, Mesh) and isinstance(dst, Mesh):
        rh = regrid_store_conserve_mesh(src, dst, norm)
    elif isinstance(src, Grid) and isinstance(dst, Grid) and src is not dst:
        rh = regrid_store_conserve_grid_to_grid(src, dst, norm)
    else:
        raise ValueError("regrid_store_conserve_2nd: src and dst must be a Mesh and a Grid, a Grid and a Mesh, two Meshes or two different Grids")
    try:
        return conserve_2nd(rh, src, dst, norm)
    finally:
        rh.release()


# ---- creep-fill extrapolation: the unmapped rows of a handle filled level by level from their neighbours' rows ------------------------------
CREEP_ALL_LEVELS = L.CREEP_ALL_LEVELS


def creep(rh, dst, num_levels=CREEP_ALL_LEVELS, dst_skip=None, dst_loc=None):
    """mpg_handle_creep (ESMF_EXTRAPMETHOD_CREEP with extrapNumLevels): a new CSR RouteHandle of rh's shape whose unmapped rows -- idx -1 in
    slot 0, or an empty CSR row -- are filled level by level: a point next to level L - 1 takes level L, and its row is the average of
    the rows of its neighbours of level L - 1 (mapped rows are level 0 and are copied).  dst: the Mesh or Grid rh was stored onto;
    dst_loc: a stagger (default STAGGERLOC_CENTER; the 8 surrounding points are the neighbours) or MESHLOC_ELEMENT (the cells that share
    a dual triangle).  num_levels >= 1, CREEP_ALL_LEVELS = until no row is filled any more.  dst_skip [n_dst]: numpy or torch, bool or
    uint8, non-zero = never filled and never a neighbour (after mask_handle: its destination mask).  store_stats: [1] rows filled, [2]
    the last level that filled a row, [3] rows still unmapped, [6] the longest row.  The bits of target_grid.creep_rows fed with rh.csr()
    / fixed_to_csr(rh.weights()) and creep_neighbours_grid / _mesh.  Not cached: release() it; rh may be released."""
    pd = _points(dst, dst_loc, "dst")
    md = _mask_dev(dst_skip, rh.n_dst, "creep", "dst_skip") if rh is not None else None
    opts = L.CreepOpts(num_levels=int(num_levels), dst_skip_dev=_mask_ptr(md))
    h = C.c_void_p()
    check(L.handle_creep(rh._h if rh is not None else None, C.byref(pd), C.byref(opts), C.byref(h)))
    return RouteHandle(h)


def creep_nearest(rh, src, dst, num_levels, src_mask=None, dst_skip=None, src_loc=None, dst_loc=None):
    """ESMF_EXTRAPMETHOD_CREEP_NRST_D: creep() for num_levels levels, then what is left unmapped takes the nearest source
    (EXTRAPMETHOD_NEAREST_STOD): extrapolate(), or extrapolate_masked() when src_mask or dst_skip is given -- the nearest UNMASKED source,
    the dst_skip rows left unmapped by both steps.  src / dst: the Mesh or Grid objects rh was stored between.  The crept intermediate is
    released.  The result is CSR (the creep's output kind).  Not cached: release() it; rh may be released."""
    crept = creep(rh, dst, num_levels, dst_skip, dst_loc)
    try:
        if src_mask is None and dst_skip is None:
            return extrapolate(crept, src, dst, EXTRAPMETHOD_NEAREST_STOD, src_loc=src_loc, dst_loc=dst_loc)
        return extrapolate_masked(crept, src, dst, src_mask, dst_skip, EXTRAPMETHOD_NEAREST_STOD, src_loc=src_loc, dst_loc=dst_loc)
    finally:
        crept.release()


# ---- nearest destination to source: every source onto its nearest destination point -------------------------------------------------------
REGRIDMETHOD_NEAREST_DTOS, DTOS_SUM, DTOS_MEAN = L.REGRIDMETHOD_NEAREST_DTOS, L.DTOS_SUM, L.DTOS_MEAN


def _points_n(obj, loc):
    if isinstance(obj, Mesh):
        loc = MESHLOC_ELEMENT if loc is None else loc
        return obj.nEdges if loc == MESHLOC_EDGE else obj.nCells if loc == MESHLOC_ELEMENT else obj.nVertices
    return int(np.prod(obj.stagger_shape(STAGGERLOC_CENTER if loc is None else loc)))


def regrid_store_nearest_dtos(src, dst, norm=DTOS_SUM, src_mask=None, dst_mask=None, src_loc=None, dst_loc=None):
    """mpg_regrid_store_nearest_dtos (ESMF_REGRIDMETHOD_NEAREST_DTOS): every point of `src` goes to the ONE point of `dst` nearest to it --
    the smallest (d2, id), a tie to the lower destination id -- and row d of the CSR RouteHandle lists the sources that chose d in
    ascending id.  src: a Mesh (src_loc MESHLOC_ELEMENT, _NODE or _EDGE; default cells) or a Grid (src_loc a stagger; default CENTER);
    dst: a Grid (dst_loc a stagger) or a Mesh's cells.  DTOS_SUM: every value 1.0 (a count / a sum per destination, ESMF's rule);
    DTOS_MEAN: 1.0 / the row's length (a box average).  src_mask [n_src] / dst_mask [n_dst]: numpy or torch, bool or uint8, non-zero =
    masked (a host mask is uploaded): a masked source goes nowhere, a masked destination is no candidate.  A destination nobody chose
    has an empty row.  src_nearest() is the binning index.  The bits of target_grid.nearest_dtos_rows fed with src.xyz() / dst.xyz().
    Not cached: release() it."""
    ps, pd = _points(src, src_loc, "src"), _points(dst, dst_loc, "dst")
    ms = md = None
    if src_mask is not None:
        ms = _mask_dev(src_mask, _points_n(src, src_loc), "regrid_store_nearest_dtos", "src_mask")
    if dst_mask is not None:
        md = _mask_dev(dst_mask, _points_n(dst, dst_loc), "regrid_store_nearest_dtos", "dst_mask")
    h = C.c_void_p()
    check(L.regrid_store_nearest_dtos(C.byref(ps), C.byref(pd), int(norm), _mask_ptr(ms), _mask_ptr(md), C.byref(h)))
    return RouteHandle(h)
