"""ctypes binding of libmpassit_amd.so (the C-ABI of include/mpassit_amd.h).

There is no CPU implementation behind this module: if the HIP library is missing, or no GPU is
present at `init()`, every entry point raises.  Nothing here imports the test oracle.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("MPASSIT_AMD_LIB") or os.path.join(_HERE, "libmpassit_amd.so")   # override: A/B builds of experiments

# every symbol include/mpassit_amd.h declares (tests check they are all exported)
SYMBOLS = [
    "mpg_init", "mpg_finalize", "mpg_last_error", "mpg_device_info", "mpg_mesh_create", "mpg_mesh_create_window", "mpg_mesh_window_info", "mpg_mesh_destroy",
    "mpg_grid_create", "mpg_grid_attach_proj", "mpg_grid_destroy", "mpg_regrid_store", "mpg_regrid_store_grid", "mpg_regrid_store_begin", "mpg_regrid_store_grid_begin", "mpg_regrid",
    "mpg_regrid_dev", "mpg_regrid_typed_dev", "mpg_regrid_typed", "mpg_handle_release", "mpg_rotate_winds", "mpg_rotate_winds_dev", "mpg_wind_destagger_dev", "mpg_wind_destagger", "mpg_handle_info",
    "mpg_handle_from_weights", "mpg_handle_get_weights", "mpg_handle_get_csr", "mpg_mesh_get_triangles", "mpg_handle_unique_sources",
    "mpg_handle_localize", "mpg_handle_rebase", "mpg_pack_dev", "mpg_handle_store_ms", "mpg_regrid_bundle_typed_dev", "mpg_regrid_bundle_typed", "mpg_handle_store_path", "mpg_tune", "mpg_handle_pole_count", "mpg_handle_kernel_choice", "mpg_handle_tile_stats",
    "mpg_handle_get_pole", "mpg_bswap_dev", "mpg_file_to_dev", "mpg_dev_to_file", "mpg_dev_alloc", "mpg_dev_free", "mpg_dev_upload", "mpg_dev_download", "mpg_post_cast_dev", "mpg_post_layer_mean_dev", "mpg_post_ptop_dev", "mpg_post_ptop_parts_dev", "mpg_grid_create_proj", "mpg_grid_get_coords",
    "mpg_grid_get_rotang", "mpg_grid_get_mapfac", "mpg_grid_rotang_dev", "mpg_handle_source_range", "mpg_mesh_set_source_window",
    "mpg_comm_init", "mpg_comm_destroy", "mpg_comm_info", "mpg_comm_allgather", "mpg_halo_build", "mpg_halo_info", "mpg_halo_exchange_dev",
    "mpg_halo_destroy", "mpg_gather_rows", "mpg_halo_plan_host", "mpg_comm_idfile_verdict", "mpg_pack_rows_dev", "mpg_comm_virtual",
    "mpg_comm_virtual_stats", "mpg_handle_store_stats", "mpg_debug_scan_i32", "mpg_device_count", "mpg_warmup_wait", "mpg_halo_build_owned", "mpg_halo_plan_owned_host",
    "mpg_dst_level_stride", "mpg_regrid_pitched_dev", "mpg_regrid_typed_pitched_dev", "mpg_regrid_bundle_typed_pitched_dev",
    "mpg_wind_destagger_pitched_dev", "mpg_dev_to_file_planes", "mpg_regrid_transpose_dev", "mpg_handle_transpose_stats",
    "mpg_handle_transpose_build_ms", "mpg_regrid_masked_dev", "mpg_regrid_store_to_mesh", "mpg_regrid_to_mesh_dev",
    "mpg_regrid_store_conserve_to_mesh", "mpg_handle_get_dst_frac", "mpg_regrid_csr_to_mesh_dev",
    "mpg_regrid_store_mesh", "mpg_regrid_rows_dev",
    "mpg_regrid_store_conserve_mesh", "mpg_regrid_csr_rows_dev",
    "mpg_regrid_store_periodic_to_mesh",
    "mpg_wind_to_mesh_dev", "mpg_mesh_rotang_dev",
    "mpg_mesh_set_edges", "mpg_mesh_edge_count", "mpg_mesh_edge_rotang_dev", "mpg_wind_to_edges_dev",
    "mpg_wind_csr_to_mesh_dev", "mpg_wind_csr_to_edges_dev",
    "mpg_sphere_frames_dev", "mpg_wind_vector_weights_dev", "mpg_wind_vector_dev",
    "mpg_reconstruct_store", "mpg_reconstruct_weights_dev", "mpg_wind_reconstruct_dev",
    "mpg_handle_compose", "mpg_compose_weights_dev",
    "mpg_rotate_winds_transpose_dev", "mpg_wind_destagger_transpose_dev",
    "mpg_regrid_masked_transpose_dev",
    "mpg_handle_extrapolate", "mpg_mesh_get_xyz", "mpg_grid_get_xyz",
    "mpg_handle_mask", "mpg_handle_extrapolate_masked",
    "mpg_handle_patch",
    "mpg_handle_conserve2nd",
    "mpg_handle_creep",
    "mpg_regrid_store_grid_to_grid", "mpg_regrid_store_conserve_grid_to_grid",
    "mpg_regrid_store_nearest_dtos", "mpg_handle_get_src_nearest",
]

MPG_SUCCESS = 0
MPG_ERR_INVALID_ARG, MPG_ERR_UNSUPPORTED, MPG_ERR_OVERFLOW = 2, 4, 5
REGRIDMETHOD_BILINEAR, REGRIDMETHOD_CONSERVE, REGRIDMETHOD_NEAREST_STOD = 0, 1, 2
MESHLOC_ELEMENT, MESHLOC_NODE, MESHLOC_EDGE = 0, 1, 2
STAGGERLOC_CENTER, STAGGERLOC_EDGE1, STAGGERLOC_EDGE2, STAGGERLOC_CORNER = 0, 1, 2, 3
LAYOUT_CELL_FAST, LAYOUT_LEV_FAST = 0, 1
GRID_PERIODIC_I, GRID_NO_SOUTH_POLE, GRID_NO_NORTH_POLE = 1, 2, 4

MISSING_NAN, MISSING_VALUE = 1, 2
MPG_NORM_DSTAREA, MPG_NORM_FRACAREA = 0, 1
NORM_DSTAREA, NORM_FRACAREA = MPG_NORM_DSTAREA, MPG_NORM_FRACAREA
MPG_POLEMETHOD_NONE, MPG_POLEMETHOD_ALLAVG = 0, 1
POLEMETHOD_NONE, POLEMETHOD_ALLAVG = MPG_POLEMETHOD_NONE, MPG_POLEMETHOD_ALLAVG
MPG_EXTRAPMETHOD_NEAREST_STOD, MPG_EXTRAPMETHOD_NEAREST_IDAVG = 1, 2
EXTRAPMETHOD_NEAREST_STOD, EXTRAPMETHOD_NEAREST_IDAVG = MPG_EXTRAPMETHOD_NEAREST_STOD, MPG_EXTRAPMETHOD_NEAREST_IDAVG
EXTRAP_MAX_PNTS = 8
MPG_REGRIDMETHOD_PATCH = 3   # the method of mpg_handle_patch's handles; no Store takes it
REGRIDMETHOD_PATCH = MPG_REGRIDMETHOD_PATCH
PATCH_MAX_PNTS = 32
MPG_REGRIDMETHOD_CONSERVE_2ND = 4   # the method of mpg_handle_conserve2nd's handles; no Store takes it
REGRIDMETHOD_CONSERVE_2ND = MPG_REGRIDMETHOD_CONSERVE_2ND
MPG_CREEP_ALL_LEVELS = 0x7fffffff   # mpg_creep_opts.num_levels: until no row is filled any more
CREEP_ALL_LEVELS = MPG_CREEP_ALL_LEVELS
MPG_REGRIDMETHOD_NEAREST_DTOS = 5   # the method of mpg_regrid_store_nearest_dtos's handles
REGRIDMETHOD_NEAREST_DTOS = MPG_REGRIDMETHOD_NEAREST_DTOS
MPG_DTOS_SUM, MPG_DTOS_MEAN = 0, 1
DTOS_SUM, DTOS_MEAN = MPG_DTOS_SUM, MPG_DTOS_MEAN
MPG_MASKRULE_AUTO, MPG_MASKRULE_ROW, MPG_MASKRULE_ENTRY = 0, 1, 2
MASKRULE_AUTO, MASKRULE_ROW, MASKRULE_ENTRY = MPG_MASKRULE_AUTO, MPG_MASKRULE_ROW, MPG_MASKRULE_ENTRY


class MaskOpts(C.Structure):
    """mpg_mask_opts of include/mpassit_amd.h (mpg_regrid_masked_dev)."""
    _fields_ = [("flags", C.c_int), ("missing_value", C.c_double), ("src_mask_dev", C.c_void_p), ("min_valid_frac", C.c_double),
                ("fill_value", C.c_double), ("scale", C.c_double), ("offset", C.c_double)]


# mpg_regrid_masked_dev with its argument types (rh, src_dev, src_type, src_layout, nlev, nfields, dst_dev, dst_type, dst_level_stride,
# opts, hip_stream).  A prototype of its own: the attribute of the loaded library stays untyped like every other entry point.
_MASKED_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64,
                            C.POINTER(MaskOpts), C.c_void_p)
_masked_fn = None


def regrid_masked_dev(*args):
    """The typed binding of mpg_regrid_masked_dev; returns the call's status code."""
    global _masked_fn
    if _masked_fn is None:
        _masked_fn = _MASKED_PROTO(("mpg_regrid_masked_dev", load()))
    return _masked_fn(*args)


# Its adjoint, bound the same way:
#   mpg_regrid_masked_transpose_dev(rh, g_dev, g_type, g_level_stride, src_dev, src_type, src_layout, nlev, nfields, dst_dev, dst_type,
#                                   opts, work_dev, hip_stream)
_REGRID_MASKED_TRANSPOSE_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_void_p, C.c_int, C.POINTER(MaskOpts), C.c_void_p, C.c_void_p)
_masked_transpose_fn = None


def regrid_masked_transpose_dev(*args):
    """The typed binding of mpg_regrid_masked_transpose_dev; returns the call's status code."""
    global _masked_transpose_fn
    if _masked_transpose_fn is None:
        _masked_transpose_fn = _REGRID_MASKED_TRANSPOSE_PROTO(("mpg_regrid_masked_transpose_dev", load()))
    return _masked_transpose_fn(*args)


# The Grid -> Mesh calls with their argument types, bound like the masked Regrid above.
#   mpg_regrid_store_to_mesh(src grid, src_staggerloc, dst mesh, dst_meshloc, regridmethod, out)
#   mpg_regrid_to_mesh_dev(rh, src_dev, src_type, src_level_stride, nlev, nfields, dst_dev, dst_type, dst_layout, scale, offset, hip_stream)
_STORE_TO_MESH_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p))
_TO_MESH_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double,
                             C.c_double, C.c_void_p)
_to_mesh_fns = {}


def regrid_store_to_mesh(*args):
    """The typed binding of mpg_regrid_store_to_mesh; returns the call's status code."""
    if "store" not in _to_mesh_fns:
        _to_mesh_fns["store"] = _STORE_TO_MESH_PROTO(("mpg_regrid_store_to_mesh", load()))
    return _to_mesh_fns["store"](*args)


def regrid_to_mesh_dev(*args):
    """The typed binding of mpg_regrid_to_mesh_dev; returns the call's status code."""
    if "apply" not in _to_mesh_fns:
        _to_mesh_fns["apply"] = _TO_MESH_PROTO(("mpg_regrid_to_mesh_dev", load()))
    return _to_mesh_fns["apply"](*args)


# The conservative Grid -> Mesh calls, bound the same way.
#   mpg_regrid_store_conserve_to_mesh(src grid, dst mesh, norm_type, out)
#   mpg_handle_get_dst_frac(rh, frac_host)
#   mpg_regrid_csr_to_mesh_dev(rh, src_dev, src_type, src_level_stride, nlev, nfields, dst_dev, dst_type, dst_layout, scale, offset, hip_stream)
_STORE_CONSERVE_TO_MESH_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p))
_DST_FRAC_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)
_CSR_TO_MESH_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double,
                                 C.c_double, C.c_void_p)


def regrid_store_conserve_to_mesh(*args):
    """The typed binding of mpg_regrid_store_conserve_to_mesh; returns the call's status code."""
    if "cstore" not in _to_mesh_fns:
        _to_mesh_fns["cstore"] = _STORE_CONSERVE_TO_MESH_PROTO(("mpg_regrid_store_conserve_to_mesh", load()))
    return _to_mesh_fns["cstore"](*args)


def handle_get_dst_frac(*args):
    """The typed binding of mpg_handle_get_dst_frac; returns the call's status code."""
    if "frac" not in _to_mesh_fns:
        _to_mesh_fns["frac"] = _DST_FRAC_PROTO(("mpg_handle_get_dst_frac", load()))
    return _to_mesh_fns["frac"](*args)


def regrid_csr_to_mesh_dev(*args):
    """The typed binding of mpg_regrid_csr_to_mesh_dev; returns the call's status code."""
    if "capply" not in _to_mesh_fns:
        _to_mesh_fns["capply"] = _CSR_TO_MESH_PROTO(("mpg_regrid_csr_to_mesh_dev", load()))
    return _to_mesh_fns["capply"](*args)


# The Mesh -> Mesh calls, bound the same way.
#   mpg_regrid_store_mesh(src mesh, src_meshloc, dst mesh, dst_meshloc, regridmethod, out)
#   mpg_regrid_rows_dev(rh, src_dev, src_type, nlev, nfields, dst_dev, dst_type, scale, offset, hip_stream)
_STORE_MESH_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p))
_ROWS_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p)


def regrid_store_mesh(*args):
    """The typed binding of mpg_regrid_store_mesh; returns the call's status code."""
    if "mstore" not in _to_mesh_fns:
        _to_mesh_fns["mstore"] = _STORE_MESH_PROTO(("mpg_regrid_store_mesh", load()))
    return _to_mesh_fns["mstore"](*args)


def regrid_rows_dev(*args):
    """The typed binding of mpg_regrid_rows_dev; returns the call's status code."""
    if "rows" not in _to_mesh_fns:
        _to_mesh_fns["rows"] = _ROWS_PROTO(("mpg_regrid_rows_dev", load()))
    return _to_mesh_fns["rows"](*args)


# The conservative Mesh -> Mesh calls, bound the same way.
#   mpg_regrid_store_conserve_mesh(src mesh, dst mesh, norm_type, out)
#   mpg_regrid_csr_rows_dev(rh, src_dev, src_type, nlev, nfields, dst_dev, dst_type, scale, offset, hip_stream)
_STORE_CONSERVE_MESH_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p))
_CSR_ROWS_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p)


def regrid_store_conserve_mesh(*args):
    """The typed binding of mpg_regrid_store_conserve_mesh; returns the call's status code."""
    if "cmstore" not in _to_mesh_fns:
        _to_mesh_fns["cmstore"] = _STORE_CONSERVE_MESH_PROTO(("mpg_regrid_store_conserve_mesh", load()))
    return _to_mesh_fns["cmstore"](*args)


def regrid_csr_rows_dev(*args):
    """The typed binding of mpg_regrid_csr_rows_dev; returns the call's status code."""
    if "crows" not in _to_mesh_fns:
        _to_mesh_fns["crows"] = _CSR_ROWS_PROTO(("mpg_regrid_csr_rows_dev", load()))
    return _to_mesh_fns["crows"](*args)


# The bilinear Grid -> Mesh Store of a periodic grid, bound the same way.
#   mpg_regrid_store_periodic_to_mesh(src grid, dst mesh, dst_meshloc, pole_method, out)
_STORE_PERIODIC_TO_MESH_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p))


def regrid_store_periodic_to_mesh(*args):
    """The typed binding of mpg_regrid_store_periodic_to_mesh; returns the call's status code."""
    if "pstore" not in _to_mesh_fns:
        _to_mesh_fns["pstore"] = _STORE_PERIODIC_TO_MESH_PROTO(("mpg_regrid_store_periodic_to_mesh", load()))
    return _to_mesh_fns["pstore"](*args)


# The Stores between two grids, bound the same way.
#   mpg_regrid_store_grid_to_grid(src grid, src_staggerloc, dst grid, dst_staggerloc, regridmethod, pole_method, out)
#   mpg_regrid_store_conserve_grid_to_grid(src grid, dst grid, norm_type, out)
_STORE_GRID_TO_GRID_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p))
_STORE_CONSERVE_GRID_TO_GRID_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p))


def regrid_store_grid_to_grid(*args):
    """The typed binding of mpg_regrid_store_grid_to_grid; returns the call's status code."""
    if "ggstore" not in _to_mesh_fns:
        _to_mesh_fns["ggstore"] = _STORE_GRID_TO_GRID_PROTO(("mpg_regrid_store_grid_to_grid", load()))
    return _to_mesh_fns["ggstore"](*args)


def regrid_store_conserve_grid_to_grid(*args):
    """The typed binding of mpg_regrid_store_conserve_grid_to_grid; returns the call's status code."""
    if "cggstore" not in _to_mesh_fns:
        _to_mesh_fns["cggstore"] = _STORE_CONSERVE_GRID_TO_GRID_PROTO(("mpg_regrid_store_conserve_grid_to_grid", load()))
    return _to_mesh_fns["cggstore"](*args)


# The wind chain turned round and the rotation angles it needs, bound the same way.
#   mpg_wind_to_mesh_dev(rh_u, rh_v, cosa_dev, sina_dev, u_dev, v_dev, src_type, u_level_stride, v_level_stride, nlev, ue_dev, ve_dev,
#                        dst_type, dst_layout, hip_stream)
#   mpg_mesh_rotang_dev(grid, mesh, meshloc, cosa_dev, sina_dev, hip_stream)
_WIND_TO_MESH_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64,
                                  C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p)
_MESH_ROTANG_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)


def wind_to_mesh_dev(*args):
    """The typed binding of mpg_wind_to_mesh_dev; returns the call's status code."""
    if "wind" not in _to_mesh_fns:
        _to_mesh_fns["wind"] = _WIND_TO_MESH_PROTO(("mpg_wind_to_mesh_dev", load()))
    return _to_mesh_fns["wind"](*args)


def mesh_rotang_dev(*args):
    """The typed binding of mpg_mesh_rotang_dev; returns the call's status code."""
    if "rotang" not in _to_mesh_fns:
        _to_mesh_fns["rotang"] = _MESH_ROTANG_PROTO(("mpg_mesh_rotang_dev", load()))
    return _to_mesh_fns["rotang"](*args)


# The mesh's edges and the winds onto them, bound the same way.
#   mpg_mesh_set_edges(mesh, nEdges, latEdge, lonEdge, angleEdge)
#   mpg_mesh_edge_count(mesh, nEdges)
#   mpg_mesh_edge_rotang_dev(grid, mesh, cn_dev, sn_dev, hip_stream)
#   mpg_wind_to_edges_dev(rh_u, rh_v, cn_dev, sn_dev, u_dev, v_dev, src_type, u_level_stride, v_level_stride, nlev, un_dev, ut_dev,
#                         dst_type, dst_layout, hip_stream)
_MESH_SET_EDGES_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p)
_MESH_EDGE_COUNT_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int64))
_MESH_EDGE_ROTANG_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_WIND_TO_EDGES_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64,
                                   C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p)


def mesh_set_edges(*args):
    """The typed binding of mpg_mesh_set_edges; returns the call's status code."""
    if "set_edges" not in _to_mesh_fns:
        _to_mesh_fns["set_edges"] = _MESH_SET_EDGES_PROTO(("mpg_mesh_set_edges", load()))
    return _to_mesh_fns["set_edges"](*args)


def mesh_edge_count(*args):
    """The typed binding of mpg_mesh_edge_count; returns the call's status code."""
    if "edge_count" not in _to_mesh_fns:
        _to_mesh_fns["edge_count"] = _MESH_EDGE_COUNT_PROTO(("mpg_mesh_edge_count", load()))
    return _to_mesh_fns["edge_count"](*args)


def mesh_edge_rotang_dev(*args):
    """The typed binding of mpg_mesh_edge_rotang_dev; returns the call's status code."""
    if "edge_rotang" not in _to_mesh_fns:
        _to_mesh_fns["edge_rotang"] = _MESH_EDGE_ROTANG_PROTO(("mpg_mesh_edge_rotang_dev", load()))
    return _to_mesh_fns["edge_rotang"](*args)


def wind_to_edges_dev(*args):
    """The typed binding of mpg_wind_to_edges_dev; returns the call's status code."""
    if "wind_edges" not in _to_mesh_fns:
        _to_mesh_fns["wind_edges"] = _WIND_TO_EDGES_PROTO(("mpg_wind_to_edges_dev", load()))
    return _to_mesh_fns["wind_edges"](*args)


# The two wind calls for CSR handles, bound the same way: the argument lists of mpg_wind_to_mesh_dev and mpg_wind_to_edges_dev.
#   mpg_wind_csr_to_mesh_dev(rh_u, rh_v, cosa_dev, sina_dev, u_dev, v_dev, src_type, u_level_stride, v_level_stride, nlev, ue_dev, ve_dev,
#                            dst_type, dst_layout, hip_stream)
#   mpg_wind_csr_to_edges_dev(rh_u, rh_v, cn_dev, sn_dev, u_dev, v_dev, src_type, u_level_stride, v_level_stride, nlev, un_dev, ut_dev,
#                             dst_type, dst_layout, hip_stream)
_WIND_CSR_TO_MESH_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64,
                                      C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p)
_WIND_CSR_TO_EDGES_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64,
                                       C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p)


def wind_csr_to_mesh_dev(*args):
    """The typed binding of mpg_wind_csr_to_mesh_dev; returns the call's status code."""
    if "wind_csr" not in _to_mesh_fns:
        _to_mesh_fns["wind_csr"] = _WIND_CSR_TO_MESH_PROTO(("mpg_wind_csr_to_mesh_dev", load()))
    return _to_mesh_fns["wind_csr"](*args)


def wind_csr_to_edges_dev(*args):
    """The typed binding of mpg_wind_csr_to_edges_dev; returns the call's status code."""
    if "wind_csr_edges" not in _to_mesh_fns:
        _to_mesh_fns["wind_csr_edges"] = _WIND_CSR_TO_EDGES_PROTO(("mpg_wind_csr_to_edges_dev", load()))
    return _to_mesh_fns["wind_csr_edges"](*args)


# A wind as a vector through one CSR handle, bound the same way.
#   mpg_sphere_frames_dev(n, lon_dev, lat_dev, c_dev, s_dev, frames_dev, hip_stream)
#   mpg_wind_vector_weights_dev(rh, src_frames_dev, dst_frames_dev, m_dev, hip_stream)
#   mpg_wind_vector_dev(rh, m_dev, u_dev, v_dev, src_type, u_level_stride, v_level_stride, nlev, r0_dev, r1_dev, dst_type, dst_layout,
#                       hip_stream)
_SPHERE_FRAMES_PROTO = C.CFUNCTYPE(C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_WIND_VECTOR_WEIGHTS_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_WIND_VECTOR_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_void_p,
                                 C.c_void_p, C.c_int, C.c_int, C.c_void_p)


def sphere_frames_dev(*args):
    """The typed binding of mpg_sphere_frames_dev; returns the call's status code."""
    if "frames" not in _to_mesh_fns:
        _to_mesh_fns["frames"] = _SPHERE_FRAMES_PROTO(("mpg_sphere_frames_dev", load()))
    return _to_mesh_fns["frames"](*args)


def wind_vector_weights_dev(*args):
    """The typed binding of mpg_wind_vector_weights_dev; returns the call's status code."""
    if "vector_weights" not in _to_mesh_fns:
        _to_mesh_fns["vector_weights"] = _WIND_VECTOR_WEIGHTS_PROTO(("mpg_wind_vector_weights_dev", load()))
    return _to_mesh_fns["vector_weights"](*args)


def wind_vector_dev(*args):
    """The typed binding of mpg_wind_vector_dev; returns the call's status code."""
    if "vector" not in _to_mesh_fns:
        _to_mesh_fns["vector"] = _WIND_VECTOR_PROTO(("mpg_wind_vector_dev", load()))
    return _to_mesh_fns["vector"](*args)


# The adjoint of the wind chain, bound the same way.
#   mpg_rotate_winds_transpose_dev(npts, nlev, cosa_dev, sina_dev, gu_dev, gv_dev, hip_stream)
#   mpg_wind_destagger_transpose_dev(rh_edge1, rh_edge2, cosa_dev, sina_dev, gu_dev, gv_dev, src_type, src_level_stride, nlev,
#                                    gumass_rot_dev, gvmass_rot_dev, gumass_dev, gvmass_dev, hip_stream)
_ROTATE_WINDS_TRANSPOSE_PROTO = C.CFUNCTYPE(C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_WIND_DESTAGGER_TRANSPOSE_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64,
                                              C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)


def rotate_winds_transpose_dev(*args):
    """The typed binding of mpg_rotate_winds_transpose_dev; returns the call's status code."""
    if "rotate_t" not in _to_mesh_fns:
        _to_mesh_fns["rotate_t"] = _ROTATE_WINDS_TRANSPOSE_PROTO(("mpg_rotate_winds_transpose_dev", load()))
    return _to_mesh_fns["rotate_t"](*args)


def wind_destagger_transpose_dev(*args):
    """The typed binding of mpg_wind_destagger_transpose_dev; returns the call's status code."""
    if "destagger_t" not in _to_mesh_fns:
        _to_mesh_fns["destagger_t"] = _WIND_DESTAGGER_TRANSPOSE_PROTO(("mpg_wind_destagger_transpose_dev", load()))
    return _to_mesh_fns["destagger_t"](*args)


# Winds from edge-normal u, bound the same way.
#   mpg_reconstruct_store(nCells, nEdges, maxEdges, nEdgesOnCell_host, edgesOnCell_host, out)
#   mpg_reconstruct_weights_dev(rh, maxEdges, coeffs_dev, dst_frames_dev, m_dev, hip_stream)
#   mpg_wind_reconstruct_dev(rh, m_dev, nout, u_dev, src_type, src_layout, u_level_stride, nlev, r0_dev, r1_dev, r2_dev, dst_type,
#                            dst_layout, hip_stream)
_RECONSTRUCT_STORE_PROTO = C.CFUNCTYPE(C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
_RECONSTRUCT_WEIGHTS_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_WIND_RECONSTRUCT_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p)


def reconstruct_store(*args):
    """The typed binding of mpg_reconstruct_store; returns the call's status code."""
    if "reconstruct_store" not in _to_mesh_fns:
        _to_mesh_fns["reconstruct_store"] = _RECONSTRUCT_STORE_PROTO(("mpg_reconstruct_store", load()))
    return _to_mesh_fns["reconstruct_store"](*args)


def reconstruct_weights_dev(*args):
    """The typed binding of mpg_reconstruct_weights_dev; returns the call's status code."""
    if "reconstruct_weights" not in _to_mesh_fns:
        _to_mesh_fns["reconstruct_weights"] = _RECONSTRUCT_WEIGHTS_PROTO(("mpg_reconstruct_weights_dev", load()))
    return _to_mesh_fns["reconstruct_weights"](*args)


def wind_reconstruct_dev(*args):
    """The typed binding of mpg_wind_reconstruct_dev; returns the call's status code."""
    if "wind_reconstruct" not in _to_mesh_fns:
        _to_mesh_fns["wind_reconstruct"] = _WIND_RECONSTRUCT_PROTO(("mpg_wind_reconstruct_dev", load()))
    return _to_mesh_fns["wind_reconstruct"](*args)


# Handle composition, bound the same way.
#   mpg_handle_compose(outer, inner, out)
#   mpg_compose_weights_dev(composed, outer, inner, nplanes, inner_m_dev, m_dev, hip_stream)
_HANDLE_COMPOSE_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
_COMPOSE_WEIGHTS_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)


def handle_compose(*args):
    """The typed binding of mpg_handle_compose; returns the call's status code."""
    if "handle_compose" not in _to_mesh_fns:
        _to_mesh_fns["handle_compose"] = _HANDLE_COMPOSE_PROTO(("mpg_handle_compose", load()))
    return _to_mesh_fns["handle_compose"](*args)


def compose_weights_dev(*args):
    """The typed binding of mpg_compose_weights_dev; returns the call's status code."""
    if "compose_weights" not in _to_mesh_fns:
        _to_mesh_fns["compose_weights"] = _COMPOSE_WEIGHTS_PROTO(("mpg_compose_weights_dev", load()))
    return _to_mesh_fns["compose_weights"](*args)


# Extrapolation, bound the same way.
#   mpg_handle_extrapolate(rh, src, dst, opts, out)
#   mpg_mesh_get_xyz(mesh, meshloc, xyz_host)
#   mpg_grid_get_xyz(grid, staggerloc, xyz_host)
class Points(C.Structure):
    """mpg_points of include/mpassit_amd.h: exactly one of mesh / grid is set."""
    _fields_ = [("mesh", C.c_void_p), ("meshloc", C.c_int), ("grid", C.c_void_p), ("staggerloc", C.c_int)]


class ExtrapOpts(C.Structure):
    """mpg_extrap_opts of include/mpassit_amd.h."""
    _fields_ = [("method", C.c_int), ("num_src_pnts", C.c_int), ("dist_exponent", C.c_double)]


_HANDLE_EXTRAPOLATE_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(Points), C.POINTER(Points), C.POINTER(ExtrapOpts), C.c_void_p)
_MESH_GET_XYZ_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p)
_GRID_GET_XYZ_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p)


def handle_extrapolate(*args):
    """The typed binding of mpg_handle_extrapolate; returns the call's status code."""
    if "handle_extrapolate" not in _to_mesh_fns:
        _to_mesh_fns["handle_extrapolate"] = _HANDLE_EXTRAPOLATE_PROTO(("mpg_handle_extrapolate", load()))
    return _to_mesh_fns["handle_extrapolate"](*args)


def mesh_get_xyz(*args):
    """The typed binding of mpg_mesh_get_xyz; returns the call's status code."""
    if "mesh_get_xyz" not in _to_mesh_fns:
        _to_mesh_fns["mesh_get_xyz"] = _MESH_GET_XYZ_PROTO(("mpg_mesh_get_xyz", load()))
    return _to_mesh_fns["mesh_get_xyz"](*args)


def grid_get_xyz(*args):
    """The typed binding of mpg_grid_get_xyz; returns the call's status code."""
    if "grid_get_xyz" not in _to_mesh_fns:
        _to_mesh_fns["grid_get_xyz"] = _GRID_GET_XYZ_PROTO(("mpg_grid_get_xyz", load()))
    return _to_mesh_fns["grid_get_xyz"](*args)


# Store-time masks, bound the same way.
#   mpg_handle_mask(rh, opts, out)
#   mpg_handle_extrapolate_masked(rh, src, dst, opts, src_mask_dev, dst_skip_dev, out)
class StoreMaskOpts(C.Structure):
    """mpg_store_mask_opts of include/mpassit_amd.h: device byte masks (0 / None = none), the rule and the Store's norm type."""
    _fields_ = [("src_mask_dev", C.c_void_p), ("dst_mask_dev", C.c_void_p), ("rule", C.c_int), ("norm_type", C.c_int)]


_HANDLE_MASK_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(StoreMaskOpts), C.c_void_p)
_HANDLE_EXTRAPOLATE_MASKED_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(Points), C.POINTER(Points), C.POINTER(ExtrapOpts), C.c_void_p,
                                               C.c_void_p, C.c_void_p)


def handle_mask(*args):
    """The typed binding of mpg_handle_mask; returns the call's status code."""
    if "handle_mask" not in _to_mesh_fns:
        _to_mesh_fns["handle_mask"] = _HANDLE_MASK_PROTO(("mpg_handle_mask", load()))
    return _to_mesh_fns["handle_mask"](*args)


def handle_extrapolate_masked(*args):
    """The typed binding of mpg_handle_extrapolate_masked; returns the call's status code."""
    if "handle_extrapolate_masked" not in _to_mesh_fns:
        _to_mesh_fns["handle_extrapolate_masked"] = _HANDLE_EXTRAPOLATE_MASKED_PROTO(("mpg_handle_extrapolate_masked", load()))
    return _to_mesh_fns["handle_extrapolate_masked"](*args)


# Nearest destination to source (include/mpassit_amd.h), bound the same way.
#   mpg_regrid_store_nearest_dtos(src, dst, norm, src_mask_dev, dst_mask_dev, out)
#   mpg_handle_get_src_nearest(rh, nearest_host)
_STORE_NEAREST_DTOS_PROTO = C.CFUNCTYPE(C.c_int, C.POINTER(Points), C.POINTER(Points), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
_HANDLE_GET_SRC_NEAREST_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)


def regrid_store_nearest_dtos(*args):
    """The typed binding of mpg_regrid_store_nearest_dtos; returns the call's status code."""
    if "store_nearest_dtos" not in _to_mesh_fns:
        _to_mesh_fns["store_nearest_dtos"] = _STORE_NEAREST_DTOS_PROTO(("mpg_regrid_store_nearest_dtos", load()))
    return _to_mesh_fns["store_nearest_dtos"](*args)


def handle_get_src_nearest(*args):
    """The typed binding of mpg_handle_get_src_nearest; returns the call's status code."""
    if "handle_get_src_nearest" not in _to_mesh_fns:
        _to_mesh_fns["handle_get_src_nearest"] = _HANDLE_GET_SRC_NEAREST_PROTO(("mpg_handle_get_src_nearest", load()))
    return _to_mesh_fns["handle_get_src_nearest"](*args)


# Patch regridding (include/mpassit_amd.h): a fixed bilinear handle turned into the CSR handle of second-degree patch recovery
#   mpg_handle_patch(rh, src, dst, out)
_HANDLE_PATCH_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(Points), C.POINTER(Points), C.c_void_p)


def handle_patch(*args):
    """The typed binding of mpg_handle_patch; returns the call's status code."""
    if "handle_patch" not in _to_mesh_fns:
        _to_mesh_fns["handle_patch"] = _HANDLE_PATCH_PROTO(("mpg_handle_patch", load()))
    return _to_mesh_fns["handle_patch"](*args)


# Second-order conservative regridding (include/mpassit_amd.h): a first-order conservative CSR handle turned into a second-order one
#   mpg_handle_conserve2nd(rh, src, dst, opts, out)
class Conserve2ndOpts(C.Structure):
    """mpg_conserve2nd_opts of include/mpassit_amd.h: the Store's norm type and a device byte mask of the sources (0 / None = none)."""
    _fields_ = [("norm_type", C.c_int), ("src_mask_dev", C.c_void_p)]


_HANDLE_CONSERVE2ND_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(Points), C.POINTER(Points), C.POINTER(Conserve2ndOpts), C.c_void_p)


def handle_conserve2nd(*args):
    """The typed binding of mpg_handle_conserve2nd; returns the call's status code."""
    if "handle_conserve2nd" not in _to_mesh_fns:
        _to_mesh_fns["handle_conserve2nd"] = _HANDLE_CONSERVE2ND_PROTO(("mpg_handle_conserve2nd", load()))
    return _to_mesh_fns["handle_conserve2nd"](*args)


# Creep-fill extrapolation (include/mpassit_amd.h): the unmapped rows of a handle filled level by level from their neighbours' rows
#   mpg_handle_creep(rh, dst, opts, out)
class CreepOpts(C.Structure):
    """mpg_creep_opts of include/mpassit_amd.h: the number of levels (>= 1, CREEP_ALL_LEVELS = all) and a device byte mask of the
    destination rows that are never filled and never a neighbour (0 / None = none)."""
    _fields_ = [("num_levels", C.c_int), ("dst_skip_dev", C.c_void_p)]


_HANDLE_CREEP_PROTO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(Points), C.POINTER(CreepOpts), C.c_void_p)


def handle_creep(*args):
    """The typed binding of mpg_handle_creep; returns the call's status code."""
    if "handle_creep" not in _to_mesh_fns:
        _to_mesh_fns["handle_creep"] = _HANDLE_CREEP_PROTO(("mpg_handle_creep", load()))
    return _to_mesh_fns["handle_creep"](*args)


_lib = None
_initialized = False


class MpgError(RuntimeError):
    def __init__(self, rc, msg):
        super().__init__("libmpassit_amd rc=%d: %s" % (rc, msg))
        self.rc = rc


def load():
    """dlopen the HIP library; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64; when torch shares the process it
        # must be loaded FIRST so that this library binds to the same runtime (two runtimes in one process
        # leave the second one without a device).  C / Fortran callers have no torch and use /opt/rocm's.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(SO_PATH):
            raise ImportError(
                "%s not found: build the HIP extension first (python -m mpassit_amd.build); "
                "mpassit_amd has no CPU fallback" % SO_PATH)
        L = C.CDLL(SO_PATH)
        L.mpg_last_error.restype = C.c_char_p
        L.mpg_comm_idfile_verdict.restype = C.c_char_p
        for name in SYMBOLS:
            if name not in ("mpg_last_error", "mpg_comm_idfile_verdict"):
                getattr(L, name).restype = C.c_int
        _lib = L
    return _lib


def check(rc):
    if rc != MPG_SUCCESS:
        raise MpgError(rc, load().mpg_last_error().decode("utf-8", "replace"))


def init(device=0):
    """ESMF_Initialize equivalent (mpassit.F90:84).  Requires a HIP device."""
    global _initialized
    check(load().mpg_init(C.c_int(device)))
    _initialized = True


def finalize():
    global _initialized
    if _lib is not None:
        check(_lib.mpg_finalize())
    _initialized = False


def device_info():
    buf = C.create_string_buffer(64)
    ncu, hbm = C.c_int(), C.c_int64()
    check(load().mpg_device_info(buf, C.c_int(64), C.byref(ncu), C.byref(hbm)))
    return buf.value.decode(), ncu.value, hbm.value


def tune(key, value):
    check(load().mpg_tune(key.encode(), C.c_int(int(value))))
