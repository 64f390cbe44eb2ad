/*
 * mpassit_amd.h -- C-ABI of the MI355X-native regrid engine that replaces the ESMF calls made by
 * LarissaReames-NOAA/MPASSIT's hot path (interp.F90 + the ESMF_Mesh/Grid objects of model_grid.F90).
 *
 * Every entry point replaces one ESMF verb at the cited reference call sites.
 * Conventions (mirroring the reference, utils.F90:16-33 / interp.F90:130-131):
 *   - every function returns an int rc, 0 == MPG_SUCCESS (like ESMF_SUCCESS); on failure
 *     mpg_last_error() returns a message; the caller decides to abort (the reference always does,
 *     error_handler -> mpi_abort(999)).
 *   - the caller owns all host buffers; the library owns device buffers and the opaque objects.
 *   - one process drives one GPU (one "PET" per GPU, mpassit.F90:84-96); calls are synchronous at the
 *     boundary unless the name ends in _dev and a stream is passed.
 *   - all floating point data is float64 (ESMF_TYPEKIND_R8 everywhere, interp.F90:479), indices int32.
 *   - there is NO CPU fallback: without a HIP device mpg_init fails and every other call returns
 *     MPG_ERR_NOT_INITIALIZED.
 */
#ifndef MPASSIT_AMD_H
#define MPASSIT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpg_mesh_s *mpg_mesh;     /* replaces type(ESMF_Mesh)        model_grid.F90:72  */
typedef struct mpg_grid_s *mpg_grid;     /* replaces type(ESMF_Grid)        model_grid.F90:73  */
typedef struct mpg_handle_s *mpg_handle; /* replaces type(ESMF_RouteHandle) interp.F90:86,192  */

enum {
  MPG_SUCCESS = 0,
  MPG_ERR_NOT_INITIALIZED = 1,
  MPG_ERR_INVALID_ARG = 2,
  MPG_ERR_HIP = 3,
  MPG_ERR_UNSUPPORTED = 4,
  MPG_ERR_OVERFLOW = 5,
  MPG_ERR_TIMEOUT = 6   /* a wait on another rank hit its deadline (mpg_comm_*): exit the process, do not retry in it */
};

/* ESMF_REGRIDMETHOD_* (interp.F90:119,204,370,420) */
enum { MPG_REGRIDMETHOD_BILINEAR = 0, MPG_REGRIDMETHOD_CONSERVE = 1, MPG_REGRIDMETHOD_NEAREST_STOD = 2 };
enum { MPG_REGRIDMETHOD_PATCH = 3 };   /* the method of mpg_handle_patch's handles; no Store takes it */
/* ESMF_MESHLOC_* (input_data.F90:927,1116-1123) */
enum { MPG_MESHLOC_ELEMENT = 0, MPG_MESHLOC_NODE = 1, MPG_MESHLOC_EDGE = 2 };   /* EDGE: a destination only, after mpg_mesh_set_edges */
/* ESMF_STAGGERLOC_* (interp.F90:480,489,509; model_grid.F90:706-728) */
enum { MPG_STAGGERLOC_CENTER = 0, MPG_STAGGERLOC_EDGE1 = 1, MPG_STAGGERLOC_EDGE2 = 2, MPG_STAGGERLOC_CORNER = 3 };
/* memory order of a source field with an ungridded (level) dimension */
enum {
  MPG_LAYOUT_CELL_FAST = 0, /* [nlev][ncell]: how the reference holds fields, input_data.F90:653-655 */
  MPG_LAYOUT_LEV_FAST = 1   /* [ncell][nlev]: MPAS file order, input_data.F90:630,645 (fused ingest) */
};

/* ---- runtime: ESMF_Initialize / ESMF_Finalize (mpassit.F90:84,140) ------------------------------ */
/* mpg_init may be repeated with the SAME device index (no-op); a different index while initialised is refused with
 * MPG_ERR_INVALID_ARG (streams and pinned staging belong to the first device): mpg_finalize first.
 * MPASSIT is a single-shot tool (mpassit.F90:105-137), so what a run pays are FIRST calls: mpg_init starts a helper thread that
 * loads the library's code objects and warms the runtime's pageable-copy staging while the caller goes on reading its
 * namelist and opening its files (the HIP runtime would otherwise load each translation unit at the first launch of one of
 * its kernels: 5-10 ms in front of the first Store of each method).  MPG_NO_WARMUP=1 in the environment switches it off. */
int mpg_init(int device);
/* Blocks until that helper thread is done (a few ms to a few hundred after mpg_init).  The thread allocates, frees and copies while it
 * runs, which a stream capture in hipStreamCaptureModeGlobal does not tolerate from another thread: a host that starts capturing
 * right after mpg_init calls this first (mpassit_amd/interp.py GraphedInterp does).  No-op when there is no such thread. */
int mpg_warmup_wait(void);
int mpg_finalize(void);
const char *mpg_last_error(void);
/* number of GPUs the process sees (0 when there is none); needs no mpg_init: a launcher's ranks choose their device with it */
int mpg_device_count(int *n);
/* "gfx950" etc.; buf may be NULL */
int mpg_device_info(char *arch_buf, int buf_len, int *n_cu, int64_t *hbm_bytes);

/* ---- ESMF_MeshCreate (model_grid.F90:488-497) ---------------------------------------------------
 * Arrays exactly as read from the MPAS file (model_grid.F90:354-417): lat/lon in RADIANS, the
 * deg conversion + (-180,180] wrap of :450-454,464-468 happens inside; verticesOnCell is
 * [nCells][maxEdges], 1-based, 0-padded (:448,479).  Elements = cells, nodes = vertices.
 * Refused with MPG_ERR_INVALID_ARG (and the offending index in mpg_last_error) before any geometry kernel runs: a vertex number
 * beyond nVertices, a coordinate that is NaN / Inf, a latitude beyond +-pi/2 (degrees handed over as radians). */
int mpg_mesh_create(int64_t nCells, int64_t nVertices, int maxEdges, const double *latCell,
                    const double *lonCell, const double *latVertex, const double *lonVertex,
                    const int32_t *verticesOnCell, mpg_mesh *out);
int mpg_mesh_destroy(mpg_mesh mesh); /* ESMF_MeshDestroy model_grid.F90:2154 */
/* The same for ONE rank of a job whose target rows are sharded over several GPUs: `grid` is this rank's row block (with the
 * halo rows it regrids itself), and only the part of the mesh that grid can see is brought to the device -- where the
 * reference hands every rank 1/N of the cells (para_range, model_grid.F90:423-438, 2428-2441) and ESMF redistributes.  The
 * host passes the same whole arrays; all cell CENTRES are uploaded (16 B per cell) and classified against the grid on the
 * device, then verticesOnCell, the vertex coordinates, the dual triangles and the nearest-neighbour BVH exist for the
 * covering id range of the cells within a margin of the grid only (spatially banded numbering makes that range tight;
 * arbitrary numbering degrades towards the whole mesh, never towards a wrong answer).  Ids stay GLOBAL: handles, source
 * ranges, windows and halo schedules are those of mpg_mesh_create, and every RegridStore of this mesh onto `grid` gives
 * bit-identical weights -- the window's closure is verified on the device and widened until it holds
 * (csrc/k_mesh_window.hip).  Stores onto any other grid are refused; `grid` must outlive the mesh's Stores.
 * mpg_mesh_window_info: the cell rows [cell_first, +cell_count) and vertices [vertex_first, +vertex_count) that are
 * resident, and the chord distance `margin` from the grid within which every cell is (any pointer may be NULL). */
int mpg_mesh_create_window(int64_t nCells, int64_t nVertices, int maxEdges, const double *latCell, const double *lonCell,
                           const double *latVertex, const double *lonVertex, const int32_t *verticesOnCell, mpg_grid grid, mpg_mesh *out);
int mpg_mesh_window_info(mpg_mesh mesh, int64_t *cell_first, int64_t *cell_count, int64_t *vertex_first, int64_t *vertex_count, double *margin);
/* The mesh's EDGES (MPG_MESHLOC_EDGE): the points that carry MPAS's prognostic wind `u`, the component normal to each cell edge.  Host
 * arrays as the MPAS file holds them, in radians: latEdge, lonEdge [nEdges] and angleEdge [nEdges], the angle of the edge's normal
 * from local east.  The coordinates go through the SAME conversion as the cell centres in mpg_mesh_create (degrees, the (-180, 180]
 * wrap, unit vectors): an edge given a cell centre's latitude and longitude gets that centre's unit vector bit for bit.  angleEdge is
 * kept on the device as given; it may be NULL, and mpg_mesh_edge_rotang_dev is then refused.  Edges are a DESTINATION location only:
 * mpg_regrid_store_to_mesh(..., MPG_MESHLOC_EDGE, ...) is their Store; every call that takes a source location, the other Stores onto
 * a mesh and mpg_mesh_rotang_dev go on refusing location 2.  The edge arrays are freed with the mesh.
 * Refusals.  MPG_ERR_INVALID_ARG, with the offending index in mpg_last_error: a NaN / Inf coordinate or angle, |lat| > pi/2; nEdges < 1;
 * NULL mesh or coordinates; a second call on the same mesh ("edges are already set": handles onto the edges, cached ones included,
 * stay valid that way).  MPG_ERR_OVERFLOW: nEdges beyond int32.  MPG_ERR_UNSUPPORTED: a mesh of mpg_mesh_create_window. */
int mpg_mesh_set_edges(mpg_mesh mesh, int64_t nEdges, const double *latEdge, const double *lonEdge, const double *angleEdge);
/* the number of edges mpg_mesh_set_edges gave the mesh; 0 for a mesh without edges */
int mpg_mesh_edge_count(mpg_mesh mesh, int64_t *nEdges);

/* ---- ESMF_GridCreateNoPeriDim / 1PeriDim + GridAddCoord x4 (model_grid.F90:684-728,736-1038) ------
 * nx, ny = mass (CENTER) point counts (i_target, j_target).  Coordinates in DEGREES, C order with i
 * fastest: centre [ny][nx], corner [ny+1][nx+1], EDGE1 (U) [ny][nx+1], EDGE2 (V) [ny+1][nx].
 * corner/edge arrays may be NULL when the corresponding stagger is never used.
 * periodic_i = 0: ESMF_GridCreateNoPeriDim (regional, model_grid.F90:699).
 * periodic_i = MPG_GRID_PERIODIC_I (1): ESMF_GridCreate1PeriDim(periodicDim=1, poleDim=2, MONOPOLE at both
 *   ends, model_grid.F90:685-694): CENTER column nx-1 neighbours column 0, and each j end is closed by a pole
 *   node at lat -/+90 whose value is the mean of the first / last CENTER row.  Array shapes are the same as
 *   in the regional case; the extra EDGE1 / CORNER column (index nx) duplicates column 0 one period later
 *   (ESMF's periodic staggers hold only the first nx columns).  Only Grid -> Grid RegridStore reads the flag.
 * OR in MPG_GRID_NO_SOUTH_POLE / MPG_GRID_NO_NORTH_POLE for a row block of a periodic grid that does not
 *   touch that pole (multi-GPU row sharding).  The two flags name an END of the row range, not a hemisphere: NO_SOUTH_POLE means
 *   "rows precede row 0", NO_NORTH_POLE "rows follow row ny - 1" -- on rows numbered south to north, which is how a row block is cut
 *   and the only numbering the Grid -> Grid RegridStore serves (it places its caps by row number and refuses a periodic grid whose
 *   rows are numbered north to south with MPG_ERR_UNSUPPORTED: reverse the rows).  mpg_regrid_store_periodic_to_mesh takes either
 *   numbering and finds each end's pole from the end row itself.
 * A coordinate that is NaN / Inf (or |lat| > 180) is refused with MPG_ERR_INVALID_ARG and the point's index; latitudes a little beyond
 * the pole (the corner row of a global lat-lon grid) are angles and pass. */
enum { MPG_GRID_PERIODIC_I = 1, MPG_GRID_NO_SOUTH_POLE = 2, MPG_GRID_NO_NORTH_POLE = 4 };
int mpg_grid_create(int nx, int ny, int periodic_i, const double *lon_center, const double *lat_center,
                    const double *lon_corner, const double *lat_corner, const double *lon_edge1,
                    const double *lat_edge1, const double *lon_edge2, const double *lat_edge2,
                    mpg_grid *out);
int mpg_grid_destroy(mpg_grid grid); /* ESMF_GridDestroy model_grid.F90:2156 */

/* ---- target grid straight from the projection, on the device -------------------------
 * Replaces the host loops of define_target_grid_params (model_grid.F90:736-1038): get_lat_lon_fields x4 staggers
 * (:2188-2219 -> xytoll, llxy_module.F90:166-216 -> ij_to_latlon, module_map_utils.F90:629-679, Lambert :1160-1233,
 * lat-lon :1398-1428), get_rotang (:2450-2507) and get_map_factor (:2229-2365).  The fields of mpg_proj are the
 * arguments of push_source_projection / map_set (model_grid.F90:676-678); the derived constants (cone, rsw, pole
 * i/j; set_lc, module_map_utils.F90:1083-1121) are computed inside.  nx, ny = mass point counts (i_target,
 * j_target); stagger shapes as in mpg_grid_create.  The grid keeps lon/lat (degrees), cos/sin(alpha) and the map
 * factors on the device; the getters copy them to the host (XLAT/XLONG/MAPFAC/SINALPHA/COSALPHA of the output file,
 * write_data.F90:1003-1140).
 * PROJ_PS (polar stereographic: truelat1, stand_lon, dx_m; set_ps / ijll_ps, module_map_utils.F90:682-822) and PROJ_MERC
 * (Mercator: truelat1, dx_m; set_merc / ijll_merc, :1293-1362) take the arguments push_source_projection passes for them
 * (llxy_module.F90:71-79,123-132).
 * Map factors: PROJ_LC / PROJ_PS / PROJ_MERC as get_map_factor; PROJ_LATLON has no branch there (the reference writes unset memory) and
 * returns 1.0 here.  cos/sin(alpha) exist for PROJ_LC only (model_grid.F90:1113), as in the reference. */
enum { MPG_PROJ_LATLON = 0, MPG_PROJ_LC = 1, MPG_PROJ_PS = 2, MPG_PROJ_MERC = 3 }; /* misc_definitions_module.F90:38-42 */
typedef struct mpg_proj {
  int code;
  double known_lat, known_lon, known_x, known_y; /* lat1, lon1, knowni, knownj */
  double dx_m;                                   /* PROJ_LC, PROJ_PS, PROJ_MERC: grid spacing in metres */
  double stand_lon, truelat1, truelat2;          /* PROJ_LC; PROJ_PS: stand_lon, truelat1; PROJ_MERC: truelat1 */
  double dlat_deg, dlon_deg;                     /* PROJ_LATLON: latinc, loninc */
} mpg_proj;
int mpg_grid_create_proj(const mpg_proj *proj, int nx, int ny, int periodic_i, mpg_grid *out);
/* A grid made from coordinate ARRAYS (mpg_grid_create) whose arrays are rows row0 .. row0 + ny - 1 of the grid `proj` describes
 * (a rank's block of target rows, model_grid.F90:693): the Stores of Mesh -> Grid handles then find a source triangle's /
 * cell's target points through the inverse projection in O(1) instead of descending the box pyramid (PROJ_LC and PROJ_LATLON;
 * other projections are accepted and change nothing).  Every candidate is still tested exactly as before: the weights are
 * those of the pyramid search.  The claim is checked -- a sample of the grid's own CENTER points must fall on their own
 * indices -- and a projection that does not fit is refused with MPG_ERR_INVALID_ARG.  Grids of mpg_grid_create_proj have
 * their inverse from the start. */
int mpg_grid_attach_proj(mpg_grid grid, const mpg_proj *proj, int row0);
int mpg_grid_get_coords(mpg_grid grid, int staggerloc, double *lon_host, double *lat_host);
int mpg_grid_get_rotang(mpg_grid grid, double *cosa_host, double *sina_host);
int mpg_grid_get_mapfac(mpg_grid grid, int staggerloc, double *mapfac_host);
/* device pointers owned by the grid ([ny][nx], CENTER), for mpg_rotate_winds_dev */
int mpg_grid_rotang_dev(mpg_grid grid, const double **cosa_dev, const double **sina_dev);

/* ---- ESMF_Field[Bundle]RegridStore (interp.F90:123,207,226,241,259,277,334,353,372,394,421,437) ---
 * srcTermProcessing=1, unmappedaction=IGNORE are implied.  Mesh -> Grid.  Handles are cached: the same
 * (mesh, src_loc, grid, dst_stagger, method) returns the same handle (reference recomputes it up to
 * 13x per run); each Store must be paired with one mpg_handle_release.  A handle whose last reference
 * was released keeps its weights in the cache (up to 8 such handles; dropped when their mesh or grid is destroyed or
 * at mpg_finalize), so the Store / Regrid / Release / Store-again sequence of interp_diag_data followed by
 * interp_hist_data (interp.F90:123-148, :207) builds the element -> CENTER bilinear weights once. */
int mpg_regrid_store(mpg_mesh src, int src_meshloc, mpg_grid dst, int dst_staggerloc, int regridmethod,
                     mpg_handle *out);
/* Grid -> Grid on the same grid, CENTER -> EDGE1/EDGE2 bilinear (interp.F90:298,316).  Everything else between two grids -- any stagger
 * onto any stagger, nearest, periodic sources, conservative -- is mpg_regrid_store_grid_to_grid / mpg_regrid_store_conserve_grid_to_grid. */
int mpg_regrid_store_grid(mpg_grid grid, int src_staggerloc, int dst_staggerloc, int regridmethod,
                          mpg_handle *out);
/* Grid -> Mesh: ESMF_FieldRegridStore(srcField on a Grid stagger, dstField on a Mesh location) -- the call that regrids BACK: a gridded
 * analysis, a grid-space increment or a model's output on the structured grid interpolated onto the MPAS cells.  (The transpose
 * Regrid below is the adjoint of a Mesh -> Grid handle and does not regrid back; this Store builds the interpolation itself.)
 * Source points: the grid's points of src_staggerloc, snx x sny of them (CENTER nx x ny, EDGE1 (nx+1) x ny, EDGE2 nx x (ny+1), CORNER
 *   (nx+1) x (ny+1)), source index = j * snx + i; any stagger whose coordinates the grid holds (a stagger without coordinates ->
 *   MPG_ERR_INVALID_ARG).  Destinations: the mesh's cell centres (MPG_MESHLOC_ELEMENT), vertices (MPG_MESHLOC_NODE) or -- on a mesh
 *   that mpg_mesh_set_edges gave edges -- its edge points (MPG_MESHLOC_EDGE; same search, same weights, nothing but the point set
 *   differs; a mesh without edges -> MPG_ERR_INVALID_ARG).  The handle is
 *   an ordinary fixed one (MPG_KIND_FIXED), nnz_per_row 4 (bilinear) or 1 (nearest); mpg_handle_info reports n_src = snx * sny,
 *   n_dst = nx_dst = the mesh count, ny_dst = 1.
 * MPG_REGRIDMETHOD_BILINEAR: source cells are the quads of four neighbouring stagger points A = (b, a), B = (b, a+1), C = (b+1, a+1),
 *   D = (b+1, a).  A mesh point belongs to the quad with the lowest quad id b * (snx - 1) + a for which the bilinear map X(xi, eta) = t * P
 *   has a solution on the point's side of the sphere with xi, eta in [-tol, 1 + tol]; tol = 10^-grid_inside_tol_exp (mpg_tune; default
 *   1e-10, the Grid -> Grid Store's).  Slots and weights are the Grid -> Grid Store's: A, B, C, D with (1-xi)(1-eta), xi (1-eta), xi eta,
 *   (1-xi) eta.  A point in no quad is unmapped: idx -1, weights 0, Regrid gives 0.0 (mpg_regrid_masked_dev: fill_value).
 *   Candidate search, two routes with identical results: on a grid with a usable inverse projection (mpg_grid_create_proj,
 *   mpg_grid_attach_proj) the quads around the point's own (i, j), within the pad of the other Stores' index boxes; where the inverse
 *   gives no index, and on every other grid, a descent of a box pyramid over the stagger's quads that tests every leaf quad whose box
 *   holds the point.  mpg_tune("store_boxes", 0) selects the pyramid everywhere; mpg_handle_store_path reports 1 (index space) or 0.
 * MPG_REGRIDMETHOD_NEAREST_STOD: the stagger point at the smallest chord distance, the lowest source index on ties; every mesh point
 *   is mapped.  A pyramid descent, seeded from the inverse projection where there is one.
 * Refusals.  MPG_ERR_UNSUPPORTED: MPG_REGRIDMETHOD_CONSERVE; bilinear on a grid created with MPG_GRID_PERIODIC_I (pole caps and the i-wrap
 *   towards a mesh are not built into THIS call: mpg_regrid_store_periodic_to_mesh below is the bilinear Store of such a grid, with its
 *   pole method argument; nearest on such a grid is accepted); a mesh of mpg_mesh_create_window (its resident cells are a window:
 *   the result would be a partial mesh).  MPG_ERR_OVERFLOW: snx * sny or the mesh count beyond int32.  MPG_ERR_INVALID_ARG: NULL
 *   objects, unknown enums.
 * Cached like every Store -- the key carries the direction, so (mesh, loc, grid, stagger, method) of the two directions never collide --
 *   and paired with one mpg_handle_release; parked entries go when their mesh or grid is destroyed.  mpg_mesh_set_source_window passes
 *   these handles by: the mesh is their destination, their sources are grid points.  There is no _begin variant.
 * Everything that takes a fixed handle takes this one: mpg_regrid_dev / _typed[_pitched]_dev / _bundle_typed_dev give [nlev][n_dst] (the
 *   source layout MPG_LAYOUT_CELL_FAST is the grid's [lev][plane]), mpg_regrid_masked_dev fills mesh points outside the grid and skips
 *   missing grid values, mpg_regrid_transpose_dev is then the Mesh -> Grid adjoint, and the weight getters, mpg_handle_unique_sources,
 *   _localize and _rebase work.  mpg_regrid_to_mesh_dev below adds the mesh's own memory order.  The conservative method has a
 *   Store of its own, with its normalisation argument: mpg_regrid_store_conserve_to_mesh. */
int mpg_regrid_store_to_mesh(mpg_grid src, int src_staggerloc, mpg_mesh dst, int dst_meshloc, int regridmethod, mpg_handle *out);
/* Periodic Grid -> Mesh: ESMF_FieldRegridStore(srcField on the CENTER stagger of a Grid of ESMF_GridCreate1PeriDim with MONOPOLE caps,
 * dstField on a Mesh location, regridmethod=BILINEAR, polemethod=) -- a global lat-lon analysis (GFS, ERA5, an SST product) taken onto MPAS
 * cells by the default method.  The grid must have been created with MPG_GRID_PERIODIC_I.
 * Source points: the grid's nx x ny CENTER points, source index = j * nx + i.  Destinations: the mesh's cell centres (MPG_MESHLOC_ELEMENT)
 *   or vertices (MPG_MESHLOC_NODE), or the edges mpg_mesh_set_edges gave it (MPG_MESHLOC_EDGE; none set -> MPG_ERR_INVALID_ARG).
 * Quads: b in [0, ny - 2], a in [0, nx - 1]; A = (b, a), B = (b, (a + 1) mod nx), C = (b + 1, (a + 1) mod nx), D = (b + 1, a);
 *   quad id = b * nx + a.  A point belongs to the lowest quad id for which the bilinear map of mpg_regrid_store_to_mesh has a solution
 *   with xi, eta in [-tol, 1 + tol], tol = 10^-grid_inside_tol_exp; weights (1-xi)(1-eta), xi (1-eta), xi eta, (1-xi) eta on A, B, C, D.
 *   It is that call's per-quad code: for a quad with a < nx - 1 the four weights are the bits mpg_regrid_store_to_mesh produces for the
 *   same coordinates handed over as a non-periodic grid; the seam quads a = nx - 1 are what that call cannot reach.
 * Pole caps are tried only when no quad passed, under MPG_POLEMETHOD_ALLAVG (ESMF_POLEMETHOD_ALLAVG, ESMF's default).  Each end row
 *   is closed by a fan of nx triangles onto a pole node, and the node sits where the end row's own points say, not where the row number
 *   says: the pole of an end is (0, 0, sign of the mean z of that end's CENTER row).  Rows numbered south to north (this project's
 *   lat-lon grids) have the south pole at row 0; rows numbered north to south (GRIB, ERA5, the IFS and JRA-55 Gaussian grids) have the
 *   north pole there, and both give the interpolation of the same physical grid.  With A = (row, a), B = (row, (a + 1) mod nx) the
 *   triangle is (A, B, N) at the north pole and (B, A, S) at the south pole -- counter-clockwise seen from outside, the triangles of the
 *   Grid -> Grid Store -- with planar barycentric weights seen from the sphere's centre, tolerance 1e-10 whatever grid_inside_tol_exp
 *   says.  Cap ids run 0 .. nx - 1 for the row-0 end, then nx .. 2 nx - 1 for the row-(ny - 1) end; the lowest passing id wins.  The pole
 *   node's value is the mean of its CENTER row, so a cap row has nx entries: every column of the row gets wr = t_pole / nx, columns A
 *   and B get t_A + wr and t_B + wr.  An end row that sits on its pole leaves no point to a cap.
 *   MPG_GRID_NO_SOUTH_POLE drops the cap of the row-0 end and MPG_GRID_NO_NORTH_POLE that of the row-(ny - 1) end, whichever pole that
 *   end closes on: they describe a row block.  Two live ends whose rows lie in the same hemisphere are refused (at most one of them
 *   closes on a pole).  MPG_POLEMETHOD_NONE (ESMF_POLEMETHOD_NONE): no caps.
 *   A point with no quad and no cap gets an empty row: Regrid gives 0.0 (mpg_regrid_masked_dev: fill_value).
 *   ESMF's NPNTAVG and TEETH pole methods are not built.  Other source staggers are not built either: the EDGE / CORNER columns of a
 *   periodic grid duplicate column 0, and their end rows sit on or beyond the poles.
 * The handle is an ordinary CSR one (nnz_per_row 0, method bilinear) with no pole terms (mpg_handle_pole_count gives 0) and
 *   no dst fraction: mpg_handle_info reports n_src = nx * ny, n_dst = nx_dst = the mesh count, ny_dst = 1.  A quad row has
 *   exactly 4 entries, zeros included, a cap row exactly nx -- ESMF's factor list for the row, row_len entries of w_pole / row_len;
 *   columns ascend within a row.
 *   No atomic decides a stored byte: two Stores on fresh objects give identical rowptr / col / val.
 *   Candidate search, two routes with identical results: on a lat-lon grid that closes the circle, with its projection attached
 *   (mpg_grid_create_proj, mpg_grid_attach_proj) and cells whose parallels leave their row by at most 0.04 index units, the quads around
 *   the point's own (i, j), a taken mod nx; where the inverse gives no index (poleward of 85 degrees), and on every other grid, a walk of a
 *   box pyramid over the nx x (ny - 1) quads, the seam column included.  mpg_tune("store_boxes", 0) selects the walk everywhere;
 *   mpg_handle_store_path reports 1 (index space) or 0.  Cap candidates are found the same way on both routes: the points no quad took
 *   are compacted into a list and only those are tested against the nx triangles of each live end.
 * Refusals, each with a message that names the way out.  MPG_ERR_INVALID_ARG: NULL arguments; an unknown dst_meshloc or pole_method;
 *   nx < 3 or ny < 2; under ALLAVG, rows 0 and ny - 1 in one hemisphere with neither MPG_GRID_NO_SOUTH_POLE nor MPG_GRID_NO_NORTH_POLE
 *   set.  MPG_ERR_UNSUPPORTED: a grid without MPG_GRID_PERIODIC_I (mpg_regrid_store_to_mesh is its Store); a mesh of
 *   mpg_mesh_create_window.  MPG_ERR_OVERFLOW: nx * ny or the mesh count beyond int32; nnz >= 2^31.
 * Cached like every Store and paired with one mpg_handle_release: the key carries the direction bit, a kind bit of its own and
 *   pole_method, so it collides with no Grid -> Mesh, conservative or Mesh -> Grid key and the two pole methods are two handles; parked
 *   entries go when the mesh or the grid is destroyed.  mpg_mesh_set_source_window passes these handles by.  There is no _begin variant.
 * mpg_handle_store_ms is filled; mpg_handle_store_stats: [1] points that had an index and still took the walk, [2] points in all,
 *   [3] points mapped by a cap, [4] points mapped by a seam quad (a = nx - 1).
 * Everything that takes a CSR handle takes this one, with no kernel of its own: mpg_regrid_csr_to_mesh_dev in both mesh orders,
 *   mpg_regrid_csr_rows_dev, mpg_regrid_typed[_pitched]_dev, mpg_regrid_masked_dev, mpg_regrid_transpose_dev, mpg_handle_get_csr.
 *   mpg_regrid_to_mesh_dev and mpg_regrid_rows_dev refuse it as they refuse every CSR handle.  Winds: mpg_wind_csr_to_mesh_dev. */
enum { MPG_POLEMETHOD_NONE = 0, MPG_POLEMETHOD_ALLAVG = 1 };
int mpg_regrid_store_periodic_to_mesh(mpg_grid src, mpg_mesh dst, int dst_meshloc, int pole_method, mpg_handle *out);
/* Mesh -> Mesh: ESMF_FieldRegridStore(srcField on a Mesh's elements, dstField on another Mesh's location) -- a global run feeding the
 * boundary and initial fields of a limited-area mesh, a 15-km state moved onto a 3-km or variable-resolution mesh, a restart remapped
 * after re-meshing -- in ONE interpolation instead of two hops through an intermediate grid.
 * Source points: the source mesh's cell centres (src_meshloc = MPG_MESHLOC_ELEMENT), source index = cell id.  Destinations: the
 *   destination mesh's cell centres (dst_meshloc = MPG_MESHLOC_ELEMENT) or vertices (MPG_MESHLOC_NODE).  The handle is an ordinary fixed
 *   one (MPG_KIND_FIXED), nnz_per_row 3 (bilinear) or 1 (nearest); mpg_handle_info reports n_src = the source mesh's nCells, n_dst =
 *   nx_dst = the destination count, ny_dst = 1 (the Grid -> Mesh convention).
 * MPG_REGRIDMETHOD_BILINEAR: source cells are the source mesh's dual (Delaunay) triangles (mpg_mesh_get_triangles).  A destination point
 *   belongs to the triangle with the lowest triangle id (= vertex id) for which the line type's weight function passes with the
 *   tolerance 1e-10 -- mpg_tune("bilinear_linetype", 0): the ray from the sphere's centre; 1: along the triangle's normal.  Slots are
 *   the triangle's cells in the stored order of mpg_mesh_get_triangles, weights dA / S, dB / S, dC / S.  A point in no triangle is
 *   unmapped: idx -1, weights 0, Regrid gives 0.0 (mpg_regrid_masked_dev: fill_value) -- the points outside a regional source mesh and
 *   the rim strip outside its outermost cell centres.  The result depends on the two meshes and the knob only: the search is a box
 *   tree over the source mesh's triangles (built at the first such Store of a source mesh and kept on it) whose boxes remove no
 *   triangle that would pass, and every passing triangle is compared by id.
 * MPG_REGRIDMETHOD_NEAREST_STOD: the source cell centre at the smallest chord distance, the lowest cell id on ties; every destination
 *   point is mapped.  The exact search of the Mesh -> Grid Store over the source mesh's site tree; the grid's index bins are not used.
 * Refusals, each with a message that names the way out.  MPG_ERR_UNSUPPORTED: MPG_REGRIDMETHOD_CONSERVE (Voronoi cell against Voronoi
 *   cell is not built here: the conservative Mesh -> Mesh Store is a call of its own, with its normalisation argument:
 *   mpg_regrid_store_conserve_mesh); src_meshloc = MPG_MESHLOC_NODE; either mesh made by mpg_mesh_create_window.  MPG_ERR_OVERFLOW: counts beyond
 *   int32.  MPG_ERR_INVALID_ARG: NULL objects, unknown enums.  src == dst is allowed (every point then sits on a triangle corner: one
 *   weight 1.0 on its own cell).
 * Cached like every Store and paired with one mpg_handle_release.  The key carries a kind bit of its own, so it collides with neither a
 *   Mesh -> Grid nor a Grid -> Mesh key, and for bilinear the line type; parked entries go when EITHER mesh is destroyed.
 *   mpg_mesh_set_source_window on the SOURCE mesh applies to these handles as it does to Mesh -> Grid handles (their sources are that
 *   mesh's cells); a window on the destination mesh does not touch them.  There is no _begin variant.
 * mpg_handle_store_ms is filled; mpg_handle_store_stats: [2] points in all, [3] microseconds this Store spent building the source
 *   mesh's triangle tree (0 when the mesh had it already).
 * Everything that takes a fixed handle takes this one unchanged: mpg_regrid_dev / _typed[_pitched]_dev / _bundle_typed_dev,
 *   mpg_regrid_masked_dev, mpg_regrid_transpose_dev, mpg_regrid_to_mesh_dev, the weight getters, mpg_handle_unique_sources, _localize and
 *   _rebase.  mpg_regrid_rows_dev below reads and writes MPAS file order. */
int mpg_regrid_store_mesh(mpg_mesh src, int src_meshloc, mpg_mesh dst, int dst_meshloc, int regridmethod, mpg_handle *out);
/* The same two Stores STARTED and not waited for.  interp.F90:207-437 stores its weight sets one after the other, each in front of
 * the Regrids that use it; they are independent of each other and of every Regrid that does not use them.  A _begin call queues
 * the Store on the library's worker thread (own stream, one Store at a time) and returns; the matching mpg_regrid_store[_grid]
 * -- same arguments -- later returns the finished handle, waiting only for what is left of it.  A host that begins its
 * conservative, nearest-neighbour and destaggering Stores before it regrids its bilinear fields hides them behind those Regrids
 * (bench.py `job` leg).  Weights, cache and reference counting are those of the plain calls; a Store that nobody collects stays
 * a parked cache entry.  Errors of a begun Store surface in the collecting call. */
int mpg_regrid_store_begin(mpg_mesh src, int src_meshloc, mpg_grid dst, int dst_staggerloc, int regridmethod);
int mpg_regrid_store_grid_begin(mpg_grid grid, int src_staggerloc, int dst_staggerloc, int regridmethod);

/* ---- ESMF_Field[Bundle]Regrid (interp.F90:134,219,236,251,268,286,307,325,344,363,382,404,431,443) --
 * dst is fully overwritten: [nfields][nlev][ny_dst][nx_dst], unmapped points = 0.0 (zeroregion=TOTAL).
 * src: nfields slabs of nlev*n_src doubles in `src_layout` order.  Host-pointer version copies
 * H2D/D2H internally; the _dev version takes device pointers and a hipStream_t (NULL = default
 * stream) and returns after enqueueing.  The first _dev call on a handle for a given layout decides the kernel and
 * may build its tile lists (allocation + synchronisation); every later call only enqueues kernels on the stream, so a
 * caller can capture its per-time-level sequence of _dev calls (Regrid, rotate_winds, post-ops) into a hipGraph. */
int mpg_regrid(mpg_handle rh, const double *src_host, int src_layout, int nlev, int nfields, double *dst_host);
int mpg_regrid_dev(mpg_handle rh, const double *src_dev, int src_layout, int nlev, int nfields,
                   double *dst_dev, void *hip_stream);
/* Pitched destinations.  The dense block above puts level k of a field k * ny_dst * nx_dst elements after level 0, which starts on
 * a 128-byte line only when the plane is a multiple of 32 (float32) / 16 (float64) points -- on most grids (1799 x 1059, every
 * stagger of 1800 x 1060) each plane starts partway into a line and its stores pay for the partial lines at both ends.  A host that
 * owns its result arrays can instead lay the planes out dst_level_stride ELEMENTS apart: plane k of field f starts at
 * (f * nlev + k) * dst_level_stride; elements [ny_dst * nx_dst, dst_level_stride) of each plane are never written.
 * mpg_dst_level_stride gives the smallest stride >= plane_points at which every plane of dst_type starts on a 128-byte line (with a
 * base pointer that does, as hipMalloc's do): pure arithmetic, callable before mpg_init.  On such planes the kernels' stores are
 * whole-line non-temporal stores whatever the grid.
 * Every _pitched_dev call takes the arguments of its dense twin plus dst_level_stride: 0 = dense (the dense twin is exactly that
 * call), a stride below the plane size -> MPG_ERR_INVALID_ARG.  Same kernels, same bits per plane, and capturable in a hipGraph
 * like the dense calls. */
int mpg_dst_level_stride(int64_t plane_points, int dst_type, int64_t *ld);
int mpg_regrid_pitched_dev(mpg_handle rh, const double *src_dev, int src_layout, int nlev, int nfields, double *dst_dev,
                           int64_t dst_level_stride, void *hip_stream);
/* Fused ingest/egress Regrid (the callers either side of the hot path): the source may be
 * float32 (MPAS history variables are single precision; the reference widens them at read, input_data.F90:630-655)
 * and the destination float32 (every output variable is NF90_FLOAT, write_data.F90:779).  The arithmetic stays
 * float64 and  dst = (dst type) fma(regrid(src), scale, offset)  reproduces the writer's post-ops (T - 300,
 * write_data.F90:1343; PHB * 9.81, :1418), so float32 results are bit-identical to the reference's file contents.
 * src_type / dst_type: MPG_TYPE_F64 or MPG_TYPE_F32, optionally | MPG_TYPE_BE: the values are big-endian in memory, as a
 * NetCDF classic (CDF-1/2/5) variable stores them -- the bytes of nf90_get_var's source (input_data.F90:630) and of
 * nf90_put_var's destination (write_data.F90:1339-1475) travel file <-> HBM untouched (mpg_file_to_dev / mpg_dev_to_file)
 * and the Regrid reads / writes them as they are: no byte-swap pass over the data exists.
 * The sum itself, a contract by identity for every call that applies a handle: a fixed handle's slots in stored order -- one slot (nearest)
 * is a copy of the source value, three slots (w0, a), (w1, b), (w2, e) give fma(w2, e, fma(w1, b, w0 * a)), four give the chain
 * acc = fma(w[q], src[idx[q]], acc) from 0.0 -- and +0.0 for an unmapped point; a CSR row is that chain over its entries in stored order,
 * +0.0 when empty.  mpg_regrid_dev stores the sum as it stands (a -0.0 stays -0.0); every typed call stores (dst type) fma(sum, scale, offset),
 * unmapped points included.
 * Device pointers, stream as in mpg_regrid_dev. */
enum { MPG_TYPE_F64 = 0, MPG_TYPE_F32 = 1, MPG_TYPE_BE = 2 };
int mpg_regrid_typed_dev(mpg_handle rh, const void *src_dev, int src_type, int src_layout, int nlev, int nfields,
                         void *dst_dev, int dst_type, double scale, double offset, void *hip_stream);
/* ... with the destination's level planes dst_level_stride elements apart (mpg_regrid_pitched_dev) */
int mpg_regrid_typed_pitched_dev(mpg_handle rh, const void *src_dev, int src_type, int src_layout, int nlev, int nfields, void *dst_dev,
                                 int dst_type, double scale, double offset, int64_t dst_level_stride, void *hip_stream);
/* Transpose Regrid: ESMF_FieldRegridStore(..., transposeRoutehandle=) applied with ESMF_FieldRegrid, mesh_out = A^T grid_in.
 * A is exactly the operator the forward Regrid of this handle applies: every stored entry with idx >= 0 (weight 1 for nearest
 * neighbour), every CSR entry (mpg_handle_from_weights duplicates included) and the pole caps of a periodic Grid -> Grid handle,
 * whose forward adds w_pole * mean(row): the transpose adds (sum_q w_pole[q] * g[pole_dst[q]]) / row_len to every source of that
 * row.  It is the ADJOINT of the Regrid, not an inverse (A^T A != I): it does not "regrid back" (mpg_regrid_store_to_mesh does).
 * src_dev: grid values [nfields][nlev][plane], plane = n_dst of mpg_handle_info, planes src_level_stride elements apart (0 = dense;
 * below n_dst -> MPG_ERR_INVALID_ARG); a pitched result of the *_pitched_dev calls can be fed back as it is, its pad is never read.
 * dst_dev: nfields slabs of nlev * n_src in dst_layout (MPG_LAYOUT_CELL_FAST [lev][cell], MPG_LAYOUT_LEV_FAST [cell][lev]), n_src
 * the handle's current index space (the window count after mpg_mesh_set_source_window, the local extent after mpg_handle_localize /
 * rebase).  dst is fully overwritten; a source no entry references gets exactly 0.0 (zeroregion=TOTAL).
 * Types: MPG_TYPE_F64 / MPG_TYPE_F32 on either side, float64 arithmetic, float32 rounded once at the store; MPG_TYPE_BE ->
 * MPG_ERR_UNSUPPORTED.  The linear part only: no scale / offset (the transpose of an affine epilogue is not defined).
 * Values, a contract by identity, per (source c, level k):
 *   acc = fma(w_j, (double)g[k][row_j], acc) from +0.0 over the stored entries j that reference c, in ascending (destination point,
 *   slot) order -- for a CSR handle ascending CSR position, duplicates each in their place; w_j of a nearest-neighbour handle is 1.0;
 *   dst = (dst type)acc, one rounding; a source no entry references gets +0.0.
 *   With pole caps the sources of the two CENTER rows get (dst type)(acc + term / row_len), the pole term last, where term is reduced in
 *   a fixed order of its own: thread t of 256 sums w_pole[q] * g[pole_dst[q]] over q = t, t + 256, ... ascending (caps of weight 0
 *   skipped; whether that product is fused into the sum is not promised), the 256 partial sums are combined by a binary tree
 *   (p[t] += p[t + s] for s = 128, 64, ..., 1), one sum per row; where the two rows coincide the first row's term is added first.
 * Determinism: no floating-point atomics; the bits are the same across calls, nfields batching, float32 / float64 inputs that hold the
 * same values and the two layouts.  Stream as mpg_regrid_dev: the first call on a handle builds the transposed index (allocates and synchronises; it is
 * dropped whenever the handle is re-indexed); every later call only enqueues and can be captured in a hipGraph. */
int mpg_regrid_transpose_dev(mpg_handle rh, const void *src_dev, int src_type, int64_t src_level_stride, int nlev, int nfields,
                             void *dst_dev, int dst_type, int dst_layout, void *hip_stream);
/* Regrid onto a mesh, in either memory order of a mesh field: grid planes in, a mesh slab out -- the argument order of
 * mpg_regrid_transpose_dev, plus the typed calls' scale and offset.  The hot path of a Grid -> Mesh handle (mpg_regrid_store_to_mesh); it
 * is not tied to how the handle was stored: fixed 4-, 3- and 1-slot handles are all accepted.
 * src_dev: [nfields][nlev][plane], plane = n_src of mpg_handle_info, planes src_level_stride elements apart (0 = dense; below n_src ->
 * MPG_ERR_INVALID_ARG); a pitched result of the *_pitched_dev calls is accepted as it is, its pad is never read.
 * dst_dev: nfields slabs of nlev * n_dst in dst_layout: MPG_LAYOUT_CELL_FAST [lev][cell] or MPG_LAYOUT_LEV_FAST [cell][lev] (MPAS file
 * order: the slab can go into an init or restart file as it is).  Fully overwritten; unmapped points get (dst type) fma(0.0, scale, offset).
 * Types: MPG_TYPE_F64 / MPG_TYPE_F32 on either side, float64 arithmetic, dst = (dst type) fma(regrid(src), scale, offset) rounded once
 * at the store; MPG_TYPE_BE -> MPG_ERR_UNSUPPORTED.  MPG_ERR_UNSUPPORTED too for CSR handles (conservative, from-weights) and for handles
 * with pole caps.
 * Contract by identity, no tolerance: with MPG_LAYOUT_CELL_FAST the bytes equal what mpg_regrid_typed_dev(rh, src, src_type,
 * MPG_LAYOUT_CELL_FAST, nlev, nfields, dst, dst_type, scale, offset, stream) writes on the same handle from a dense source -- slot order,
 * accumulate expression, unmapped rule and epilogue are the same code; with MPG_LAYOUT_LEV_FAST element [c][k] has the bits of element
 * [k][c] of that result.  The same bits across calls, across nfields batching and between a pitched and a dense source.  No atomics.
 * Stream as mpg_regrid_dev.  The call allocates nothing and synchronises nothing: it can be captured in a hipGraph from the first call.
 * CSR handles are served by mpg_regrid_csr_to_mesh_dev. */
int mpg_regrid_to_mesh_dev(mpg_handle rh, const void *src_dev, int src_type, int64_t src_level_stride, int nlev, int nfields,
                           void *dst_dev, int dst_type, int dst_layout, double scale, double offset, void *hip_stream);
/* Conservative Store onto a mesh: ESMF_FieldRegridStore(regridmethod=CONSERVE, normType=) with a Grid as the source and a Mesh's elements
 * as the destination -- snow, precipitation, increments of extensive quantities taken back to the MPAS cells with their integral kept.
 * Source polygons are the grid's cells, the four CORNER points around centre (i, j), source index = j * nx + i, n_src = nx * ny (a grid
 *   without CORNER coordinates -> MPG_ERR_INVALID_ARG).  Destination polygons are the mesh's Voronoi cells from verticesOnCell;
 *   mpg_handle_info reports n_dst = nx_dst = nCells, ny_dst = 1.  I(c, g), the area of cell c inside grid cell g, is the very number
 *   the Mesh -> Grid conservative Store computes (great-circle sides, the same clip and the same area code, no floating-point
 *   contraction); area(c) is the cell polygon's own area by the same triangle fan.
 * Weights, rows keyed by mesh cell.  MPG_NORM_DSTAREA (ESMF's default normType): w = I / area(c) -- a partly covered cell gets coverage
 *   times mean.  MPG_NORM_FRACAREA: w = I / sum_g I -- a partly covered cell gets the mean of its covered part.  An entry is dropped when
 *   I <= 1e-14 * area(c) (the sliver rule of the Mesh -> Grid Store, applied to this destination).  An uncovered cell has an empty row:
 *   Regrid gives 0.0.  The dst fraction frac(c) = sum_g I / area(c), summed in ascending g (0 for an uncovered cell), stays on the device
 *   with the handle; mpg_handle_get_dst_frac copies its n_dst values to the host (MPG_ERR_INVALID_ARG on a handle that has none).
 *   This is NOT the transpose of the Mesh -> Grid handle: with A[g][c] = I / area(g) this matrix is B = D_c^-1 A^T D_g.
 * The handle is an ordinary CSR one (nnz_per_row 0, method conservative), columns ascending within a row, the same bytes from run to run.
 *   Both candidate routes -- index boxes on a grid with an inverse projection, the pyramid walk otherwise or under
 *   mpg_tune("store_boxes", 0) -- give identical handles; grids created with MPG_GRID_PERIODIC_I are accepted (collapsed pole sides
 *   bound nothing).  mpg_handle_store_stats, _store_path and _store_ms are filled as for the Mesh -> Grid Store.
 * Refusals.  MPG_ERR_UNSUPPORTED: a mesh of mpg_mesh_create_window; maxEdges > 12.  MPG_ERR_OVERFLOW: ids or entries beyond int32; a
 *   clipped polygon that outgrew its vertex slots (a non-convex cell).  MPG_ERR_INVALID_ARG: NULL arguments, unknown norm_type.
 * Cached like every Store, the key carrying the direction and norm_type (the two normalisations are two handles, and neither collides
 *   with a Mesh -> Grid key of the same pair); parked entries go when their mesh or grid is destroyed; mpg_mesh_set_source_window
 *   passes these handles by.  There is no _begin variant.  Everything that takes a CSR handle takes this one: mpg_regrid_typed[_pitched]_dev
 *   ([lev][cell]), mpg_regrid_masked_dev, mpg_regrid_transpose_dev, mpg_handle_get_csr; mpg_regrid_csr_to_mesh_dev below adds the mesh's
 *   own memory order. */
enum { MPG_NORM_DSTAREA = 0, MPG_NORM_FRACAREA = 1 };
int mpg_regrid_store_conserve_to_mesh(mpg_grid src, mpg_mesh dst, int norm_type, mpg_handle *out);
int mpg_handle_get_dst_frac(mpg_handle rh, double *frac_host);   /* [n_dst]; MPG_ERR_INVALID_ARG on a handle that has none (mpg_regrid_store_conserve_mesh stores one too) */
/* CSR Regrid in mesh order: the arguments of mpg_regrid_to_mesh_dev with the same meaning -- grid planes [nfields][nlev][plane], plane =
 * n_src, src_level_stride elements apart (0 = dense; below n_src -> MPG_ERR_INVALID_ARG; the pad is never read), out a slab of
 * nlev * n_dst per field in MPG_LAYOUT_CELL_FAST [lev][cell] or MPG_LAYOUT_LEV_FAST [cell][lev], MPG_TYPE_F64 / MPG_TYPE_F32 on either
 * side, float64 arithmetic, dst = (dst type) fma(x, scale, offset) rounded once at the store.  Accepts ANY CSR handle without pole caps:
 * mpg_regrid_store_conserve_to_mesh's, a Mesh -> Grid conservative one, one of mpg_handle_from_weights (an ESMF weight file).
 * Refusals.  MPG_ERR_UNSUPPORTED: a fixed handle (mpg_regrid_to_mesh_dev serves those); MPG_TYPE_BE.  MPG_ERR_INVALID_ARG: a stride
 * below the plane, a bad layout, nlev < 1, NULL.
 * Contract by identity, no tolerance: a row's value is acc = fma(val[q], src[col[q]], acc) from 0.0 in stored order, then the epilogue
 * -- the expression of the typed Regrid's CSR kernel -- so with MPG_LAYOUT_CELL_FAST the bytes equal what mpg_regrid_typed_dev writes on
 * the same handle from a dense source, and with MPG_LAYOUT_LEV_FAST element [c][k] has the bits of element [k][c] of that result; an
 * empty row gives (dst type) fma(0.0, scale, offset).  The same bits across calls, across nfields batching and between a pitched and a
 * dense source.  No atomics.  Stream as mpg_regrid_dev.  The call allocates nothing and synchronises nothing: it can be captured in a
 * hipGraph from the first call. */
int mpg_regrid_csr_to_mesh_dev(mpg_handle rh, const void *src_dev, int src_type, int64_t src_level_stride, int nlev, int nfields,
                               void *dst_dev, int dst_type, int dst_layout, double scale, double offset, void *hip_stream);
/* Regrid from rows to rows: [cell][lev] in and [cell][lev] out -- MPAS file order on both sides, what a Mesh -> Mesh job reads from one
 * MPAS file and writes to another, in one pass (mpg_regrid_typed_dev writes only [lev][point], mpg_regrid_to_mesh_dev reads only
 * [lev][plane]).  The hot path of a Mesh -> Mesh handle (mpg_regrid_store_mesh); it is not tied to how the handle was stored: any fixed
 * handle with 1, 3 or 4 slots and no pole caps is accepted.
 * src_dev: nfields slabs of [n_src][nlev], n_src the handle's current index space (the window count after mpg_mesh_set_source_window,
 * the local extent after mpg_handle_localize / rebase).  dst_dev: nfields slabs of [n_dst][nlev], fully overwritten; an unmapped point
 * gets (dst type) fma(0.0, scale, offset).
 * Types: MPG_TYPE_F64 / MPG_TYPE_F32 on either side, float64 arithmetic, dst = (dst type) fma(regrid(src), scale, offset) rounded once
 * at the store.  Refusals.  MPG_ERR_UNSUPPORTED: MPG_TYPE_BE; CSR handles (conservative, from-weights: mpg_regrid_csr_rows_dev serves
 * them); handles with pole caps.
 * MPG_ERR_INVALID_ARG: nlev < 1, nfields < 1, NULL.
 * Contract by identity, no tolerance: element [p][k] has the bits of element [k][p] of what mpg_regrid_typed_dev(rh, src, src_type,
 * MPG_LAYOUT_LEV_FAST, nlev, nfields, dst, dst_type, scale, offset, stream) writes on the same handle -- slot order, accumulate
 * expression, unmapped rule and epilogue are the same code.  The same bits across calls and across nfields batching.  No atomics.
 * Stream as mpg_regrid_dev.  The call allocates nothing and synchronises nothing: it can be captured in a hipGraph from the first call. */
int mpg_regrid_rows_dev(mpg_handle rh, const void *src_dev, int src_type, int nlev, int nfields, void *dst_dev, int dst_type, double scale,
                        double offset, void *hip_stream);
/* Conservative Mesh -> Mesh: ESMF_FieldRegridStore(regridmethod=CONSERVE, normType=) with the elements of one Mesh as the source and
 * the elements of another as the destination -- precipitation, snow, soil water, mass increments and tracers of a global run feeding a
 * limited-area mesh, of a 15-km state moved onto a 3-km mesh, of a restart after re-meshing -- in ONE conservative step instead of two
 * hops through a grid (which smear twice and conserve only on the intermediate grid's footprint).
 * Polygons: the Voronoi cells of both meshes from verticesOnCell, great-circle sides.  I(d, s) is the area of source cell s inside
 *   destination cell d: the source cell is the subject polygon, made counter-clockwise by the sign of its own fan area (its listed
 *   order reversed when that is negative); it is clipped by the destination cell's sides in listed order, that cell made
 *   counter-clockwise the same way; clip-plane normals in difference form a x (b - a); the in-place clip of the other conservative
 *   Stores with its 1e-15 * |n| inside rule; a side with |b - a|^2 < 1e-24 bounds nothing; the area is the triangle fan from slot 0,
 *   clamped at 0; area(d) is the cell polygon's own fan area; no floating-point contraction.
 * Weights, rows keyed by destination cell, columns = source cell ids, ascending.  MPG_NORM_DSTAREA: w = I / area(d).  MPG_NORM_FRACAREA:
 *   w = I / sum_s I.  An entry is dropped when I <= 1e-14 * area(d); an uncovered cell has an empty row: Regrid gives 0.0.  The dst
 *   fraction frac(d) = sum_s I / area(d), summed in ascending s, stays with the handle (mpg_handle_get_dst_frac).
 * The handle is an ordinary CSR one (nnz_per_row 0, method conservative): mpg_handle_info reports n_src = the source mesh's nCells,
 *   n_dst = nx_dst = the destination's nCells, ny_dst = 1.  Two Stores of the same pair give the same bytes: rows come from a count, a
 *   scan and an ordered insert, no atomic decides a stored byte.
 * Candidates: a box tree over the source mesh's cell polygons (built at the first such Store of a source mesh and kept on it) walked
 *   by every destination cell with its own box; the boxes hold the whole spherical polygons, so no pair with I > 0
 *   is removed.  The pair list has exact size: there is no fixed per-cell list and no spill path.
 * Refusals.  MPG_ERR_UNSUPPORTED: either mesh made by mpg_mesh_create_window; maxEdges > 12 on either mesh.  MPG_ERR_OVERFLOW: counts,
 *   pairs or entries beyond int32; a clipped polygon that outgrew its vertex slots (a non-convex cell).  MPG_ERR_INVALID_ARG: NULL
 *   arguments, unknown norm_type.  src == dst is allowed (the diagonal, up to slivers below the 1e-14 rule).
 * Cached like every Store under (src, ELEMENT, dst, ELEMENT, CONSERVE + 256 * norm_type + the Mesh -> Mesh kind bit): the two
 *   normalisations are two handles; mpg_mesh_set_source_window on the SOURCE mesh rebases these handles like every other Mesh -> Mesh
 *   handle, a window on the destination mesh passes them by; parked entries go when EITHER mesh is destroyed.  There is no _begin
 *   variant.  mpg_handle_store_ms is filled; mpg_handle_store_stats: [1] pairs clipped, [2] destination cells that left the common
 *   path (always 0: there is one path), [3] microseconds this Store spent building the source mesh's cell tree (0 when the mesh had it
 *   already), [6] vertex slots of the clip (the two meshes' largest vertex counts added, at most 24).
 * Everything that takes a CSR handle takes this one: mpg_regrid_typed[_pitched]_dev, mpg_regrid_masked_dev, mpg_regrid_transpose_dev,
 *   mpg_regrid_csr_to_mesh_dev, mpg_handle_get_csr; mpg_regrid_csr_rows_dev reads and writes MPAS file order.
 *
 * mpg_regrid_csr_rows_dev: the CSR Regrid of rows onto rows -- the arguments and meaning of mpg_regrid_rows_dev: src_dev nfields slabs of
 *   [n_src][nlev], dst_dev nfields slabs of [n_dst][nlev], fully overwritten, MPG_TYPE_F64 / MPG_TYPE_F32 on either side, float64
 *   arithmetic.  Accepts ANY CSR handle without pole caps: this Store's, both other conservative Stores', mpg_handle_from_weights'.
 *   Refusals.  MPG_ERR_UNSUPPORTED: a fixed handle (mpg_regrid_rows_dev serves those); MPG_TYPE_BE; handles with pole caps.
 *   MPG_ERR_INVALID_ARG: nlev < 1, nfields < 1, NULL.
 *   Contract by identity, no tolerance: acc = fma(val[q], src[col[q] * nlev + k], acc) from 0.0 in stored order, then
 *   (dst type) fma(acc, scale, offset); element [p][k] has the bits of element [k][p] of what mpg_regrid_typed_dev(rh, src, src_type,
 *   MPG_LAYOUT_LEV_FAST, ...) writes on the same handle; an empty row gives (dst type) fma(0.0, scale, offset).  The same bits across
 *   calls and across nfields batching.  No atomics.  Stream as mpg_regrid_dev.  The call allocates nothing and synchronises nothing:
 *   it can be captured in a hipGraph from the first call. */
int mpg_regrid_store_conserve_mesh(mpg_mesh src, mpg_mesh dst, int norm_type, mpg_handle *out);
int mpg_regrid_csr_rows_dev(mpg_handle rh, const void *src_dev, int src_type, int nlev, int nfields, void *dst_dev, int dst_type, double scale,
                            double offset, void *hip_stream);
/* diagnostics: sources with at least one entry, and the longest transposed row (builds the transposed index if needed) */
int mpg_handle_transpose_stats(mpg_handle rh, int64_t *n_referenced, int64_t *max_per_source);
/* GPU time (ms) of the last transposed index build of this handle; 0 while none is built */
int mpg_handle_transpose_build_ms(mpg_handle rh, float *ms);
/* Masked Regrid: missing sources are skipped, the valid ones stand in for them above a threshold, everything else is filled.
 * What ESMF calls dynamic masking (dynamicSrcMaskValue) and xESMF skipna / na_thres -- NOT ESMF's Store-time srcMaskValues (mpg_handle_mask and
 * mpg_handle_extrapolate_masked are those): the weights are those of the unmasked Store of this handle, only their use changes per call.
 * For a destination point p and level k take the stored entries q in stored order (slot order of a fixed-nnz handle, CSR order of
 * a conservative or a from-weights handle, duplicates included).  All arithmetic is float64.
 *   valid(q)   idx_q >= 0, its source is not statically masked (src_mask_dev), and its value at level k is not missing under
 *              `flags`: MPG_MISSING_NAN -> a NaN is missing; MPG_MISSING_VALUE -> an element is missing when
 *              (double)element == missing_value.  flags may be 0 (static mask only).
 *   Wt         the plain left-to-right sum of the point's stored weights (1 for nearest neighbour)
 *   Wv         the same sum with the weight of every invalid entry replaced by 0.0
 *   N          the unmasked Regrid's own expression with weight AND value of every invalid entry replaced by 0.0 (a missing NaN never
 *              enters a product)
 *   defined    the point has at least one stored entry, Wv > 0 and Wv >= min_valid_frac * Wt
 *   result     defined: dst = (dst type) fma(N * (Wt / Wv), scale, offset);  undefined -- unmapped points included --:
 *              dst = (dst type) fill_value, whatever scale and offset are (fill_value for unmapped points: a result can tell
 *              "no data" from 0).  Wt / Wv keeps a partly covered conservative cell scaled as the unmasked Regrid scales it; for
 *              bilinear weights (Wt = 1 up to rounding) it is the usual renormalisation.
 * Bit identity with the unmasked Regrid when nothing is missing: a point none of whose entries is invalid has Wv and Wt of the same
 * bits, Wt / Wv == 1.0, and stores exactly what the typed, pitched unmasked call with scale 1, offset 0 stores for it -- switching the
 * call on for a field that happens to have no gaps changes nothing.  Nearest-neighbour handles copy when valid and fill when not
 * (no search for the next valid neighbour).
 * src_mask_dev: optional [n_src] bytes on the device, in the handle's CURRENT index space (the window after
 * mpg_mesh_set_source_window, the local ids after a localize / rebase of the handle): non-zero = never use this source.
 * The destination is fully overwritten; dst_level_stride as in the _pitched_dev calls (0 = dense, below the plane size ->
 * MPG_ERR_INVALID_ARG), the pad of pitched planes is never written.  Both source layouts, MPG_TYPE_F64 / MPG_TYPE_F32 on either
 * side, every handle kind.  Refused with MPG_ERR_UNSUPPORTED: MPG_TYPE_BE on either side, and handles with pole caps (pole-cap
 * count > 0: winds are never masked).  Refused with MPG_ERR_INVALID_ARG: rh or opts NULL, min_valid_frac outside [0, 1] or NaN,
 * MPG_MISSING_VALUE with a NaN missing_value, unknown flag bits.
 * Stream as mpg_regrid_dev; the call allocates nothing and synchronises nothing, so it can be captured in a hipGraph from the first
 * call.  No atomics: the same bits across calls, across nfields batching and for the two source layouts holding the same values. */
enum { MPG_MISSING_NAN = 1, MPG_MISSING_VALUE = 2 };
typedef struct mpg_mask_opts {
  int flags;                    /* MPG_MISSING_NAN | MPG_MISSING_VALUE, may be 0 (static mask only) */
  double missing_value;         /* with MPG_MISSING_VALUE: an element is missing when (double)element == missing_value */
  const uint8_t *src_mask_dev;  /* optional [n_src] in the handle's CURRENT index space: non-zero = never use this source (every level, every field) */
  double min_valid_frac;        /* in [0, 1] */
  double fill_value;            /* any double, NaN allowed */
  double scale, offset;         /* writer's epilogue, applied to DEFINED points only */
} mpg_mask_opts;
int mpg_regrid_masked_dev(mpg_handle rh, const void *src_dev, int src_type, int src_layout, int nlev, int nfields,
                          void *dst_dev, int dst_type, int64_t dst_level_stride, const mpg_mask_opts *opts, void *hip_stream);
/* The adjoint of the masked Regrid: the gradient of a loss with respect to the source of mpg_regrid_masked_dev, from its gradient with
 * respect to the result.  The forward is linear in the valid source values and Wv depends only on WHICH sources are missing, so the
 * adjoint is exact.  mpg_regrid_transpose_dev of the incoming gradient is not it: that ignores Wt / Wv, sends gradient into sources
 * that never entered the forward, and lets a NaN in the gradient of an undefined output spread to every source the output touches.
 *   g_dev     the gradient of the masked Regrid's result, [nfields][nlev][plane of n_dst], MPG_TYPE_F64 or MPG_TYPE_F32; planes
 *             g_level_stride elements apart (0 = dense, below n_dst -> MPG_ERR_INVALID_ARG).  The pad is never read: a pitched
 *             result buffer can be fed back as it is.
 *   src_dev   the source the forward call read, in src_layout ([lev][cell] or [cell][lev]), nfields slabs.  It is read only to decide
 *             validity: its values never enter a product.
 *   dst_dev   the gradient with respect to src: nfields slabs of nlev * n_src in the same src_layout, fully overwritten.
 *   opts      the forward's mpg_mask_opts: flags, missing_value, src_mask_dev, min_valid_frac and scale are used; fill_value and
 *             offset are ignored (they have no derivative).
 *   work_dev  a caller-owned float64 workspace of nfields * nlev * n_dst elements, dense.  It holds the scaled gradient h below and is
 *             fully overwritten; its contents on return are part of the contract.  It must not be NULL and must not alias g_dev,
 *             src_dev or dst_dev (MPG_ERR_INVALID_ARG).
 * MPG_TYPE_F64 or MPG_TYPE_F32 on each of g, src and dst independently; arithmetic is float64, with one rounding at the store.
 * Contract by identity, no tolerance; nothing is contracted.  valid(q), Wt, Wv and defined are, word for word, those of the
 * mpg_regrid_masked_dev contract above: same order, same expressions; the decision Wv > 0 && Wv >= min_valid_frac * Wt is bit-exact.
 *   h[k][p]    = defined(p, k) ? ((double)g[k][p] * scale) * (Wt / Wv) : +0.0 -- two separately rounded products; a select, never a
 *                product with 0: a NaN or Inf in g at an undefined or unmapped point reaches no source
 *   acc        = fma(w_j, h[k][row_j], acc) from +0.0 over the stored entries j that reference source c, in ascending (destination
 *                point, slot) order -- exactly the chain of mpg_regrid_transpose_dev (nearest neighbour: w_j = 1.0)
 *   ok(c, k)   = src_mask[c] == 0 and src(c, k) not missing under flags
 *   dst[c][k]  = ok(c, k) ? (dst type) acc : +0.0 -- a select; a source no entry references gets +0.0
 * Identity with the unmasked transpose: with nothing missing, scale == 1 and every point mapped, Wt / Wv == 1.0, h equals (double)g
 * bit for bit and the result equals mpg_regrid_transpose_dev into the same type and layout bit for bit.
 * Derivative: the result is the derivative of the forward with respect to every valid source element, and exactly +0.0 at every
 * invalid one.  It is the adjoint of the linear part, scale included; it is not an inverse.
 * No floating-point atomics: the same bits across calls, across nfields batching, for the two layouts and across float32 / float64
 * inputs that hold the same values.
 * Refused as mpg_regrid_masked_dev refuses: MPG_ERR_UNSUPPORTED for MPG_TYPE_BE on any side and for handles with pole caps;
 * MPG_ERR_INVALID_ARG for a NULL rh, opts, g_dev, src_dev, dst_dev or work_dev, a bad layout, nlev or nfields < 1, min_valid_frac
 * outside [0, 1] or NaN, MPG_MISSING_VALUE with a NaN missing_value, unknown flag bits, a stride below n_dst and an aliased workspace.
 * A refused call writes nothing.
 * Stream as mpg_regrid_transpose_dev: the first call on a handle builds its transposed index, which allocates and synchronises;
 * later calls only enqueue and can be captured in a hipGraph. */
int mpg_regrid_masked_transpose_dev(mpg_handle rh, const void *g_dev, int g_type, int64_t g_level_stride, const void *src_dev, int src_type,
                                    int src_layout, int nlev, int nfields, void *dst_dev, int dst_type, const mpg_mask_opts *opts,
                                    double *work_dev, void *hip_stream);
/* ESMF_FieldBundleRegrid as interp.F90:240-254 issues it: ONE Regrid over every field of a bundle whose fields are SEPARATE
 * arrays (an ESMF bundle holds independent fields; here: nfields device pointers on either side, host arrays of pointers).
 * All fields share the handle, the layout, nlev and the element types; offsets (nfields values, or NULL for 0) is the
 * epilogue offset per field (T - 300 beside fields written as they are).  The same kernels as mpg_regrid_typed_dev with
 * nfields consecutive slabs -- one launch, the per-point indices and weights shared by the fields from the L2 -- and the same
 * bits as nfields single calls; 10 % (configuration 4) to 18 % (configuration 5) faster than those. */
int mpg_regrid_bundle_typed_dev(mpg_handle rh, int nfields, const void *const *src_dev, int src_type, int src_layout, int nlev,
                                void *const *dst_dev, int dst_type, double scale, const double *offsets, void *hip_stream);
/* ... with the level planes of every destination array dst_level_stride elements apart (plane k of field f at dst_dev[f] + k * stride) */
int mpg_regrid_bundle_typed_pitched_dev(mpg_handle rh, int nfields, const void *const *src_dev, int src_type, int src_layout, int nlev,
                                        void *const *dst_dev, int dst_type, double scale, const double *offsets, int64_t dst_level_stride,
                                        void *hip_stream);
/* The same on HOST buffers (pageable memory: Fortran allocatables, numpy arrays), for hosts that keep the reference's
 * file -> host array -> regrid -> host array -> file shape and are therefore bound by the PCIe link: float32 sources
 * and results cross the link as they are stored in the files (half the bytes of the float64 route), and the field is cut
 * into chunks whose upload, kernel and download overlap (full duplex, a helper thread downloads while the caller
 * uploads).  Blocks until dst_host is complete. */
int mpg_regrid_typed(mpg_handle rh, const void *src_host, int src_type, int src_layout, int nlev, int nfields,
                     void *dst_host, int dst_type, double scale, double offset);
/* ... and over a bundle whose fields are SEPARATE host arrays (mpg_regrid_bundle_typed_dev's host twin): all fields go through
 * one pipeline -- the upload of field k + 1, the Regrid of field k and the download of field k - 1 overlap -- where a file-order
 * field handed over alone is uploaded, regridded and downloaded one step after the other (configuration 4, float64: 39 ms per
 * field alone, 24 in a bundle).  offsets: one epilogue offset per field, or NULL.  Blocks until every destination is complete. */
int mpg_regrid_bundle_typed(mpg_handle rh, int nfields, const void *const *src_host, int src_type, int src_layout, int nlev,
                            void *const *dst_host, int dst_type, double scale, const double *offsets);
/* ESMF_FieldBundleRegridRelease (interp.F90:450,455,461) */
int mpg_handle_release(mpg_handle rh);

/* ---- rotate_winds_cgrid (interp.F90:689-749): in place on CENTER-stagger u, v [nlev][ny][nx] with
 * cosalpha/sinalpha [ny][nx] (model_grid.F90:1154).  Values, a contract by identity (interp.F90:737-748 as written): per point
 *   tana = sa / ca;  den = ca + sa * tana                       and per level, from the old uo, vo
 *   un = (uo + vo * tana) / den;  vn = (vo - un * sa) / ca      (vn uses the NEW un)
 * seven float64 operations, each rounded, nothing contracted or reordered; ca == +-0.0 and non-finite winds give what IEEE 754 gives.
 * The host form uploads, runs the same kernel and downloads: the same bits. */
int mpg_rotate_winds(int64_t npts, int nlev, const double *cosa_host, const double *sina_host,
                     double *u_host, double *v_host);
int mpg_rotate_winds_dev(int64_t npts, int nlev, const double *cosa_dev, const double *sina_dev,
                         double *u_dev, double *v_dev, void *hip_stream);
/* The whole wind chain of interp_hist_data in ONE pass over the mass-point winds (interp.F90:291-328): rotate_winds_cgrid on
 * (UMASS, VMASS) -- :291-293, 737-748 -- followed by the two Grid -> Grid Regrids UMASS(CENTER) -> U(EDGE1) -- :295-311 -- and
 * VMASS(CENTER) -> V(EDGE2) -- :313-328.  u/v_target_grid_nostag are intermediates the reference never writes, so the earth-relative
 * mass winds are read once and only U and V are stored; the results are bit-identical to mpg_rotate_winds_dev followed by
 * mpg_regrid_dev (dst_type MPG_TYPE_F64) or mpg_regrid_typed_dev(..., dst_type, 1.0, 0.0) (any other dst_type) on the two handles.
 *   rh_edge1, rh_edge2   handles of mpg_regrid_store_grid(grid, CENTER, EDGE1 / EDGE2) on ONE grid; either may be NULL (that
 *                        component is not produced: do_u_interp / do_v_interp, interp.F90:295,313)
 *   cosa_dev, sina_dev   [ny][nx] as for mpg_rotate_winds_dev, or both NULL: no rotation (proj_code /= PROJ_LC, or one component)
 *   umass_dev, vmass_dev [nlev][ny][nx] float64, NOT modified
 *   u_dev, v_dev         [nlev][ny][nx+1], [nlev][ny+1][nx] of dst_type
 *   umass_rot_dev, vmass_rot_dev   optional (NULL): the rotated mass winds [nlev][ny][nx] as mpg_rotate_winds_dev would have left
 *                        them in place; must not be the input arrays
 * MPG_ERR_UNSUPPORTED: the handles are not such a pair (re-indexed by mpg_handle_localize / rebase, different grids): use the
 * three separate calls. */
int mpg_wind_destagger_dev(mpg_handle rh_edge1, mpg_handle rh_edge2, const double *cosa_dev, const double *sina_dev,
                           const double *umass_dev, const double *vmass_dev, int nlev, void *u_dev, void *v_dev, int dst_type,
                           double *umass_rot_dev, double *vmass_rot_dev, void *hip_stream);
/* ... with U's and V's level planes dst_level_stride elements apart: ONE stride for both, at least ny * (nx + 1) and (ny + 1) * nx
 * (mpg_dst_level_stride of the larger plane); umass_rot_dev / vmass_rot_dev stay dense. */
int mpg_wind_destagger_pitched_dev(mpg_handle rh_edge1, mpg_handle rh_edge2, const double *cosa_dev, const double *sina_dev,
                                   const double *umass_dev, const double *vmass_dev, int nlev, void *u_dev, void *v_dev, int dst_type,
                                   double *umass_rot_dev, double *vmass_rot_dev, int64_t dst_level_stride, void *hip_stream);
/* The same chain for a host that keeps its fields in HOST arrays, as the reference does (farrayPtr in, farrayPtr out: interp.F90:702-735
 * fetches the pointers, :291-328 runs the chain).  The three separate host calls -- mpg_rotate_winds, then mpg_regrid on each handle --
 * move 4 fields up and 4 down over the link; this one moves the earth-relative mass winds up ONCE in chunks of levels and only U and V
 * down, both directions at once (2 up, 2 down: the chain is link-bound, so about half the time).  Same bits as mpg_wind_destagger_dev.
 * All pointers are host pointers; cosa_host / sina_host [ny][nx] or both NULL; umass_rot_host / vmass_rot_host optional (NULL) and --
 * unlike the device form -- MAY be the input arrays themselves: rotate_winds_cgrid's in-place result (a level's rotated winds come
 * down after that level went up).  Blocks until every destination is complete. */
int mpg_wind_destagger(mpg_handle rh_edge1, mpg_handle rh_edge2, const double *cosa_host, const double *sina_host,
                       const double *umass_host, const double *vmass_host, int nlev, void *u_host, void *v_host, int dst_type,
                       double *umass_rot_host, double *vmass_rot_host);
/* The ADJOINT of the wind chain, for a loss on the target grid's U and V whose gradient has to reach the mass-point winds (and from
 * there the mesh, through mpg_regrid_transpose_dev): a three-call chain -- mpg_regrid_transpose_dev on each handle, then the rotation's
 * adjoint below -- and a fused call that matches that chain bit for bit.
 * mpg_rotate_winds_transpose_dev: the adjoint of mpg_rotate_winds_dev, in place on the gradients gu, gv [nlev][npts] float64 with
 * cosa / sina [npts].  Values, a contract by identity: the reverse mode of interp.F90:737-748 as stated above, per point
 *   tana = sa / ca;  den = ca + sa * tana                       and per level, from the incoming gun, gvn (the gradients of un, vn)
 *   a = gvn / ca;  t = a * sa;  b = gun - t;  guo = b / den;  p = guo * tana;  gvo = a + p
 * each operation rounded once, nothing contracted or reordered; ca == +-0.0 and non-finite inputs give what IEEE 754 gives.
 * (Algebraically guo = gun ca - gvn sa, gvo = gun sa + gvn ca.)  Not an adjoint with respect to the angles. */
int mpg_rotate_winds_transpose_dev(int64_t npts, int nlev, const double *cosa_dev, const double *sina_dev, double *gu_dev, double *gv_dev,
                                   void *hip_stream);
/* The adjoint of mpg_wind_destagger_dev in ONE pass: the gradients of U and V back to the gradients of the mass-point winds.
 *   rh_edge1, rh_edge2   the CENTER -> EDGE1 / CENTER -> EDGE2 pair of one grid, under the same test as mpg_wind_destagger_dev; anything
 *                        else -> MPG_ERR_UNSUPPORTED.  Either may be NULL without a rotation (that component is not produced)
 *   cosa_dev, sina_dev   [ny][nx] as for the forward, or both NULL: no rotation
 *   gu_dev, gv_dev       [nlev][ny][nx+1], [nlev][ny+1][nx], both of src_type (MPG_TYPE_F64 or MPG_TYPE_F32), planes src_level_stride
 *                        elements apart: 0 = dense, else ONE stride for both, at least the larger plane.  A pitched result of
 *                        mpg_wind_destagger_pitched_dev can be fed back as it is, its pad is never read
 *   gumass_rot_dev, gvmass_rot_dev   optional (NULL): the gradients of the forward's umass_rot / vmass_rot results, [nlev][ny][nx]
 *                        float64 (rotation only)
 *   gumass_dev, gvmass_dev   [nlev][ny][nx] float64, dense, fully overwritten
 * Values, per (mass point c, level k):
 *   s1, s2    exactly the sums of the mpg_regrid_transpose_dev contract on rh_edge1 / rh_edge2: ascending (destination point, slot)
 *             order, an fma chain from +0.0, +0.0 for a source no entry references.  Unmapped U and V points have no entries and are
 *             never read
 *   gun = s1 + gumass_rot, gvn = s2 + gvmass_rot   one add; no add when the pointer is NULL
 *   with rotation (guo, gvo) come from (gun, gvn) by the expressions of mpg_rotate_winds_transpose_dev; without, the components are
 *   independent, as in the forward: gumass = s1 iff rh_edge1 is given, gvmass = s2 iff rh_edge2 is given, and for handles with pole
 *   caps the pole term of the transpose contract is added last.
 * MPG_ERR_INVALID_ARG: both handles NULL; cosa without sina or the reverse; a rotation without both handles; gumass_rot_dev /
 * gvmass_rot_dev without a rotation; nlev < 1; a stride below the larger plane; an output pointer equal to an input pointer; a NULL
 * array that is needed.  MPG_ERR_UNSUPPORTED: MPG_TYPE_BE; a rotation together with pole caps, as in the forward; a level plane of
 * 4 GiB or more.
 * Bit contract: the result equals two mpg_regrid_transpose_dev calls into float64, then the optional adds, then
 * mpg_rotate_winds_transpose_dev.  The same bits across calls and across float32 / float64 inputs that hold the same values.  No
 * floating-point atomics.  Stream as mpg_regrid_transpose_dev: the first call on a handle builds its transposed index (allocates and
 * synchronises); every later call only enqueues and can be captured in a hipGraph. */
int mpg_wind_destagger_transpose_dev(mpg_handle rh_edge1, mpg_handle rh_edge2, const double *cosa_dev, const double *sina_dev,
                                     const void *gu_dev, const void *gv_dev, int src_type, int64_t src_level_stride, int nlev,
                                     const double *gumass_rot_dev, const double *gvmass_rot_dev, double *gumass_dev, double *gvmass_dev,
                                     void *hip_stream);
/* The wind chain turned round: U on one stagger and V on another -- grid-relative on a Lambert grid -- onto the points of a mesh as
 * earth-relative winds (uReconstructZonal / uReconstructMeridional), in ONE pass: the two Regrids, the rotation and the cast, without
 * float64 intermediates.  The inverse of interp.F90:737-748, which is algebraically u_g = u_e ca + v_e sa, v_g = v_e ca - u_e sa.
 *   rh_u, rh_v           fixed handles onto the SAME n_dst points, both with nnz_per_row 4 or both 1: typically
 *                        mpg_regrid_store_to_mesh(grid, EDGE1 / EDGE2, mesh, loc, BILINEAR).  rh_u == rh_v is allowed (winds on mass
 *                        points, any CENTER handle); the kernel then stages one set of indices.
 *   u_dev, v_dev         [nlev][rh_u.n_src], [nlev][rh_v.n_src] of src_type, planes u_level_stride / v_level_stride elements apart
 *                        (0 = dense; below n_src -> MPG_ERR_INVALID_ARG): the pitched U / V of mpg_wind_destagger_pitched_dev are
 *                        accepted as they are, their pad is never read
 *   cosa_dev, sina_dev   [n_dst] float64 at the DESTINATION points (mpg_mesh_rotang_dev), or both NULL: no rotation; exactly one NULL
 *                        -> MPG_ERR_INVALID_ARG
 *   ue_dev, ve_dev       nlev * n_dst each of dst_type, in dst_layout: MPG_LAYOUT_CELL_FAST [lev][cell] or MPG_LAYOUT_LEV_FAST
 *                        [cell][lev] (MPAS file order).  Both fully overwritten; neither may alias the other, a source or the
 *                        angles (MPG_ERR_INVALID_ARG)
 * Values, a contract by identity: float64 arithmetic without contraction (as mpg_rotate_winds_dev), per (point, level)
 *   a  = wsum_fixed<NNZ>(w_u, U[idx_u])       exactly mpg_regrid_to_mesh_dev(rh_u, dst F64, scale 1, offset 0)
 *   b  = wsum_fixed<NNZ>(w_v, V[idx_v])
 *   ue = a * ca - b * sa ;  ve = a * sa + b * ca     four products and two sums, each rounded; no rotation: ue = a, ve = b
 *   store (TD)ue, (TD)ve                              one rounding to the destination type
 * A point that is unmapped in either handle gets (TD)(+0.0) in BOTH results.  The same bits for both layouts ([c][k] of one is [k][c]
 * of the other), for dense and pitched sources, and from call to call.  No atomics.  Stream as mpg_regrid_dev.  The call allocates
 * nothing and synchronises nothing: it can be captured in a hipGraph from the first call.
 * Refusals, each with a message that names the way out.  MPG_ERR_UNSUPPORTED: CSR handles (conservative, periodic, from-weights: winds
 * from a periodic global grid go through mpg_wind_csr_to_mesh_dev), handles with pole caps, 3-slot handles or a pair of mixed nnz_per_row, MPG_TYPE_BE on
 * either side.  MPG_ERR_INVALID_ARG: NULL handles or arrays, rh_u.n_dst != rh_v.n_dst, nlev < 1, unknown enums.  MPG_ERR_OVERFLOW: more
 * 64-point blocks than one launch holds. */
int mpg_wind_to_mesh_dev(mpg_handle rh_u, mpg_handle rh_v, const double *cosa_dev, const double *sina_dev, const void *u_dev,
                         const void *v_dev, int src_type, int64_t u_level_stride, int64_t v_level_stride, int nlev, void *ue_dev,
                         void *ve_dev, int dst_type, int dst_layout, void *hip_stream);
/* cos / sin of the rotation angle at the cells (MPG_MESHLOC_ELEMENT, [nCells]) or vertices (MPG_MESHLOC_NODE, [nVertices]) of a mesh,
 * float64 device arrays for mpg_wind_to_mesh_dev: alpha = -hemi * cone * wrap180(lon - stand_lon) * pi / 180 with hemi, cone and
 * stand_lon of the grid's own projection and lon = atan2(y, x) in degrees of the mesh's stored unit vectors; cosa = cos(alpha), sina =
 * sin(alpha).  The sign is get_rotang's (model_grid.F90:2450-2507), whose centred differences the closed form meets to 2.3e-6 in sina on
 * the interior rows of a 30-km grid.  PROJ_LC only, as mpg_grid_get_rotang: any other projection -> MPG_ERR_UNSUPPORTED ("the forward
 * chain does not rotate there: pass NULL angles"), as are a grid without a projection (mpg_grid_create without mpg_grid_attach_proj) and
 * a mesh of mpg_mesh_create_window.  Asynchronous on hip_stream (as mpg_regrid_dev); allocates nothing. */
int mpg_mesh_rotang_dev(mpg_grid grid, mpg_mesh mesh, int meshloc, double *cosa_dev, double *sina_dev, void *hip_stream);
/* The same angles for the mesh's EDGES, composed with the projection onto the edge normal: per edge phi = angleEdge - alpha (one
 * float64 subtraction), cn = cos(phi), sn = sin(phi), float64 device arrays [nEdges] for mpg_wind_to_edges_dev.  alpha is exactly
 * mpg_mesh_rotang_dev's, -hemi * cone * wrap180(lon - stand_lon) * pi / 180 with lon = atan2(y, x) of the edge's stored unit vector;
 * the rotation to earth-relative winds (alpha) and the projection onto the normal (theta = angleEdge) are ONE rotation by theta - alpha.
 * grid == NULL gives alpha = 0: winds that are already earth-relative (a lat-lon or Mercator source).  A grid whose projection is not
 * PROJ_LC, or that carries none -> MPG_ERR_UNSUPPORTED ("the forward chain does not rotate there: pass a NULL grid").  A mesh without
 * edges or without angleEdge -> MPG_ERR_INVALID_ARG (mpg_mesh_set_edges).  Asynchronous on hip_stream; allocates nothing. */
int mpg_mesh_edge_rotang_dev(mpg_grid grid, mpg_mesh mesh, double *cn_dev, double *sn_dev, void *hip_stream);
/* Winds onto mesh EDGES: U on one stagger and V on another -- grid-relative on a Lambert grid -- onto the edge points of a mesh as the
 * edge-normal wind `u` MPAS carries (and, when asked, the tangential component), in ONE pass: the two Regrids, one rotation and the
 * cast, without float64 intermediates.
 *   rh_u, rh_v           fixed handles onto the SAME n_dst points, both with nnz_per_row 4 or both 1: typically
 *                        mpg_regrid_store_to_mesh(grid, EDGE1 / EDGE2, mesh, MPG_MESHLOC_EDGE, BILINEAR).  rh_u == rh_v is allowed; the
 *                        kernel then stages one set of indices.  The call does not look at the mesh: any such pair is served.
 *   cn_dev, sn_dev       [n_dst] float64, cos / sin of phi = angleEdge - alpha (mpg_mesh_edge_rotang_dev).  REQUIRED: there is no
 *                        un-rotated form; a host that wants one passes cos / sin of angleEdge
 *   u_dev, v_dev         [nlev][rh_u.n_src], [nlev][rh_v.n_src] of src_type, planes u_level_stride / v_level_stride elements apart
 *                        (0 = dense; below n_src -> MPG_ERR_INVALID_ARG): the pitched U / V of mpg_wind_destagger_pitched_dev are
 *                        accepted as they are, their pad is never read
 *   un_dev, ut_dev       nlev * n_dst each of dst_type, in dst_layout: MPG_LAYOUT_CELL_FAST [lev][edge] or MPG_LAYOUT_LEV_FAST
 *                        [edge][lev], the file order of u(nEdges, nVertLevels).  ut_dev may be NULL: only the normal component is
 *                        computed and stored.  Fully overwritten; neither may alias the other, a source or the angles
 *                        (MPG_ERR_INVALID_ARG)
 * Values, a contract by identity: float64 arithmetic without contraction, per (point, level)
 *   a  = fma(wsum_fixed<NNZ>(w_u, U[idx_u]), 1.0, 0.0)    exactly mpg_regrid_to_mesh_dev(rh_u, dst F64, scale 1, offset 0)
 *   b  = fma(wsum_fixed<NNZ>(w_v, V[idx_v]), 1.0, 0.0)
 *   un = a * cn + b * sn        two products and one sum, each rounded
 *   ut = b * cn - a * sn        only when ut_dev != NULL (the tangential component, 90 degrees counter-clockwise of the normal)
 *   store (TD)un [, (TD)ut]     one rounding to the destination type
 * (un = ue cos(theta) + ve sin(theta) with the earth-relative ue = a ca - b sa, ve = a sa + b ca of mpg_wind_to_mesh_dev, composed.)
 * A point that is unmapped in either handle gets (TD)(+0.0) in every result.  The same bits for both layouts, for dense and pitched
 * sources, and from call to call.  No atomics.  Stream as mpg_regrid_dev.  The call allocates nothing and synchronises nothing: it
 * can be captured in a hipGraph from the first call.
 * Refusals, those of mpg_wind_to_mesh_dev under the name mpg_wind_to_edges.  MPG_ERR_UNSUPPORTED: CSR handles (conservative, periodic,
 * from-weights: winds from a periodic global grid go through mpg_wind_csr_to_edges_dev), handles with pole caps, 3-slot handles or a pair of mixed
 * nnz_per_row, MPG_TYPE_BE on either side.  MPG_ERR_INVALID_ARG: NULL handles or arrays (cn_dev / sn_dev included), rh_u.n_dst !=
 * rh_v.n_dst, nlev < 1, unknown enums, aliased arrays.  MPG_ERR_OVERFLOW: more 64-point blocks than one launch holds. */
int mpg_wind_to_edges_dev(mpg_handle rh_u, mpg_handle rh_v, const double *cn_dev, const double *sn_dev, const void *u_dev,
                          const void *v_dev, int src_type, int64_t u_level_stride, int64_t v_level_stride, int nlev,
                          void *un_dev, void *ut_dev, int dst_type, int dst_layout, void *hip_stream);
/* Winds through CSR handles: the two calls above for the handles they refuse -- U and V of a periodic global lat-lon or Gaussian
 * analysis (GFS, ERA5, an IFS product) onto the cells, vertices or edges of a mesh, in ONE pass: the two Regrids of
 * mpg_regrid_csr_to_mesh_dev, the rotation and the cast, without the two float64 intermediates of nlev * n_dst and with the handle's
 * indices and weights staged once.  The argument lists are those of mpg_wind_to_mesh_dev and mpg_wind_to_edges_dev and keep their
 * meaning: cosa_dev / sina_dev both set or both NULL (no rotation; exactly one NULL -> MPG_ERR_INVALID_ARG); cn_dev / sn_dev REQUIRED
 * (mpg_mesh_edge_rotang_dev; a NULL grid there for winds that are earth-relative already, as a lat-lon analysis has them); ut_dev may
 * be NULL; u_level_stride / v_level_stride in elements, 0 = dense, below n_src -> MPG_ERR_INVALID_ARG; results in MPG_LAYOUT_CELL_FAST
 * [lev][point] or MPG_LAYOUT_LEV_FAST [point][lev], fully overwritten.
 *   rh_u, rh_v           CSR handles (nnz_per_row 0) onto the SAME n_dst points: mpg_regrid_store_periodic_to_mesh,
 *                        mpg_regrid_store_conserve_to_mesh, mpg_regrid_store_conserve_mesh, mpg_handle_from_weights.  rh_u == rh_v is
 *                        the main case, a collocated analysis: the kernel then stages ONE run and feeds both accumulators from each
 *                        staged (col, val).  With two different handles each handle's run is walked for its own component.  The calls
 *                        do not look at the mesh.
 * Values, a contract by identity: float64 arithmetic without contraction, per (point, level) and per handle
 *   acc = fma(val[q], (double)src[col[q]], acc)    from 0.0, the row's entries in stored order, whatever LDS chunk an entry arrives in
 *   a  = fma(acc_u, 1.0, 0.0)                      exactly mpg_regrid_csr_to_mesh_dev(rh_u, dst F64, scale 1, offset 0)
 *   b  = fma(acc_v, 1.0, 0.0)                      the same with rh_v, V
 *   mesh call:   ue = a * ca - b * sa ;  ve = a * sa + b * ca      (no rotation: ue = a, ve = b)
 *   edges call:  un = a * cn + b * sn ;  ut = b * cn - a * sn      (ut only when ut_dev != NULL)
 *   store (TD)o0 [, (TD)o1]                        every product and sum rounded; one rounding to the destination type
 * A point whose row is empty in either handle gets (TD)(+0.0) in every result (0 * c - 0 * s can be -0.0, hence a mask).  The same bits
 * for both layouts, for dense and pitched sources, for rh_u == rh_v given once or as two equal handles, and from call to call.
 * No atomics.  Stream as mpg_regrid_dev.  The calls allocate nothing and synchronise nothing: they can be captured in a hipGraph from
 * the first call.  n_dst == 0 is success; a handle with no entries gives zeroed results.
 * CAVEAT, pole caps: under MPG_POLEMETHOD_ALLAVG a cap point gets the row mean of each wind COMPONENT -- what two scalar ESMF Regrids
 * give, and not a wind: for a solid-body rotation of unit speed about an axis tilted 45 degrees, from a 72 x 36 grid onto the 59 994
 * edges of a 20 000-cell mesh, un is off by at most 1.41e-3 on quad rows and by up to 0.53 on the 57 cap edges (24 x 12: 1.23e-2 and
 * 0.71).  A host that cares stores with MPG_POLEMETHOD_NONE and fills the cap points itself (mpg_regrid_masked_dev, a nearest handle);
 * a Cartesian-vector Regrid (ESMF 8.6's vectorRegrid) is the real answer: mpg_wind_vector_dev, below (6.0e-4 on those 57 cap edges).
 * Refusals, each with a message that names the way out, under the names mpg_wind_csr_to_mesh / mpg_wind_csr_to_edges.
 * MPG_ERR_UNSUPPORTED: a fixed handle on either side (mpg_wind_to_mesh_dev / mpg_wind_to_edges_dev serve those), a handle with pole
 * terms (mpg_handle_pole_count > 0), MPG_TYPE_BE on either side.  MPG_ERR_INVALID_ARG: NULL handles or arrays, exactly one NULL angle
 * (mesh call), NULL cn_dev / sn_dev (edges call), rh_u.n_dst != rh_v.n_dst, nlev < 1, unknown enums, a level stride below n_src,
 * results aliasing each other, a source or the angles.  MPG_ERR_OVERFLOW: more 64-point blocks than one launch holds. */
int mpg_wind_csr_to_mesh_dev(mpg_handle rh_u, mpg_handle rh_v, const double *cosa_dev, const double *sina_dev, const void *u_dev,
                             const void *v_dev, int src_type, int64_t u_level_stride, int64_t v_level_stride, int nlev, void *ue_dev,
                             void *ve_dev, int dst_type, int dst_layout, void *hip_stream);
int mpg_wind_csr_to_edges_dev(mpg_handle rh_u, mpg_handle rh_v, const double *cn_dev, const double *sn_dev, const void *u_dev,
                              const void *v_dev, int src_type, int64_t u_level_stride, int64_t v_level_stride, int nlev,
                              void *un_dev, void *ut_dev, int dst_type, int dst_layout, void *hip_stream);
/* A wind as a VECTOR through one CSR handle (ESMF 8.6's vectorRegrid): (u, v) at every source point is taken to a Cartesian 3-vector
 * with the source point's local frame, the three components are regridded with the handle's weights, and the result is projected onto
 * the destination point's frame.  Under MPG_POLEMETHOD_ALLAVG a cap point then gets the mean of the row's VECTORS as seen from the cap
 * point, which is a wind (the solid-body case of the caveat above: 6.0e-4 on the 57 cap edges where the two scalar Regrids are off by
 * 0.53; on quad rows 1.88e-3 against 1.41e-3, because the chord of the interpolated position shrinks the vector, as it does in ESMF:
 * the calls stand beside mpg_wind_csr_to_mesh_dev / mpg_wind_csr_to_edges_dev, not in their place).  The weights do not depend on the
 * level, so the three steps fold into one 2 x 2 block per CSR entry, computed once per (handle, frames); the hot path is four fmas and
 * two gathers per entry and level, for every CSR handle: periodic, conservative Grid -> Mesh, conservative Mesh -> Mesh, from-weights.
 * None of the three calls allocates, synchronises with the host or uses atomics: all can be captured in a hipGraph from their first
 * call.  Stream as mpg_regrid_dev.  The calls do not look at the mesh or the grid.
 *
 * mpg_sphere_frames_dev: the frames of n points.  lon_dev / lat_dev [n] float64, radians.  frames_dev [6][n] float64, the planes
 *   D0x D0y D0z D1x D1y D1z.  east = (-sin lon, cos lon, 0), north = (-sin lat cos lon, -sin lat sin lon, cos lat).
 *   c_dev, s_dev both NULL: D0 = east, D1 = north -- earth-relative winds.  Both set ([n] float64): D0 = c east + s north,
 *   D1 = c north - s east, every product and sum rounded (fp contract(off)).  cosa / sina for the grid-relative winds of a Lambert
 *   grid; cos / sin of angleEdge for (normal, tangent) at mesh edges, so that un / ut need no second rotation; what
 *   mpg_mesh_edge_rotang_dev gives to go straight to un / ut of a projected grid.  Exactly one NULL -> MPG_ERR_INVALID_ARG; so are NULL
 *   lon_dev / lat_dev / frames_dev (checked before the n == 0 success), n < 0 and frames aliasing an input.
 *
 * mpg_wind_vector_weights_dev: the blocks of (handle, frames).  src_frames_dev [6][n_src], dst_frames_dev [6][n_dst], m_dev [4][nnz]:
 *   the planes m00 m01 m10 m11 in the handle's CSR entry order (mpg_handle_get_csr); the caller owns m_dev, 4 * nnz doubles with nnz
 *   from mpg_handle_info.  The same bits as numpy: for entry q of row p with c = col[q]
 *     m00 = val[q] * ((e.x*D0.x + e.y*D0.y) + e.z*D0.z)     e  = source D0 at c,  D0 = destination D0 at p
 *     m01 = val[q] * ((n.x*D0.x + n.y*D0.y) + n.z*D0.z)     n  = source D1 at c
 *     m10, m11                                              the same against the destination D1
 *   every operation rounded, nothing contracted.  A handle with no entries is success and writes nothing.
 *
 * mpg_wind_vector_dev: the apply.  The arguments are those of mpg_wind_csr_to_mesh_dev with one handle and m_dev in place of the
 *   angles: u_level_stride / v_level_stride in elements, 0 = dense, below n_src -> MPG_ERR_INVALID_ARG; results in MPG_LAYOUT_CELL_FAST
 *   [lev][point] or MPG_LAYOUT_LEV_FAST [point][lev], fully overwritten.  r1_dev may be NULL: then only r0 is computed and only the
 *   planes m00, m01 are read -- un alone.  Values, a contract by identity, per (point, level):
 *     acc_kl = fma(m_kl[q], (double)src_l[col[q]], acc_kl)    from 0.0, in stored order, whatever LDS chunk an entry arrives in
 *     o0 = fma(acc00, 1.0, 0.0) + fma(acc01, 1.0, 0.0)        src_0 = U, src_1 = V
 *     o1 = fma(acc10, 1.0, 0.0) + fma(acc11, 1.0, 0.0)
 *     store (TD)o0 [, (TD)o1]                                 one rounding to the destination type
 *   o0 is bit for bit mpg_regrid_csr_to_mesh_dev of a from-weights handle with values m00 applied to U, plus the same with m01 applied
 *   to V, both into float64 with scale 1 and offset 0, added once.  An empty row gives (TD)(+0.0).  The same bits for both layouts, for
 *   dense and pitched sources, and from call to call.  n_dst == 0 is success; a handle with no entries gives zeroed results.
 * Refusals, each with a message that names the call and the way out, under the names mpg_sphere_frames / mpg_wind_vector_weights /
 * mpg_wind_vector.  MPG_ERR_UNSUPPORTED: a fixed handle (mpg_handle_get_weights -> mpg_handle_from_weights makes a CSR handle of
 * it), a handle with pole terms (mpg_handle_pole_count > 0), MPG_TYPE_BE on either side.  MPG_ERR_INVALID_ARG: NULL handle or arrays,
 * nlev < 1, unknown enums, a level stride below n_src, results aliasing each other, a source or m_dev.  MPG_ERR_OVERFLOW: more
 * 64-point blocks than one launch holds. */
int mpg_sphere_frames_dev(int64_t n, const double *lon_dev, const double *lat_dev, const double *c_dev, const double *s_dev,
                          double *frames_dev, void *hip_stream);
int mpg_wind_vector_weights_dev(mpg_handle rh, const double *src_frames_dev, const double *dst_frames_dev, double *m_dev,
                                void *hip_stream);
int mpg_wind_vector_dev(mpg_handle rh, const double *m_dev, const void *u_dev, const void *v_dev, int src_type,
                        int64_t u_level_stride, int64_t v_level_stride, int nlev, void *r0_dev, void *r1_dev, int dst_type,
                        int dst_layout, void *hip_stream);
/* Winds FROM the edge-normal u a mesh carries: MPAS's mpas_reconstruct.  Restart, LBC and many init files hold only the prognostic
 * u(nEdges, nVertLevels) and the mesh's coeffs_reconstruct; at cell c
 *     V(k, c) = sum_i coeffs_reconstruct(:, i, c) * u(k, edgesOnCell(i, c))
 * is the Cartesian wind, and its projection on east / north at the cell is uReconstructZonal / uReconstructMeridional.  The
 * coefficients do not depend on the level, so the projection folds into 2 or 3 values per entry of the CSR pattern of edgesOnCell,
 * computed once per (handle, coefficients, frames); the hot path is one gather and nout fmas per entry and level, with col staged once
 * and u gathered once for all results.  The two device calls neither allocate, synchronise with the host nor use atomics: both can be
 * captured in a hipGraph from their first call.  Stream as mpg_regrid_dev.
 *
 * mpg_reconstruct_store: the pattern as an ordinary from-weights CSR handle, n_src = nEdges, n_dst = nx_dst = nCells, ny_dst = 1.
 *   nEdgesOnCell_host [nCells], edgesOnCell_host [nCells][maxEdges] int32 as in the file: ids are 1-based, slots past the count are not
 *   read.  Row c holds the first nEdgesOnCell[c] entries of edgesOnCell[c][0..maxEdges) in the file's slot order, which is the
 *   summation order; every value is 1.0.  A cell with nEdgesOnCell = 0 has an empty row; duplicate edge ids in a row are allowed.  The
 *   handle goes through mpg_handle_from_weights's machinery (always CSR) and every CSR consumer takes it, mpg_handle_get_csr and
 *   mpg_regrid_transpose_dev included.  Not cached: pair it with mpg_handle_release.  The handle keeps its longest row, taken on the
 *   host at Store time.  MPG_ERR_INVALID_ARG with the offending cell: a count outside [0, maxEdges], an id outside [1, nEdges] among
 *   the counted slots; NULL arrays, nCells < 1, nEdges < 1, maxEdges < 0.  MPG_ERR_OVERFLOW: nCells, nEdges or the entries beyond int32.
 *
 * mpg_reconstruct_weights_dev: the values of (handle, coefficients, frames).  coeffs_dev [nCells][maxEdges][3] float64, the file's
 *   coeffs_reconstruct(nCells, maxEdges, R3), padding included.  dst_frames_dev [6][nCells] from mpg_sphere_frames_dev, or NULL.
 *   m_dev [nout][nnz] in the handle's entry order, nout = 2 with frames, 3 without; the caller owns it.  The same bits as numpy, every
 *   operation rounded, nothing contracted (fp contract(off)): for entry q of row c, slot i = q - rowptr[c], (cx, cy, cz) = coeffs[c][i][:]
 *     frames:  m0 = val[q] * ((cx*D0.x + cy*D0.y) + cz*D0.z)      m1: the same against D1
 *     NULL:    m_k = val[q] * c_k                                  k = X, Y, Z
 *   Frames of (lonCell, latCell) with no turn give uReconstructZonal / uReconstructMeridional; frames turned by cosa / sina at the
 *   cells (mpg_mesh_rotang_dev) give grid-relative winds; NULL gives uReconstructX / Y / Z.  A handle without entries is success and
 *   writes nothing.  Refused under the name mpg_reconstruct_weights: MPG_ERR_UNSUPPORTED for a fixed handle and for a handle with pole
 *   terms; MPG_ERR_INVALID_ARG for a handle whose longest row exceeds maxEdges (the message says so; no device read-back is used: the
 *   handle must record its longest row, as those of mpg_reconstruct_store and mpg_handle_from_weights do), NULL arrays, m_dev
 *   aliasing an input.
 *
 * mpg_wind_reconstruct_dev: the apply.  nout is 2 or 3 and r2_dev is non-NULL exactly when nout == 3; nout == 1 is refused
 *   (mpg_regrid_csr_to_mesh_dev / mpg_regrid_csr_rows_dev of a from-weights handle serve one result).  src_layout:
 *   MPG_LAYOUT_LEV_FAST is u[nEdges][nlev], MPAS file order, dense (u_level_stride must be 0); MPG_LAYOUT_CELL_FAST is nlev planes
 *   u_level_stride elements apart, 0 = dense, below n_src -> MPG_ERR_INVALID_ARG.  dst_layout: MPG_LAYOUT_CELL_FAST [lev][cell] or
 *   MPG_LAYOUT_LEV_FAST [cell][lev]; results are fully overwritten.  src_type / dst_type: float32 or float64 in any pairing.
 *   Values, a contract by identity, per (cell, level, k < nout):
 *     acc_k = fma(m_k[q], (double)u[col[q]], acc_k)     from 0.0, the row's entries in stored order, whatever LDS chunk an entry arrives in
 *     store (TD) fma(acc_k, 1.0, 0.0)                   one rounding to the destination type; an empty row gives (TD)(+0.0)
 *   Result k is bit for bit mpg_regrid_csr_to_mesh_dev of a from-weights handle with the values m_k, at scale 1 and offset 0.  The
 *   same bits for all four layout pairs, for dense and pitched sources, and from call to call.  n_dst == 0 is success; a handle
 *   without entries gives zeroed results.
 * Refusals of the apply, each with a message that names the call, under the name mpg_wind_reconstruct.  MPG_ERR_UNSUPPORTED: a fixed
 * handle, a handle with pole terms (mpg_handle_pole_count > 0), MPG_TYPE_BE on either side (mpg_bswap_dev swaps an array in place).
 * MPG_ERR_INVALID_ARG: NULL handle or arrays, nout outside {2, 3}, r2_dev not matching nout, nlev < 1, unknown enums, a non-zero
 * stride with MPG_LAYOUT_LEV_FAST sources, a level stride below n_src, results aliasing each other, the source or m_dev.
 * MPG_ERR_OVERFLOW: more 64-row blocks than one launch holds. */
int mpg_reconstruct_store(int64_t nCells, int64_t nEdges, int maxEdges, const int32_t *nEdgesOnCell_host,
                          const int32_t *edgesOnCell_host, mpg_handle *out);
int mpg_reconstruct_weights_dev(mpg_handle rh, int maxEdges, const double *coeffs_dev, const double *dst_frames_dev,
                                double *m_dev, void *hip_stream);
int mpg_wind_reconstruct_dev(mpg_handle rh, const double *m_dev, int nout, const void *u_dev, int src_type, int src_layout,
                             int64_t u_level_stride, int nlev, void *r0_dev, void *r1_dev, void *r2_dev, int dst_type,
                             int dst_layout, void *hip_stream);

/* ---- handle composition: two Regrids folded into ONE CSR handle ----------------------------------------------------------------------
 * Every operator of this library is a sparse matrix behind a route handle.  A job that needs "A after B" -- edges -> cells -> grid, global
 * grid -> global mesh -> limited-area mesh, a destagger in front of a Grid -> Mesh handle -- pays an intermediate array between two
 * applies, and the rounding of that array.  mpg_handle_compose builds C = A . B on the device (a sparse-matrix x sparse-matrix product with
 * a stated pattern and a stated summation order) as an ordinary CSR handle: every CSR consumer takes it without new apply code
 * (mpg_regrid_typed_dev, mpg_regrid_csr_to_mesh_dev, mpg_regrid_csr_rows_dev, mpg_regrid_masked_dev, mpg_regrid_transpose_dev,
 * mpg_wind_vector_weights_dev, mpg_wind_reconstruct_dev, mpg_handle_get_csr).
 *
 * mpg_handle_compose: A = outer (n_dst_A x n_src_A), B = inner (n_dst_B x n_src_B), n_dst_B == n_src_A.
 *   Shape: n_src = n_src_B; n_dst, nx_dst and ny_dst are those of outer.  Always a CSR handle, method -1 as from-weights handles, not
 *   cached: pair it with mpg_handle_release.  It records its longest row (mpg_reconstruct_weights_dev accepts it).  It owns its arrays:
 *   outer and inner may be released right after the call.  No destination fraction is carried.  The call is blocking: it allocates and
 *   reads the entry count back; mpg_handle_store_ms gives the GPU time of the build.  It orders itself after whatever produced the two
 *   handles, as mpg_handle_get_csr does.
 *   Operands: either may be fixed (3, 4 or 1 slots per row) or CSR.  An entry of a fixed handle with idx = -1 is skipped; a nearest handle
 *   without a weight array has weight 1.0.
 *   Pattern: row i of C holds the distinct source ids reachable from row i of A through the rows of B -- column e appears if at least one
 *   pair (p in A's row i, q in B's row col_A[p]) has col_B[q] == e -- in ascending order.  Entries are structural: one whose value comes
 *   out 0.0 stays.  A row of A that is empty or unmapped gives an empty row of C, and so does a row that reaches only empty rows of B:
 *   Regrid gives 0.0 there, as the chain does.
 *   Values, a contract by identity, bit for bit those of the numpy mirror (target_grid.compose_csr): c[i,e] starts from 0.0; over A's
 *   entries p of row i in stored order, and within each p over B's entries q of row col_A[p] in stored order with col_B[q] == e,
 *     acc = acc + (a_p * b_q)
 *   the product and the sum rounded separately, nothing contracted (fp contract(off)).  Duplicate columns in a row of either operand
 *   are allowed: each occurrence is one term.  The same bytes from run to run: no floating-point atomics, and the result does not depend
 *   on the blocks of destination rows the build works in (mpg_tune "compose_block_rows").
 *   Limits: rows of any length are served (nothing is held per row in LDS).  The temporaries of the pattern are bounded by a fixed byte
 *   budget per block of rows; one row alone may reach at most 2^31 - 2 pairs before de-duplication.
 *   Refusals, each with a message that names the call and the way out.  MPG_ERR_INVALID_ARG: NULL outer, inner or out; n_dst of inner
 *   != n_src of outer (both numbers are printed; a localized or rebased outer fails here).  MPG_ERR_UNSUPPORTED: a handle with pole terms
 *   (mpg_handle_pole_count > 0) on either side.  MPG_ERR_OVERFLOW: a composite of more than 2^31 - 2 entries (rowptr is int32); the
 *   candidate count before de-duplication is a 64-bit quantity and is not what overflows.  A failed allocation returns its error and
 *   leaks nothing.
 *
 * mpg_compose_weights_dev: the same product for caller-owned value planes of B -- how the blocks of mpg_reconstruct_weights_dev or
 *   mpg_wind_vector_weights_dev pass through a composition.  inner_m_dev [nplanes][nnz_B] in inner's CSR entry order; m_dev
 *   [nplanes][nnz_C] in composed's entry order; m_k[i,e] follows the rule above with b_q = inner_m[k][q]; nplanes in 1..4.  It neither
 *   allocates nor synchronises with the host, uses no atomics and can be captured in a hipGraph from its first call.  Memory-safe for any
 *   three handles whose sizes agree: a pair that does not occur contributes nothing.  With nplanes = 1 and inner's own values it writes
 *   exactly composed's values.  A composite without entries is success and writes nothing.  Stream as mpg_regrid_dev.
 *   Refused under the name mpg_compose_weights.  MPG_ERR_UNSUPPORTED: a fixed inner (the planes are defined on CSR entries:
 *   mpg_handle_get_weights, then mpg_handle_from_weights, makes a CSR handle of it), a fixed composed, pole terms on any handle.
 *   MPG_ERR_INVALID_ARG: NULL arguments, nplanes outside 1..4, sizes that do not chain (composed.n_dst != outer.n_dst, composed.n_src !=
 *   inner.n_src, inner.n_dst != outer.n_src), m_dev aliasing inner_m_dev. */
int mpg_handle_compose(mpg_handle outer, mpg_handle inner, mpg_handle *out);
int mpg_compose_weights_dev(mpg_handle composed, mpg_handle outer, mpg_handle inner, int nplanes, const double *inner_m_dev,
                            double *m_dev, void *hip_stream);

/* ---- extrapolation: the unmapped rows of a handle filled from the nearest source points ---------------------------------------------------
 * Every Store maps a destination point only where the source geometry covers it; elsewhere the handle holds idx = -1 or an empty row and
 * every Regrid writes +0.0: the outermost U columns and V rows of the destagger handles, the grid points outside a limited-area mesh, the
 * rim of a mesh under a regional analysis, the cap points of MPG_POLEMETHOD_NONE.  mpg_handle_extrapolate is ESMF_FieldRegridStore's
 * extrapMethod (with extrapNumSrcPnts and extrapDistExponent) as a call of its own: it returns an ordinary handle whose unmapped rows are
 * filled, which every consumer takes; a host that extrapolates its Stores once pays nothing per Regrid.
 *
 * Point sets (mpg_points): exactly one of mesh / grid is non-NULL.  Sources: a mesh's cells (MPG_MESHLOC_ELEMENT, searched through the
 *   mesh's site BVH built whole) or any stagger of any grid (searched through that stagger's point pyramid).  Destinations: any stagger of
 *   a grid, or a mesh's cells, vertices or edges.  One entry point serves Mesh -> Grid, Mesh -> Mesh, Grid -> Mesh and Grid -> Grid.
 * Unmapped row: of a fixed handle, slot 0's index < 0; of a CSR handle, an empty row.  Every other row is copied verbatim.
 * Neighbours of an unmapped destination point p: the candidates are all source points; d2(p, c) is dist2_nofma of the stored unit
 *   vectors, ((dx*dx + dy*dy) + dz*dz) in float64 without contraction (mpg_mesh_get_xyz / mpg_grid_get_xyz export their bits).  The row takes
 *   the K = min(N, n_src) smallest candidates in lexicographic (d2, id) order, N = 1 for MPG_EXTRAPMETHOD_NEAREST_STOD; id is the handle's
 *   source index: the cell id, or j * snx + i.  Ties go to the lower id, at every rank including the last.
 * MPG_EXTRAPMETHOD_NEAREST_STOD: one entry (c0, 1.0).
 * MPG_EXTRAPMETHOD_NEAREST_IDAVG: if d2_0 == 0.0, one entry (c0, 1.0).  Otherwise, for i = 0 .. K - 1 in that order: r_i = d2_0 / d2_i,
 *   t_i = r_i when e == 2.0, else pow(r_i, 0.5 * e); S = ((t_0 + t_1) + ...) from left to right; w_i = t_i / S.  Every operation is rounded
 *   on its own (fp contract(off)).  This is ESMF's (1/d^e) / sum(1/d^e) with the nearest distance divided out: nothing overflows, and a
 *   far neighbour may underflow to weight 0.  The entries are stored in ascending (d2, id) order, which is the Regrid's summation order.
 *   A contract by identity with the numpy mirror target_grid.extrapolate_rows for e == 2.0; for other exponents up to the device pow.
 * Output: a new handle with the input's n_src, n_dst, nx_dst, ny_dst and method.  It is not cached and owns its arrays: pair it with
 *   mpg_handle_release; rh may be released right after the call.  It carries no dst_frac.  mpg_handle_store_ms is the GPU time of the call;
 *   mpg_handle_store_stats [1] is the number of rows filled, [2] is K.
 *   Fixed output: a fixed input of S slots stays fixed when every new row fits: STOD always, IDAVG when N <= S.  A new row puts its
 *   entries in slots 0 .. k - 1; every remaining slot repeats entry 0's id with weight +0.0.  A nearest handle without a weight array
 *   stays without one.  (This keeps a filled bilinear Mesh -> Grid handle on the staged kernels.)
 *   CSR output: otherwise.  A mapped row of a fixed input becomes its S slots in slot order with their weights (a slot without an index is
 *   dropped; a nearest handle has weight 1.0); a mapped row of a CSR input is its entries in stored order.  The longest row is recorded.
 *   Nothing unmapped is success: a copy of the pattern.  A source set without points fills nothing.
 * Determinism: the same bytes from run to run; no floating-point atomics.
 * Blocking: the call allocates, reads the count of unmapped rows back, and drains the Store worker first (it may build a grid's pyramid
 *   or a mesh's BVH).  It orders itself after whatever produced rh, as mpg_handle_get_csr does.
 * Refusals, each with a message that names mpg_handle_extrapolate and the way out.  MPG_ERR_INVALID_ARG: a NULL argument; both or neither
 *   of mesh / grid set in a point set; an unknown method; N outside 1..MPG_EXTRAP_MAX_PNTS; e not finite or <= 0; rh's n_src differs from
 *   the source set's size (both numbers are printed; a node-located handle fails here); rh's n_dst, nx_dst or ny_dst differ from the
 *   destination set (both are printed); a source mesh location other than ELEMENT; a destination MPG_MESHLOC_EDGE on a mesh without edges;
 *   a stagger without coordinates.  MPG_ERR_UNSUPPORTED: a handle with pole terms (mpg_handle_pole_count > 0); a localized or rebased
 *   handle; a source mesh that carries a source window.  MPG_ERR_OVERFLOW: a CSR output of more than 2^31 - 2 entries.  A failed
 *   allocation returns its error and leaks nothing. */
enum { MPG_EXTRAPMETHOD_NEAREST_STOD = 1, MPG_EXTRAPMETHOD_NEAREST_IDAVG = 2 };
#define MPG_EXTRAP_MAX_PNTS 8
typedef struct mpg_points {      /* a point set: exactly one of mesh / grid is non-NULL */
  mpg_mesh mesh; int meshloc;    /* MPG_MESHLOC_* */
  mpg_grid grid; int staggerloc; /* MPG_STAGGERLOC_* */
} mpg_points;
typedef struct mpg_extrap_opts {
  int method;            /* MPG_EXTRAPMETHOD_* */
  int num_src_pnts;      /* IDAVG: N in 1..MPG_EXTRAP_MAX_PNTS (ESMF's default 8); ignored for STOD */
  double dist_exponent;  /* IDAVG: e, finite and > 0 (ESMF's default 2.0); ignored for STOD */
} mpg_extrap_opts;
int mpg_handle_extrapolate(mpg_handle rh, const mpg_points *src, const mpg_points *dst, const mpg_extrap_opts *opts, mpg_handle *out);

/* ---- Store-time masks: ESMF_FieldRegridStore's srcMaskValues / dstMaskValues as two handle-to-handle calls ---------------------------------
 * Land values must not be made from water cells: a land point of the target takes the nearest LAND cell, a conservative mean is taken over
 * the land part of a cell.  Masks that do not change from call to call belong into the handle: mpg_handle_mask removes masked sources and
 * destinations from a finished handle's pattern, mpg_handle_extrapolate_masked refills rows from the UNMASKED sources alone.  Both return
 * an ordinary handle which every consumer takes, so every Store and every Regrid is served at once and a host that masks its Stores once
 * pays nothing per Regrid.  (mpg_regrid_masked_dev is the other thing: masks that change per call, renormalised per call on the weights of
 * the unmasked Store, never a search for the next valid neighbour.)  Masks are device bytes, non-zero = masked.
 *
 * mpg_handle_mask(rh, opts, out): static masks on a handle's pattern.  It needs no geometry.
 *   src_mask_dev [n_src] in the handle's source index space, dst_mask_dev [n_dst]; either may be NULL (no mask on that side); both NULL is
 *   success: a copy of the pattern.
 *   Destination mask: a masked destination row becomes unmapped, under either rule.
 *   MPG_MASKRULE_ROW (ESMF's rule for bilinear and nearest: a source cell with a masked corner is masked): a row with at least one stored
 *     entry (index >= 0, whatever its weight, a weight of 0.0 included) that references a masked source becomes unmapped; every other row is
 *     copied verbatim.  Fixed and CSR handles are served.  The cap rows of a periodic Grid -> Mesh CSR handle (MPG_POLEMETHOD_NONE's or
 *     ALLAVG's rows of nx entries) are rows like any other: one masked point of the end row unmaps them.  A fixed input stays fixed with the
 *     same slot count, a nearest handle stays without a weight array, and an unmapped row is written as the Stores write one: every slot's
 *     index -1, every weight +0.0.  A CSR input stays CSR: unmapped rows are empty.
 *   MPG_MASKRULE_ENTRY (ESMF's rule for conservative: masked source cells do not take part), CSR handles only: the entries of masked
 *     sources are removed, the kept entries stay in stored order.  Wk = ((0.0 + v_0) + v_1) + ... over the kept values from left to right,
 *     each add rounded on its own (fp contract(off)).  MPG_NORM_DSTAREA: the values are unchanged and frac' = Wk.  MPG_NORM_FRACAREA:
 *     w' = w / Wk and frac' = frac * Wk.  norm_type is the one the Store was called with.  A row with nothing kept, or with Wk <= 0 (or
 *     NaN), is empty and frac' = +0.0.  A row with no masked entry is copied verbatim, its dst_frac included, bit for bit.  A
 *     destination-masked row is empty with frac' = +0.0.  An input without dst_frac gives an output without one (frac reads as 0.0 in the
 *     rule and frac' is dropped); under MPG_MASKRULE_ROW a dst_frac is carried, +0.0 on the rows the call unmaps.
 *   MPG_MASKRULE_AUTO: ROW for handles whose method is MPG_REGRIDMETHOD_BILINEAR or MPG_REGRIDMETHOD_NEAREST_STOD, ENTRY for
 *     MPG_REGRIDMETHOD_CONSERVE.  Where the handle records no method (from weights, composed, reconstruct): MPG_ERR_INVALID_ARG, the message
 *     asks for an explicit rule.
 *   Output: a new handle with the input's n_src, n_dst, nx_dst, ny_dst, method and kind.  It is not cached and owns its arrays: pair it
 *     with mpg_handle_release; rh may be released right after the call.  A CSR output records its longest row.  mpg_handle_store_ms is the
 *     GPU time of the call.  mpg_handle_store_stats: [1] = mapped rows (a stored entry) the source rule unmapped, [2] = mapped rows the
 *     destination mask unmapped (a row under both counts here), [3] = stored entries removed (the input's minus the output's).
 *     A contract by identity with the numpy mirror target_grid.mask_rows.  The same bytes from run to run; no floating-point atomics.
 *   Blocking: the call allocates, reads its counts back and drains the Store worker first.  It orders itself after whatever produced rh, as
 *     mpg_handle_get_csr does.
 *   Refusals, each with a message that names mpg_handle_mask and the way out.  MPG_ERR_INVALID_ARG: a NULL rh, opts or out; an unknown rule;
 *     under ENTRY an unknown norm_type; AUTO on a handle without a method.  MPG_ERR_UNSUPPORTED: a handle with pole terms
 *     (mpg_handle_pole_count > 0); a localized or rebased handle; a handle whose mesh carries a source window; ENTRY on a fixed handle
 *     (mpg_handle_get_weights -> mpg_handle_from_weights makes a CSR handle of it).  The output never has more entries than the input:
 *     there is no overflow refusal.  A failed allocation returns its error and leaks nothing.
 *
 * mpg_handle_extrapolate_masked(rh, src, dst, opts, src_mask_dev, dst_skip_dev, out): the contract of mpg_handle_extrapolate above, word
 *   for word, with two changes.  First, the candidates are the sources c with src_mask[c] == 0, and K = min(N, number of unmasked
 *   sources).  Second, an unmapped row with dst_skip[p] != 0 is left unmapped.  The (d2, id) order is the same: ties go to the lower
 *   UNMASKED id at every rank; knn_weights and the fixed-or-CSR output rule are the same.  Either pointer may be NULL; with both NULL the
 *   output bytes equal mpg_handle_extrapolate's.  With every source masked nothing is filled: that is success.
 *   mpg_handle_store_stats: [1] = rows filled, [2] = K, [3] = unmasked sources.  A contract by identity with the numpy mirror
 *   target_grid.extrapolate_rows_masked (for e == 2.0; for other exponents up to the device pow).
 *   The search never enters a subtree that holds no unmasked source: per call one `alive` byte per tree node is built bottom-up (a leaf
 *   is alive if it holds an unmasked item, a parent if a child is) and the walk sees a dead node as absent; without that a query would walk
 *   the whole tree while fewer than K unmasked sources have been met.  The boxes stay valid lower bounds, so the result is exact.
 *   Refusals: those of mpg_handle_extrapolate, each message under the name mpg_handle_extrapolate_masked.
 *
 * ESMF's masked Store is the composition mask, then extrapolate_masked: regrid.store_masks (Python), INTEGRATION.md.
 * Not served: handles with pole terms, localized or windowed handles, node-located sources, creep fills. */
enum { MPG_MASKRULE_AUTO = 0, MPG_MASKRULE_ROW = 1, MPG_MASKRULE_ENTRY = 2 };
typedef struct mpg_store_mask_opts {
  const uint8_t *src_mask_dev;  /* [n_src] device bytes in the handle's index space, non-zero = masked; NULL = none */
  const uint8_t *dst_mask_dev;  /* [n_dst] device bytes, non-zero = masked; NULL = none */
  int rule;                     /* MPG_MASKRULE_* */
  int norm_type;                /* ENTRY rule only: MPG_NORM_DSTAREA / MPG_NORM_FRACAREA, the one the Store was called with */
} mpg_store_mask_opts;
int mpg_handle_mask(mpg_handle rh, const mpg_store_mask_opts *opts, mpg_handle *out);
int mpg_handle_extrapolate_masked(mpg_handle rh, const mpg_points *src, const mpg_points *dst, const mpg_extrap_opts *opts,
                                  const uint8_t *src_mask_dev, const uint8_t *dst_skip_dev, mpg_handle *out);

/* ---- patch regridding: second-degree patch recovery as a CSR handle -------------------------------------------------------------------------
 * ESMF_REGRIDMETHOD_PATCH, the method the reference names its main route handle after (rh_patch, interp.F90:123,207) and then stores
 * bilinearly.  mpg_handle_patch turns a finished bilinear handle into a patch handle: per source node a second-degree polynomial is fitted
 * by least squares through the node's neighbours, per destination point the polynomials of its bilinear row's nodes are blended with the
 * bilinear weights.  Third-order fields at rows of about 12 entries instead of 3.  The result is an ordinary CSR handle, which every
 * consumer takes; the call needs no new search and serves Mesh -> Grid, Mesh -> Mesh, Grid -> Mesh and Grid -> Grid at once.
 *
 * rh: a fixed bilinear handle of S = 3 or 4 slots (mpg_regrid_store from elements, mpg_regrid_store_mesh, mpg_regrid_store_to_mesh,
 *   mpg_regrid_store_grid).  src / dst: the point sets the handle was stored between, by the mpg_points rules and size checks of
 *   mpg_handle_extrapolate (sources: a mesh's cells or a grid stagger).
 * The rule.  Every operation is rounded on its own (fp contract(off)); the only operations are + - * / sqrt.
 *   Unit vectors: X is the stored unit vector of a point, the bits mpg_mesh_get_xyz / mpg_grid_get_xyz export.
 *   Ring-1 patch of a source node c, N1(c), in ascending id.  Mesh cells: c together with the three cells of every valid dual triangle
 *     (mpg_mesh_get_triangles: no -1 in its column) of every listed vertex of c (the non-zero entries of c's verticesOnCell row).  Grid
 *     stagger of snx x sny points, id = j * snx + i: the window [i0, i0 + 2] x [j0, j0 + 2] cut to the grid, i0 = clamp(i - 1, 0,
 *     max(snx - 3, 0)), j0 likewise: border nodes keep a full 3 x 3 block.
 *   Ring-2 patch, meshes only: N2(c) = the union of N1(d) over d in N1(c), in ascending id.
 *   A patch is used only when it holds at most MPG_PATCH_MAX_PNTS points (N1 as well as N2).
 *   Local coordinates about c: n = X_c; a = the unit axis of n's smallest |component|, the lowest axis on ties; t = a - (a . n) n;
 *     e1 = t / sqrt(t . t); e2 = n x e1 = (n_y e1_z - n_z e1_y, n_z e1_x - n_x e1_z, n_x e1_y - n_y e1_x).  For a point q: d = X_q - X_c,
 *     h = sqrt(max over the patch of d . d), u = (d . e1) / h, v = (d . e2) / h; the destination point p is mapped the same way (an
 *     orthographic projection).  Dot products are (x*x' + y*y') + z*z'.
 *   The fit: phi = (1, u, v, u*u, u*v, v*v) for degree 2, (1, u, v) for degree 1.  G = sum_k phi(q_k) phi(q_k)^T, every element summed in
 *     patch order from 0.0.  G = R^T R by a Cholesky with left-to-right inner products: for k = 0, 1, ...: s_k = G_kk - R_0k R_0k - ... -
 *     R_(k-1)k R_(k-1)k, R_kk = sqrt(s_k), and for j > k: R_kj = (G_kj - R_0k R_0j - ... - R_(k-1)k R_(k-1)j) / R_kk, each subtraction
 *     in that order.  An attempt passes when h > 0 and every pivot s_k > 2^-26 * G_kk: a definition, not a tuning constant.
 *   Attempts, in this order: (A) degree 2 on N1 if |N1| >= 6; (B) degree 2 on N2, on a mesh with 6 <= |N2| <= MPG_PATCH_MAX_PNTS;
 *     (C) degree 1 on N1 if |N1| >= 3; (D) degree 0: the node itself with value 1.  The attempt is a property of the node alone.
 *   Shape values: R^T z = phi(p) by forward substitution (z_k = (phi_k - R_0k z_0 - ... - R_(k-1)k z_(k-1)) / R_kk), R y = z by back
 *     substitution (y_k = (z_k - R_k(k+1) y_(k+1) - ... ) / R_kk, the terms in ascending column order); L_k = sum_a phi_a(q_k) * y_a from
 *     0.0 in basis order.
 *   A row: for a mapped destination point with slots (c_s, b_s), s = 0 .. S - 1, every slot with an index >= 0 takes part, whatever its
 *     weight.  The row's columns are the distinct ids of the slots' patches, in ascending order; a column's value is acc = acc + (b_s *
 *     L_(s,k)) from 0.0 over (slot, patch position) in ascending order.  Zero values stay in the row: the pattern does not depend on the
 *     values.  An unmapped row (slot 0's index < 0) is empty.
 *   A contract by identity with the numpy mirror target_grid.patch_rows; mpassit_amd/csrc/patch.h is the arithmetic, for device and host.
 * Output: a new CSR handle with the input's n_src, n_dst, nx_dst and ny_dst; its method is MPG_REGRIDMETHOD_PATCH.  It has no dst_frac; its
 *   longest row is recorded.  It is not cached and owns its arrays: pair it with mpg_handle_release; rh may be released right after the
 *   call.  mpg_handle_store_ms is the GPU time of the call.  mpg_handle_store_stats: [1] is the number of rows written, [2] .. [5] are the
 *   (row, slot) pairs served by attempts A, B, C and D, [6] is the longest row.
 * Determinism: the same bytes from run to run; no floating-point atomics.
 * Blocking: the call allocates, reads the entry count back (its only host round trip) and drains the Store worker first.  It orders itself
 *   after whatever produced rh, as mpg_handle_get_csr does.
 * Order with the other handle calls: patch first, then mpg_handle_mask / mpg_handle_extrapolate (a polynomial evaluated far outside its
 *   patch is not an extrapolation).  MPG_MASKRULE_AUTO picks MPG_MASKRULE_ROW for method MPG_REGRIDMETHOD_PATCH.  The Stores go on refusing
 *   method 3.
 * Refusals, each with a message that names mpg_handle_patch and the way out.  MPG_ERR_INVALID_ARG: a NULL argument; a point set that
 *   breaks the mpg_points rules; sizes that differ from the handle's (both numbers are printed); a source mesh location other than
 *   ELEMENT; a handle whose method is not MPG_REGRIDMETHOD_BILINEAR.  MPG_ERR_UNSUPPORTED: a CSR or 1-slot handle; a handle with pole terms
 *   (mpg_handle_pole_count > 0); a localized or rebased handle; a handle whose mesh carries a source window; a mesh of
 *   mpg_mesh_create_window; a source grid with MPG_GRID_PERIODIC_I.  MPG_ERR_OVERFLOW: more than 2^31 - 2 entries.  A failed allocation
 *   returns its error and leaks nothing.
 * Not served: periodic sources, node-located sources, CSR inputs, a _begin variant, caching. */
#define MPG_PATCH_MAX_PNTS 32
int mpg_handle_patch(mpg_handle rh, const mpg_points *src, const mpg_points *dst, mpg_handle *out);

/* ---- second-order conservative regridding: a linear reconstruction inside every source cell, as a CSR handle ------------------------------
 * ESMF_REGRIDMETHOD_CONSERVE_2ND.  The first-order conservative Stores treat a source cell as a constant: precipitation, snow, soil water
 * or a tracer remapped onto a finer mesh or grid comes out in staircases of source-cell size.  mpg_handle_conserve2nd turns a finished
 * first-order conservative handle into a second-order one: every source cell carries a least-squares gradient over its neighbours' means,
 * and every stored (destination, source) piece is evaluated at the piece's own centroid.  The integral is kept as the first-order handle
 * keeps it; smooth fields are second-order accurate.  The result is an ordinary CSR handle, which every consumer takes; the call needs no
 * new search -- the stored pairs are the candidate list -- and serves Mesh -> Grid, Grid -> Mesh and Mesh -> Mesh at once.
 *
 * rh: a conservative CSR handle of mpg_regrid_store(..., MPG_REGRIDMETHOD_CONSERVE), mpg_regrid_store_conserve_to_mesh or
 *   mpg_regrid_store_conserve_mesh, also after mpg_handle_mask.  src / dst: the point sets the handle was stored between, by the mpg_points
 *   rules; a mesh side takes part with its cells (meshloc MPG_MESHLOC_ELEMENT), a grid side with its cells (staggerloc
 *   MPG_STAGGERLOC_CENTER; the cells are the quadrilaterals of its CORNER points).  opts->norm_type: the one the Store was called with.
 *   opts->src_mask_dev: optional device bytes [n_src] in the handle's source index space, non-zero = masked.
 * The rule is ours, built from this header's primitives as the patch rule is; ESMF's Green's-theorem gradient is not reproduced.  Every
 * operation is rounded on its own (fp contract(off)); the only operations are + - * / sqrt.  Dot products are (x*x' + y*y') + z*z'.
 *   Triangle area: the signed area of the spherical triangle a, b, c is tri(a, b, c): num = a . ((b - a) x (c - a)), den = ((1 + a . b) +
 *     b . c) + c . a (sph_tri_area's two numbers); x = num / den; while |x| >= 2^-10: x = x / (1 + sqrt(1 + x * x)), at most 64 times,
 *     h counting the steps; tri = 2^(h + 1) * (x * (1 - x2 * (1/3 - x2 * (1/5 - x2 * (1/7))))) with x2 = x * x.  den <= 0 gives 0.  The
 *     half-angle steps stand where sph_tri_area calls atan2: a library function has its library's bits, this form has the same bits
 *     everywhere (it agrees with sph_tri_area to a few units in the last place).
 *   1. Polygons.  A mesh cell is its non-zero verticesOnCell entries in listed order.  A grid cell is the four CORNER points around centre
 *     (i, j) -- (i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1) -- with id = j * nx + i.  The fan area of a polygon is the sum from 0.0 of
 *     tri(p_0, p_t, p_(t+1)), t = 1 .. n - 2; a polygon is made counter-clockwise by the sign of its own fan area (the listed order
 *     reversed when that is negative).  The source cell is the subject polygon; it is clipped by the destination cell's sides in listed
 *     (counter-clockwise) order, the closing side last.  Everything else follows the Mesh -> Mesh Store's contract word for word: normals
 *     a x (b - a), the 1e-15 * |n| inside rule, and the rule that a side with |b - a|^2 < 1e-24 bounds nothing.  This one clip rule serves
 *     all three pairings; the areas it gives may differ from the input handle's in the last bits.
 *   2. Piece (j, i) of every stored entry q.  a_t = tri(p_0, p_t, p_(t+1)) over the clipped polygon's fan from slot 0; A_q = the sum of the
 *     a_t from 0.0, clamped at 0; the moment m_q = sum_t a_t * (((p_0 + p_t) + p_(t+1)) / 3) from 0.0, per component.  A polygon of fewer
 *     than three vertices has A_q = 0, m_q = 0.  area(d) is |fan area| of the destination polygon in listed order.
 *   3. Source cell i.  A_i = sum A_q and M_i = sum m_q over its pieces, from 0.0 in ascending destination id (the handle's transposed
 *     index).  The geometric centroid G_i is the unit vector m / sqrt(m . m) of the counter-clockwise cell polygon's own fan moment m; it
 *     is the stored cell centre when the polygon has fewer than 3 vertices or sqrt(m . m) is not > 0.  The frame (e1, e2) is the patch
 *     rule's frame about n = G_i.
 *   4. Stencil.  S(i) = N1(i) as mpg_handle_patch defines it (mesh cells; the CENTER stagger of a grid), minus i, minus the cells flagged
 *     in src_mask_dev (ESMF's rule: masked cells take no part in a gradient).  d_k = ((G_k - G_i) . e1, (G_k - G_i) . e2).  M = sum_k d_k
 *     d_k^T, every element from 0.0 in ascending k.  The stencil passes when |S| >= 2, |N1| <= MPG_PATCH_MAX_PNTS, i is not masked, and
 *     det = M00 * M11 - M01 * M01 > 2^-26 * (M00 * M11).  On a pass b_k = ((M11 * dx - M01 * dy) / det, (M00 * dy - M01 * dx) / det) and
 *     b_i = -(sum_k b_k), the sum from 0.0 in ascending k; the stencil's entries are S(i) and i, ascending.  A stencil that fails has the
 *     single entry i with b = 0: that source stays first order.
 *   5. Offsets and weights.  delta_q = ((m_q / A_q - M_i / A_i) . e1, ( ... ) . e2), per component a division, a division and a
 *     subtraction; 0 when A_q <= 0 or A_i <= 0.  MPG_NORM_DSTAREA: w_q = A_q / area(d).  MPG_NORM_FRACAREA: w_q = A_q / (sum over the row of
 *     A_q from 0.0 in stored order).  A divisor that is not > 0 gives w_q = 0.
 *   6. Row j.  Its columns are the ascending distinct union of the stencils of the row's source cells: exactly the pattern of
 *     mpg_handle_compose(rh, the stencils as a CSR matrix).  The value of column e is acc = acc + (w_q * t) from 0.0 over the row's entries
 *     q in stored order whose stencil holds e (each holds it at most once): g = (dx * bx) + (dy * by) with delta_q = (dx, dy) and the
 *     stencil entry's b = (bx, by); t = 1.0 + g when e is the entry's own source cell, else t = g.  Zero values stay in the row.  An empty
 *     input row stays empty.  A dst_frac is carried over bit for bit.
 *   Two identities make this the right rule (DESIGN.md s4.2 proves them; both hold up to rounding).  Conservation: sum_j area(d_j) * c_(j,e)
 *     = A_e under MPG_NORM_DSTAREA -- the integral over the covered part is kept exactly as the first-order handle keeps it, for any field,
 *     partly covered source cells included -- because sum_q A_q delta_q = 0 over the pieces of a source cell by the construction of
 *     M_i / A_i.  Row sums: every row's sum equals the first-order row sum, because sum_k b_k = 0 over a stencil.
 *   The price: weights can be negative, so over- and undershoots occur and there is no limiter; a partly covered source cell expands about
 *     the centroid of its covered part, so the rim is only first-order accurate.
 *   A contract by identity with the numpy mirror target_grid.conserve2nd_rows; mpassit_amd/csrc/conserve2nd.h is the arithmetic, for
 *   device and host.
 * Output: a new CSR handle with the input's n_src, n_dst, nx_dst and ny_dst; its method is MPG_REGRIDMETHOD_CONSERVE_2ND.  Its longest row
 *   is recorded.  It is not cached and owns its arrays: pair it with mpg_handle_release; rh may be released right after the call.
 *   mpg_handle_store_ms is the GPU time of the call.  mpg_handle_store_stats: [1] pairs clipped, [2] sources with a passing stencil,
 *   [3] sources without one, [4] stencil entries, [6] the longest row.
 * Determinism: the same bytes from run to run; no floating-point atomics.
 * Blocking: the call allocates, builds rh's transposed index if it is absent (as mpg_regrid_transpose_dev does), reads the stencils'
 *   entry count back (its own host round trip; the pattern's row blocks add theirs, mpg_tune("compose_block_rows") covers them) and drains
 *   the Store worker first.  It orders itself after whatever produced rh, as mpg_handle_get_csr does.
 * Order with the other handle calls: mask the first-order handle with MPG_MASKRULE_ENTRY (mpg_handle_mask, the Store's norm_type), then
 *   call this with the same source mask.  mpg_handle_mask is unchanged: MPG_MASKRULE_AUTO refuses method 4, which it does not know.
 * Refusals, each with a message that names mpg_handle_conserve2nd and the way out.  MPG_ERR_INVALID_ARG: a NULL argument; a point set that
 *   breaks the mpg_points rules, a mesh location other than ELEMENT or a stagger other than CENTER; sizes that differ from the handle's
 *   (both numbers are printed); an unknown norm_type; a handle whose method is not MPG_REGRIDMETHOD_CONSERVE; a grid without CORNER
 *   coordinates.  MPG_ERR_UNSUPPORTED: a fixed handle; a handle with pole terms; a localized, rebased or windowed handle; a mesh of
 *   mpg_mesh_create_window; maxEdges > 12; a source grid with MPG_GRID_PERIODIC_I (the rings do not wrap).  MPG_ERR_OVERFLOW: more than
 *   2^31 - 2 entries; a clipped polygon that outgrew its slots (a non-convex cell).  A failed allocation returns its error and leaks nothing.
 * Not served: ESMF's own gradient; a limiter; periodic source grids and pole terms; node-located fields; caching or a _begin variant;
 *   multi-GPU sharding; use from interp.py or the Fortran driver; a pin-kit export for -m conserve2nd. */
enum { MPG_REGRIDMETHOD_CONSERVE_2ND = 4 };   /* the method of mpg_handle_conserve2nd's handles; no Store takes it */
typedef struct mpg_conserve2nd_opts {
  int norm_type;                /* MPG_NORM_DSTAREA / MPG_NORM_FRACAREA, the one the Store was called with */
  const uint8_t *src_mask_dev;  /* [n_src] device bytes in the handle's index space, non-zero = masked; NULL = none */
} mpg_conserve2nd_opts;
int mpg_handle_conserve2nd(mpg_handle rh, const mpg_points *src, const mpg_points *dst, const mpg_conserve2nd_opts *opts, mpg_handle *out);

/* ---- creep-fill extrapolation: the unmapped rows of a handle filled level by level from their neighbours' rows ------------------------------
 * ESMF_EXTRAPMETHOD_CREEP with extrapNumLevels, the one value of ESMF_FieldRegridStore's extrapMethod that mpg_handle_extrapolate does not
 * take (this section supersedes the "creep fills" remark that ends the Store-time-mask section above; mpg_handle_extrapolate, its enum
 * and its refusals are unchanged, which is why this is a call of its own).  The nearest-source fill jumps between neighbouring points,
 * reaches arbitrarily far and ignores the interpolation that was just stored.  A creep fill continues the mapped field outward: every
 * newly filled point takes the average of its already filled neighbours, repeated for a number of levels -- the grid points just outside
 * a limited-area mesh, the rim of a mesh under a regional analysis, SST and soil fields carried a few points across a coastline.  It is a
 * pure handle-to-handle transform: the new row of a filled point is the average of its neighbours' rows.  It needs no source geometry
 * and no search, only the destination's connectivity, and it returns an ordinary CSR handle, which every consumer takes.
 * ESMF_EXTRAPMETHOD_CREEP_NRST_D is this call followed by mpg_handle_extrapolate with MPG_EXTRAPMETHOD_NEAREST_STOD for what is left
 * (regrid.creep_nearest in Python).  Masks are served this way: mpg_handle_mask first, then mpg_handle_creep with dst_skip_dev = the
 * destination mask.
 *
 * rh: any handle without pole terms, fixed or CSR.  dst: the destination point set rh was stored onto, by the mpg_points rules and size
 *   checks of mpg_handle_extrapolate: any stagger of a grid, or a mesh's cells.  No source set is given: none is read.
 * The rule.  A contract by identity with the numpy mirror target_grid.creep_rows; mpassit_amd/csrc/creep.h is the arithmetic, for
 *   device and host.  Every operation is rounded on its own (fp contract(off)); the only operations are + and /.
 *   Rows.  An unmapped row is as mpg_handle_extrapolate defines it: of a fixed handle, slot 0's index < 0; of a CSR handle, an empty row.
 *     Every mapped row is copied verbatim by that section's CSR-output rule: a fixed row's slots in slot order, -1 slots dropped, weight
 *     1.0 for a nearest handle without a weight array; a CSR row's entries in stored order.
 *   Neighbours Nb(p) of a destination point p, in ascending id, p itself excluded.  Any stagger of a grid with snx x sny points,
 *     id = j * snx + i: the points of [i - 1, i + 1] x [j - 1, j + 1] that lie inside the grid, up to 8; this is NOT the shifted 3 x 3
 *     window of the patch rule, and there is no wrap.  A mesh's cells (MPG_MESHLOC_ELEMENT): N1(p) as mpg_handle_patch defines it, minus
 *     p -- the cells that share a valid dual triangle with p, i.e. the node neighbours of ESMF's dual mesh.  A mesh of bare centres (no
 *     verticesOnCell entries) has no neighbours: nothing is filled, and that is success.
 *   Levels.  level[p] = 0 for a mapped row.  An unmapped row with dst_skip[p] != 0 never gets a level: it is never filled and never a
 *     neighbour.  For L = 1, 2, ... up to num_levels: an unmapped, unskipped p without a level gets level L iff some q in Nb(p) has
 *     level[q] == L - 1.  The loop ends early at the first L that assigns nothing.  A skipped row that is mapped keeps its row and is
 *     level 0: dst_skip only stops filling.
 *   Row of a point of level L >= 1.  The contributors are Q = { q in Nb(p) : level[q] == L - 1 }, ascending, m = |Q| >= 1.  The columns
 *     are the ascending distinct union of the contributors' columns.  The value of column e is acc = acc + v from 0.0, the sum running
 *     over the contributors in ascending id and within a contributor over its entries with column e in stored order; then
 *     w = acc / (double)m.  Zero values stay in the row: the pattern does not depend on the values.  Duplicate columns in a mapped input
 *     row are one term each.
 *   Two consequences.  With m = 1 the row is that neighbour's row with its columns sorted and merged, and values that appear once are
 *     copied exactly.  Chain identity: creep(creep(h, a), b) has the bytes of creep(h, a + b).
 *   Row sums are kept up to rounding: a column's value is a sum of k terms and one division, so with weights of one sign a filled row's
 *     sum differs from the average of its contributors' sums by at most k * 2^-53 relative per level -- k <= 8 on a grid whose mapped
 *     rows hold no duplicate column; with m = 1 and no duplicate column the row is an exact copy.
 * Output: always a new CSR handle with the input's n_src, n_dst, nx_dst, ny_dst and method.  It has no dst_frac; its longest row is
 *   recorded.  It is not cached and owns its arrays: pair it with mpg_handle_release; rh may be released right after the call.
 *   mpg_handle_store_ms is the GPU time of the call.  mpg_handle_store_stats: [1] rows filled, [2] the last level that filled a row,
 *   [3] rows still unmapped (skipped ones included), [6] the longest row.  Nothing unmapped is success: a CSR copy of the pattern.
 * Determinism: the same bytes from run to run; no floating-point atomics; the one sort is stable.  There is no blocking knob: rows of any
 *   length take the same path.
 * Blocking: the call allocates, drains the Store worker first, orders itself after whatever produced rh (as mpg_handle_get_csr does)
 *   and reads counts back: once before the first level, twice per level (the front's size with its candidates, then the level's
 *   entries), once for the output's entry count.
 * Refusals, each with a message that names mpg_handle_creep and the way out.  MPG_ERR_INVALID_ARG: a NULL rh, dst, opts or out; a point
 *   set that breaks the mpg_points rules; num_levels < 1; rh's n_dst, nx_dst or ny_dst differ from the destination set (both are printed).
 *   MPG_ERR_UNSUPPORTED: a destination MPG_MESHLOC_NODE or MPG_MESHLOC_EDGE (no ring is defined there); a mesh of
 *   mpg_mesh_create_window; maxEdges > 12; a destination grid with MPG_GRID_PERIODIC_I (the seam would be a wall); a handle with pole
 *   terms (mpg_handle_pole_count > 0); a localized, rebased or windowed handle.  MPG_ERR_OVERFLOW: more than 2^31 - 2 entries in the
 *   output, or among the candidate entries of one level (the contributors' rows before they are merged).  A failed allocation returns
 *   its error and leaks nothing.
 * Not served: vertices and edges; periodic destinations; distance-weighted averages; a fixed-handle output; caching or a _begin variant;
 *   multi-GPU sharding; use from interp.py or the Fortran driver. */
enum { MPG_CREEP_ALL_LEVELS = 0x7fffffff };
typedef struct mpg_creep_opts {
  int num_levels;               /* ESMF's extrapNumLevels: >= 1; MPG_CREEP_ALL_LEVELS = until no row is filled any more */
  const uint8_t *dst_skip_dev;  /* [n_dst] device bytes, non-zero = never filled and never a neighbour; NULL = none */
} mpg_creep_opts;
int mpg_handle_creep(mpg_handle rh, const mpg_points *dst, const mpg_creep_opts *opts, mpg_handle *out);

/* ---- Grid -> Grid between two grids: ESMF_FieldRegridStore(srcField on a Grid stagger, dstField on a stagger of another Grid) -- a GFS /
 * ERA5 lat-lon analysis onto the Lambert target grid, a parent domain onto its nest and the nest back onto the parent, the target grid's
 * results onto a lat-lon verification grid, precipitation moved conservatively between two regular grids -- without a detour through a
 * mesh.  mpg_regrid_store_grid above stays the destaggering Store of ONE grid.
 * Common to both calls.  Sources: the snx x sny points of src_staggerloc of `src`, source index = j * snx + i, n_src = snx * sny.
 *   Destinations: the points of dst_staggerloc of `dst`, dnx x dny of them; any stagger whose coordinates the grid holds, CORNER
 *   included.  mpg_handle_info reports n_dst = dnx * dny, nx_dst = dnx, ny_dst = dny: every Regrid writes [lev][dny][dnx].  src == dst is
 *   allowed.  The destination's periodic flag is irrelevant for bilinear and nearest: its points are just points.  A destination that is
 *   a row block of a larger grid is an ordinary grid: that is how a row-sharded host uses these calls.
 * mpg_regrid_store_grid_to_grid, MPG_REGRIDMETHOD_BILINEAR, source without MPG_GRID_PERIODIC_I: per destination point the rule of
 *   mpg_regrid_store_to_mesh -- the same quads, the lowest passing quad id, the grid_inside_tol_exp tolerance, slots A, B, C, D -- run by
 *   that call's kernels on the destination stagger's points.  A fixed 4-slot handle; an unmapped point has idx -1.  Both candidate routes
 *   give identical bytes: the index route through the SOURCE grid's inverse projection, and the pyramid walk;
 *   mpg_tune("store_boxes", 0), mpg_handle_store_path and mpg_handle_store_stats [1] [2] behave as in that call.
 * MPG_REGRIDMETHOD_BILINEAR, source with MPG_GRID_PERIODIC_I: src_staggerloc must be MPG_STAGGERLOC_CENTER (any other source stagger ->
 *   MPG_ERR_UNSUPPORTED).  The rule of mpg_regrid_store_periodic_to_mesh: seam quads, pole caps under pole_method, the end-row hemisphere
 *   rule and the MPG_GRID_NO_*_POLE flags.  An ordinary CSR handle without pole terms: quad rows have 4 entries, cap rows nx.
 *   mpg_handle_store_stats are that call's.
 * pole_method must be MPG_POLEMETHOD_NONE or MPG_POLEMETHOD_ALLAVG on every call; for a non-periodic source (and for nearest) it is
 *   ignored, and it is 0 in the cache key.
 * MPG_REGRIDMETHOD_NEAREST_STOD: the rule of the Grid -> Mesh nearest Store, periodic sources included: the smallest chord distance,
 *   the lowest source index on ties.  A fixed 1-slot handle; every point is mapped.
 * MPG_REGRIDMETHOD_CONSERVE -> MPG_ERR_UNSUPPORTED; the message names mpg_regrid_store_conserve_grid_to_grid.
 * mpg_regrid_store_conserve_grid_to_grid: ESMF_FieldRegridStore(regridmethod=CONSERVE, normType=) between the CELLS of two grids.  Cell
 *   (i, j) is the quadrilateral of CORNER points (i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1), index j * nx + i; a grid without CORNER
 *   coordinates -> MPG_ERR_INVALID_ARG.  I(d, s) is the Mesh -> Mesh statement above (mpg_regrid_store_conserve_mesh) word for word, with
 *   "cell polygon" read as this quadrilateral: the source cell is the subject polygon, made counter-clockwise by the sign of its own fan
 *   area; it is clipped by the destination cell's sides in listed order, that cell made counter-clockwise the same way; clip-plane
 *   normals in difference form a x (b - a); the in-place clip of the other conservative Stores with its 1e-15 * |n| inside rule; a side
 *   with |b - a|^2 < 1e-24 bounds nothing; the area is the triangle fan from slot 0, clamped at 0; area(d) is the cell's own fan area; no
 *   floating-point contraction.  Rows are keyed by destination cell, columns ascending.  MPG_NORM_DSTAREA: w = I / area(d);
 *   MPG_NORM_FRACAREA: w = I / sum_s I.  An entry is dropped when I <= 1e-14 * area(d); an uncovered cell has an empty row.  The dst
 *   fraction, summed in ascending source index, stays with the handle (mpg_handle_get_dst_frac).  Two Stores on fresh objects give the
 *   same bytes: no atomic decides a stored byte.  Periodic grids are accepted on either side: the collapsed pole sides bound nothing, and
 *   a cell without area is part of no pair.
 *   Candidates: one thread per destination cell walks the source grid's cell pyramid with the cell's own padded box (the coordinate
 *   hull of its corners, padded by 2 e2 + 1e-9: DESIGN.md s4.2), so no pair with I > 0 is removed; the pair list has exact size.  The
 *   pyramid walk is the only candidate route of this Store: mpg_handle_store_path reports 0.  mpg_handle_store_stats: [1] pairs clipped,
 *   [6] vertex slots of the clip.
 * Refusals, each with a message that names the call and the way out.  MPG_ERR_INVALID_ARG: NULL arguments; unknown enums; a stagger
 *   without coordinates; fewer than 2 x 2 source points for bilinear; the periodic call's own argument errors (nx < 3 or ny < 2; two live
 *   end rows in one hemisphere).  MPG_ERR_UNSUPPORTED: as stated above.  MPG_ERR_OVERFLOW: counts beyond int32; nnz >= 2^31; a clipped
 *   polygon that outgrew its vertex slots.
 * Cached like every Store and paired with one mpg_handle_release.  The keys carry kind bits of their own, both grids, both staggers and
 *   the method, inside_tol_exp for bilinear, pole_method for a periodic source's bilinear Store and norm_type for the conservative Store:
 *   they collide with no other Store's key -- mpg_regrid_store_grid's included --, and staggers, methods, norms, pole methods and the two
 *   directions are distinct handles.  Parked entries go when EITHER grid is destroyed.  There are no _begin variants.
 * The wind chain does not mistake these handles: mpg_wind_destagger[_pitched]_dev and mpg_wind_destagger_transpose_dev recognise the
 *   destagger pair by shape, so a handle of these Stores whose source grid is not its destination grid is marked, and those calls return
 *   MPG_ERR_UNSUPPORTED for it.  With src == dst the CENTER -> EDGE1 / EDGE2 handles of this call are served like mpg_regrid_store_grid's.
 * Everything that takes a fixed 1- or 4-slot handle or a CSR handle takes these unchanged: mpg_regrid_dev / _typed[_pitched]_dev, the
 *   bundle calls, mpg_regrid_masked_dev, mpg_regrid_transpose_dev, the weight getters, mpg_handle_extrapolate[_masked], mpg_handle_mask,
 *   mpg_handle_creep, mpg_handle_patch (non-periodic bilinear), mpg_handle_conserve2nd (the conservative handle, non-periodic source) and
 *   mpg_handle_compose. */
int mpg_regrid_store_grid_to_grid(mpg_grid src, int src_staggerloc, mpg_grid dst, int dst_staggerloc, int regridmethod, int pole_method,
                                  mpg_handle *out);
int mpg_regrid_store_conserve_grid_to_grid(mpg_grid src, mpg_grid dst, int norm_type, mpg_handle *out);

/* ---- nearest destination to source: ESMF_FieldRegridStore(regridmethod=ESMF_REGRIDMETHOD_NEAREST_DTOS) --------------------------------------
 * The one method that scatters: every source point goes to the ONE destination point nearest to it, and a destination point receives the
 * sum of all sources that chose it.  No source is lost; a destination may receive nothing.  Counts (flashes, point emissions, "how many
 * fine cells fall in this box"), a cell-to-box membership table, with MPG_DTOS_MEAN a cheap box average onto a verification grid -- and
 * the only aggregating route for fields on vertices and edges, since the conservative Stores know cells only.
 *
 * Point sets (mpg_points): exactly one of mesh / grid is non-NULL, as for mpg_handle_extrapolate.  Sources are the QUERIES: any stagger of
 *   a grid that holds its coordinates, or a mesh's cells, vertices or edges (edges after mpg_mesh_set_edges).  Destinations are the
 *   SEARCHED set: any stagger of a grid (through that stagger's point pyramid) or a mesh's cells (MPG_MESHLOC_ELEMENT, through the site BVH
 *   built whole).  Ids are the handle's usual indices: the cell, vertex or edge id, or j * snx + i.
 * Rule.  For a source s that is not masked the candidates are the destination points that are not masked.  nearest(s) is the candidate
 *   with the smallest (d2, id) in lexicographic order; d2 is dist2_nofma of the stored unit vectors, ((dx*dx + dy*dy) + dz*dz) in float64
 *   without contraction (mpg_mesh_get_xyz / mpg_grid_get_xyz export their bits).  A tie goes to the lower destination id.  A masked
 *   source, or a call in which every destination is masked, gives nearest(s) = -1.  A mask is bytes on the device, [n_src] / [n_dst];
 *   non-zero = masked, NULL = no mask.
 * Handle: an ordinary CSR handle of method MPG_REGRIDMETHOD_NEAREST_DTOS with n_src of the source set and n_dst, nx_dst, ny_dst of the
 *   destination set.  Row d holds the sources with nearest(s) == d in ascending source id, which is the Regrid's summation order.
 *   MPG_DTOS_SUM (ESMF's rule): every value is 1.0.  MPG_DTOS_MEAN: every value of row d is 1.0 / (double)len(d), rounded once.  A
 *   destination that no source chose has an empty row: every Regrid writes +0.0 there and mpg_regrid_masked_dev the fill value.  The val
 *   array is always present; the handle carries no dst_frac; the longest row is recorded.  mpg_handle_store_stats: [1] sources mapped,
 *   [2] non-empty rows, [3] the longest row.  mpg_handle_store_ms is the GPU time of the call.
 *   mpg_handle_get_src_nearest downloads nearest[] -- the binning index itself, which the handle keeps at 4 bytes per source; for a
 *   handle of any other origin it returns MPG_ERR_INVALID_ARG.
 * Determinism and ownership: no atomic decides a stored byte (integer atomics count, none places); two Stores on fresh objects give the
 *   same bytes.  The handle is not cached: pair it with mpg_handle_release.  The call blocks and drains the Store worker first, as
 *   mpg_handle_extrapolate does.
 * Refusals, each with a message that names mpg_regrid_store_nearest_dtos and the way out.  MPG_ERR_INVALID_ARG: a NULL argument (src, dst
 *   and out are mandatory); both or neither of mesh / grid set in a point set; an unknown mesh location, stagger or norm; a stagger
 *   without coordinates; an edge source on a mesh without edges.  MPG_ERR_UNSUPPORTED: a destination at MPG_MESHLOC_NODE or
 *   MPG_MESHLOC_EDGE (no tree is built over them); a mesh of mpg_mesh_create_window on either side; a destination mesh that carries a
 *   source window.  MPG_ERR_OVERFLOW: counts beyond int32.  Empty input is success: a source set without points, or a source mask that
 *   masks everything, gives an all-empty pattern.
 * Consumers: every CSR consumer takes the handle unchanged -- mpg_regrid_typed[_pitched]_dev, mpg_regrid_csr_to_mesh_dev,
 *   mpg_regrid_csr_rows_dev, mpg_regrid_masked_dev, mpg_regrid_transpose_dev, mpg_handle_compose, mpg_handle_get_csr.  The transpose of a
 *   MPG_DTOS_SUM handle hands each source the value of its destination: the nearest gather in the other direction.  mpg_handle_mask with
 *   MPG_MASKRULE_AUTO refuses the handle with MPG_ERR_UNSUPPORTED -- a destination masked afterwards would not re-route its sources: pass
 *   the masks to this Store -- while the explicit rules work as for any CSR handle. */
enum { MPG_REGRIDMETHOD_NEAREST_DTOS = 5 };
enum { MPG_DTOS_SUM = 0, MPG_DTOS_MEAN = 1 };
int mpg_regrid_store_nearest_dtos(const mpg_points *src, const mpg_points *dst, int norm,
                                  const uint8_t *src_mask_dev, const uint8_t *dst_mask_dev, mpg_handle *out);
int mpg_handle_get_src_nearest(mpg_handle rh, int32_t *nearest_host /* [n_src] */);

/* ---- output epilogues: what write_data.F90 computes on rank 0 between ESMF_FieldGather and nf90_put_var, done on
 * the device-resident regridded fields so that only final float32 arrays leave the GPU.
 * Every output variable is NF90_FLOAT (write_data.F90:312-980) while the fields are float64: the cast below is the
 * conversion nf90_put_var applies (round to nearest).  Device pointers; hip_stream as in mpg_regrid_dev.  dst_be != 0
 * stores the float32 results big-endian (the variable's bytes in a NetCDF classic file), as MPG_TYPE_BE does for Regrid.
 *   mpg_post_cast_dev        dst = (float)fma(src, scale, offset), one float64 rounding and the conversion: plain fields (scale 1,
 *                            offset 0), T - 300 (:1339-1347, the `continue` in that loop is a no-op statement, so every point is
 *                            shifted), PHB*9.81 (:1418).  The writer uses scale or offset, never both: fma(src, 1, offset) is
 *                            src + offset and fma(src, scale, 0) is src * scale rounded once, the reference's single operation;
 *                            with both set the product is NOT rounded before the sum
 *   mpg_post_layer_mean_dev  Z_C(k) = 0.5*(PHB(k+1) + PHB(k)), src [nlevp1][n_pts] -> dst [nlevp1-1][n_pts] (:1406-1415)
 *   mpg_post_ptop_dev        P_TOP from P_HYD [nlev][n_pts]: min(maxval(P_HYD), 0.8*P_HYD(top) over columns whose top
 *                            value is >= 10) (:1362-1371); float64 result returned to the host, blocks on the stream */
/* ---- device buffers for hosts without a HIP binding of their own ---------------------------------------------------
 * ESMF owned the field storage (ESMF_FieldCreate, farrayPtr: input_data.F90:638, interp.F90:702).  A host that keeps its
 * fields in HBM between the input and the output file (fortran/mpassit_driver.F90 on NetCDF files) allocates them
 * here and passes the pointers to the _dev entry points.  upload / download are plain blocking copies. */
int mpg_dev_alloc(int64_t nbytes, void **out_dev);
int mpg_dev_free(void *dev);
int mpg_dev_upload(void *dst_dev, const void *src_host, int64_t nbytes);
int mpg_dev_download(void *dst_host, const void *src_dev, int64_t nbytes);

/* In-place byte swap of n elements of elem_size 2, 4 or 8 bytes on the device, for big-endian file data that does NOT
 * pass through mpg_regrid_typed_dev / mpg_post_*_dev (those take and produce it directly, MPG_TYPE_BE). */
int mpg_bswap_dev(void *buf_dev, int64_t n, int elem_size, void *hip_stream);
/* The transport of such a variable: bytes [offset, offset + nbytes) of a file -> device memory and back, untouched,
 * through pinned staging buffers and a few pread / pwrite threads (the page-cache side of the copy is what limits a
 * single core: eight readers -- MPG_IO_READ_THREADS=1..8 in the environment overrides --, four writers).  Replaces the nf90_get_var / nf90_put_var data movement of input_data.F90:630 and
 * write_data.F90:1008-1475 for NetCDF classic files; offset / nbytes come from ncio_var_extent.  Blocking: hip_stream is
 * synchronised first (earlier users / the producer of the device buffer), the range is complete on return.  The file
 * must already have the size (ncio_var_extent extends a file being written).  One read and one write may run
 * concurrently from two host threads. */
int mpg_file_to_dev(const char *path, int64_t offset, int64_t nbytes, void *dst_dev, void *hip_stream);
int mpg_dev_to_file(const char *path, int64_t offset, int64_t nbytes, const void *src_dev, void *hip_stream);
/* ... from pitched planes: nplanes planes of plane_bytes, src_pitch_bytes apart in device memory (>= plane_bytes; the results of
 * the _pitched_dev calls), -> the contiguous range [offset, offset + nplanes * plane_bytes) of the file.  The range is cut into
 * chunks and written by the same threads as mpg_dev_to_file; each chunk is gathered from the planes it covers. */
int mpg_dev_to_file_planes(const char *path, int64_t offset, int64_t plane_bytes, int64_t nplanes, const void *src_dev,
                           int64_t src_pitch_bytes, void *hip_stream);
int mpg_post_cast_dev(const double *src_dev, int64_t n, double scale, double offset, float *dst_dev, int dst_be, void *hip_stream);
int mpg_post_layer_mean_dev(const double *src_dev, int nlevp1, int64_t n_pts, float *dst_dev, int dst_be, void *hip_stream);
int mpg_post_ptop_dev(const double *p_hyd_dev, int nlev, int64_t n_pts, double *ptop_host, void *hip_stream);
/* The two reductions P_TOP is made of, for a host that holds only a block of the grid rows (one driver image per GPU):
 * vmax = maxval(P_HYD) of the block, candmin = min of 0.8*P_HYD(top) over its columns with P_HYD(top) >= 10 (has_cand = 0
 * when there is none).  P_TOP = min(max of the vmax, min of the candmin) over the blocks -- exact, independent of the split. */
int mpg_post_ptop_parts_dev(const double *p_hyd_dev, int nlev, int64_t n_pts, double *vmax_host, double *candmin_host, int *has_cand_host,
                            void *hip_stream);

/* ---- bring-your-own weights: the factorList / factorIndexList form of ESMF_FieldRegridStore (and of an
 * ESMF_RegridWeightGen file: S, col, row).  Builds a route handle that applies externally computed weights with the
 * same Regrid kernels, e.g. to compare this library's weight generation with ESMF's on a site that has ESMF.
 * col = source index, row = destination index (j*nx_dst + i), both 1-based as in ESMF; any entry order (order
 * inside a destination row is kept = summation order).  Destination points without entries regrid to 0.0. */
int mpg_handle_from_weights(int64_t n_src, int nx_dst, int ny_dst, int64_t nnz, const int32_t *row_host,
                            const int32_t *col_host, const double *S_host, mpg_handle *out);

/* ---- introspection (tests, INTEGRATION.md, multi-GPU halo schedule) -------------------------------- */
/* n_src: source points the handle indexes; n_dst = nx_dst*ny_dst; nnz_per_row: 3 bilinear(mesh),
 * 4 bilinear(grid), 1 nearest, 0 = CSR (conservative); nnz = total stored weights. */
int mpg_handle_info(mpg_handle rh, int64_t *n_src, int64_t *n_dst, int *nx_dst, int *ny_dst,
                    int *nnz_per_row, int64_t *nnz);
/* fixed-nnz handles: idx/w are [n_dst][nnz_per_row] (row-major, host); idx = -1 where unmapped */
int mpg_handle_get_weights(mpg_handle rh, int32_t *idx_host, double *w_host);
/* CSR handles: rowptr [n_dst+1], col/val [nnz] (host) */
int mpg_handle_get_csr(mpg_handle rh, int64_t *rowptr_host, int32_t *col_host, double *val_host);
/* Which Regrid kernel serves a 3-point (bilinear) handle, decided when its tile lists are built on the first Regrid:
 * cell_fast_kernel / lev_fast_kernel: 0 = not decided yet (no bundle of >= 8 levels in that layout so far), -1 = lane- /
 * row-gather kernel, > 0 = LDS-staged ("a3_staged" value + 1 / 1);  max_unique = largest number of distinct source cells one
 * tile of the lists in use references (0 without lists). */
int mpg_handle_kernel_choice(mpg_handle rh, int *cell_fast_kernel, int *lev_fast_kernel, int *max_unique);
/* Locality of the source cells as the staged Regrid kernels see them, from the tile lists in use (error before the first
 * staged Regrid of the handle): the tile shape in target points; reuse = 3 * n_dst / (sum over the tiles of their
 * distinct source cells) -- how often a staged value is used; line_fill = the fraction of every 128-byte line of a
 * cell-fast float64 field touched by a tile that the tile actually uses (1 = its cells are dense runs of consecutive
 * ids, as on a row-numbered regional mesh; towards 1/16 = scattered ids: the mesh's cell numbering has no locality and
 * the level-fast (file-order) layout, which gathers whole rows, is the better route).  Diagnostics only; the reference
 * has no counterpart (ESMF hides its route handle). */
int mpg_handle_tile_stats(mpg_handle rh, int *tile_nx, int *tile_ny, double *reuse, double *line_fill);
/* Pole terms of a Grid -> Grid handle on a periodic (monopole) grid.  Destination points inside a pole cap
 * (triangle pole / A / B of the first or last CENTER row) carry, besides the A and B entries reported by
 * mpg_handle_get_weights, a weight on the pole node; the pole's value is the mean of the `row_len` sources
 * starting at `src_row_start`, i.e. ESMF's factor list holds row_len entries of w_pole/row_len for it.
 * mpg_handle_pole_count: n_points = 0 for every other handle.  mpg_handle_get_pole: arrays [n_points] (host);
 * entries with w_pole == 0 are destination points of the two candidate rows that are not in a cap. */
int mpg_handle_pole_count(mpg_handle rh, int64_t *n_points, int *row_len);
int mpg_handle_get_pole(mpg_handle rh, int32_t *dst_id_host, int32_t *src_row_start_host, double *w_pole_host);
/* dual (Delaunay) triangles of a mesh: tri_host [nVertices][3], 0-based cell ids or -1 */
int mpg_mesh_get_triangles(mpg_mesh mesh, int32_t *tri_host);
/* the stored unit vectors of a point set, xyz_host [3][n] (x, y, z planes): the bits every search of this library uses (its sin and cos
 * are not the host's).  mesh: n of MPG_MESHLOC_ELEMENT / NODE / EDGE; grid: n = snx * sny of the stagger, j * snx + i */
int mpg_mesh_get_xyz(mpg_mesh mesh, int meshloc, double *xyz_host);     /* [3][n]: the stored unit vectors */
int mpg_grid_get_xyz(mpg_grid grid, int staggerloc, double *xyz_host);  /* [3][snx*sny] */

/* Multi-GPU (ESMF's per-Regrid source exchange): sorted unique source ids the handle
 * references.  Call with ids_host == NULL to get the count.  mpg_handle_localize rewrites the handle's
 * indices to positions in that list so that Regrid reads a compact [nlev][n_unique] halo buffer. */
int mpg_handle_unique_sources(mpg_handle rh, int64_t *n_unique, int32_t *ids_host);
/* Source window of a mesh: a host that holds, for every source field, only the contiguous id range [first, first + count)
 * its target rows reference -- one driver image per GPU reading just that range of every variable (MPAS variables are
 * [nCells][nLevels]: a cell range is one byte range of the file), where the reference has every rank read everything
 * (input_data.F90:645) and ESMF redistributes.  mpg_handle_source_range reports the global ids [first, end) a Mesh -> Grid
 * handle references (first == end: none).  mpg_mesh_set_source_window then declares the window for one mesh location:
 * every handle of that mesh and location -- existing (in use or parked in the cache) and future -- indexes its sources
 * relative to `first`, and Regrid reads source slabs of `count` ids ([nlev][count] / [count][nlev]); mpg_handle_info
 * reports n_src = count.  A handle that references a source outside the window fails the call.  Grid -> Mesh handles
 * (mpg_regrid_store_to_mesh) are not touched: the mesh is their destination.  Unlike the two calls
 * below the handles stay in the Store cache.  The whole mesh (first 0, count nCells / nVertices) resets it. */
int mpg_handle_source_range(mpg_handle rh, int64_t *first, int64_t *end);
int mpg_mesh_set_source_window(mpg_mesh mesh, int meshloc, int64_t first, int64_t count);
/* Both re-index the handle IN PLACE and detach it from the Store cache; a handle that is shared (mpg_regrid_store returned
 * the same pointer twice: refcount 2) is refused with MPG_ERR_INVALID_ARG -- release the other reference first. */
int mpg_handle_localize(mpg_handle rh);
/* Halo in "range" form (spatially banded cell numbering): subtract `base` from every source index and
 * declare the local source extent n_local, so that Regrid reads a [nlev][n_local] buffer holding the
 * global cell range [base, base + n_local).  Fails if any referenced id falls outside that range. */
int mpg_handle_rebase(mpg_handle rh, int64_t base, int64_t n_local);
/* dst[k][i] = src[k][ids[i]] (pack owned cells for the halo exchange); all device pointers */
int mpg_pack_dev(const double *src_dev, int64_t n_src, int nlev, const int32_t *ids_dev, int64_t n_ids,
                 double *dst_dev, void *hip_stream);

/* ---- several GPUs: one process per GPU, RCCL underneath (ESMF's source exchange and ESMF_FieldGather) -------------------
 * Target rows are sharded over the ranks (regDecomp = (/1, npets/), model_grid.F90:693) and source cells owned in contiguous
 * id blocks (model_grid.F90:423-438, 2428-2441); a rank whose rows reference cells of another rank's block receives them in
 * ONE grouped ncclSend / ncclRecv exchange per field batch -- what ESMF does inside every ESMF_FieldRegrid (interp.F90:134...).
 * No torch, no MPI: the ranks meet through `id_file` (rank 0 writes the RCCL unique id there; a path all ranks see, fresh per
 * run), the library loads librccl on first use.  A host that READS its sources from files needs none of this: it reads the
 * window its rows reference (mpg_mesh_set_source_window above); these verbs serve hosts whose source fields are produced or
 * held partitioned on the devices (bench.py --gpus N, a coupled model).
 *   mpg_comm_init / _destroy / _info      communicator of this process (its GPU = the one of mpg_init)
 *   mpg_comm_allgather                    small host-side metadata, rank order (blocking)
 *   mpg_halo_build                        the schedule for one Mesh -> Grid handle whose grid is this rank's row block:
 *                                         asks the handle for its source ids, agrees on the ownership blocks with the other
 *                                         ranks (ownership 0: block boundaries in the middle of the overlap of neighbouring
 *                                         ranks' needs -- only the strip along a row-block boundary travels; 1: equal blocks
 *                                         like the reference's para_range) and RE-INDEXES THE HANDLE IN PLACE to the local
 *                                         source space of n_local ids (range form: the covering id range, own block in place
 *                                         at own_pos; compact form for arbitrary numbering: the sorted needed ids) -- the
 *                                         handle leaves the Store cache, as with mpg_handle_rebase / _localize
 *   mpg_halo_exchange_dev                 one exchange of nrows rows (nfields * nlev): pack, grouped send / recv, unpack,
 *                                         enqueued on the stream; buffers allocated at the first call of a batch size
 *   mpg_gather_rows                       ESMF_FieldGather (write_data.F90:1006-1453): row blocks -> the whole field on root
 *   mpg_halo_plan_host                    the schedule as a pure function of every rank's needed ids (tests, diagnostics) */
/* The id file and its deadlines: rank 0 removes whatever is at `id_file`, writes {magic, launch tag = hash of the
 * environment's MPASSIT_RUN_ID (0 without), wall-clock time, nranks, id} and removes the file again once ncclCommInitRank
 * has returned; the other ranks ignore a file with another tag / nranks or written more than MPG_COMM_STALE_S (300) seconds
 * before they loaded the library.  Several ranks WITHOUT MPASSIT_RUN_ID are refused (MPG_ERR_INVALID_ARG: an untagged launch cannot
 * tell its file from one a crashed launch left behind); MPG_COMM_ALLOW_UNTAGGED=1 overrides, a reader then takes only a file at most
 * 30 s older than itself whose bytes are unchanged one second later.  Waiting for the file, ncclCommInitRank (run on a helper thread) and the blocking
 * all-gathers give up after MPG_COMM_TIMEOUT_S (120) seconds with MPG_ERR_TIMEOUT: a dead or missing peer is an error exit,
 * never a hang.  mpg_comm_idfile_verdict is that acceptance rule as a pure function (NULL = accepted; CPU tests). */
typedef struct mpg_comm_s *mpg_comm;
typedef struct mpg_halo_s *mpg_halo;
int mpg_comm_init(int rank, int nranks, const char *id_file, mpg_comm *out);
const char *mpg_comm_idfile_verdict(const void *bytes, int64_t nbytes, int nranks, uint64_t tag, int64_t reader_loaded_ns, double stale_s);
int mpg_comm_destroy(mpg_comm comm);
int mpg_comm_info(mpg_comm comm, int *rank, int *nranks);
int mpg_comm_allgather(mpg_comm comm, const void *send_host, int64_t nbytes, void *recv_host);
int mpg_halo_build(mpg_comm comm, mpg_handle rh, int64_t n_cells_global, int ownership, mpg_halo *out);
/* The same for a partition of the source cells that is the CALLER's (owned form): owned_ids_host = this rank's sorted unique global
 * ids, any shape -- the model's own decomposition of a coupled run (MPAS partitions its cells with a graph partitioner, not in id
 * blocks), or one that follows the target rows of a mesh without banded numbering: bench.py gives every cell to the lowest rank whose
 * rows reference it, so that only the overlap of neighbouring row blocks travels (equal id blocks of a Morton-numbered global mesh
 * would move 7/8 of all referenced values at 8 ranks).  The ranks' lists must be disjoint and cover every cell some rank references
 * (else MPG_ERR_INVALID_ARG).  The handle is re-indexed to the rank's sorted needed ids (n_local of them, as in the compact form);
 * mpg_halo_info reports mode 2 and own = {0, n_owned}; own_dev of mpg_halo_exchange_dev is [nrows][own_ld >= n_owned] in the order
 * of owned_ids_host.  What a peer sends arrives in id order and is scattered to its positions among the needed ids. */
int mpg_halo_build_owned(mpg_comm comm, mpg_handle rh, int64_t n_cells_global, const int32_t *owned_ids_host, int64_t n_owned, mpg_halo *out);
/* mode 0 range / 1 compact / 2 owned; own = the global id block [own[0], own[1]) this rank holds; base = global id of local index 0
 * (range form); own_pos = where the own block sits in the local space (range form); sent / received per row = elements that
 * cross the links per exchanged row.  Any pointer may be NULL. */
int mpg_halo_info(mpg_halo halo, int *mode, int64_t *n_local, int64_t *own, int64_t *base, int64_t *own_pos, int64_t *sent_per_row,
                  int64_t *received_per_row);
/* own_dev: nrows rows of the own block, row stride own_ld elements; local_dev: [nrows][n_local], filled in place.
 * elem_bytes: 4 or 8 for sources held cell-fast ([level][cell], input_data.F90:653-655: nrows = nfields * nlev), or the bytes of
 * one whole source row for sources held in MPAS file order ([cell][level], input_data.F90:630,645: nrows = nfields, elem_bytes =
 * nlev * 4 for float32, nlev * 8 for float64; any multiple of 4) -- in range form a neighbour's strip of a file-order slab is
 * ONE contiguous byte range per field, no pack step at all.
 * Range form: own_dev may be the in-place view (local_dev + own_pos[0] elements, own_ld = n_local) -- the own
 * data is then where Regrid reads it and only the neighbours' strips move -- or a separate buffer, which is copied to
 * its place first; any other overlap with local_dev is refused.  Compact form: own_dev is always a separate buffer. */
int mpg_halo_exchange_dev(mpg_halo halo, const void *own_dev, int64_t own_ld, void *local_dev, int nrows, int elem_bytes, void *hip_stream);
int mpg_halo_destroy(mpg_halo halo);
/* dst[k][i] = src[k * ld + ids[i]], nrows rows of elements of elem_bytes bytes (as above): the pack step of the compact halo
 * form on its own, for a host that runs the exchange through its own transport (mpassit_amd/dist.py on torch.distributed). */
int mpg_pack_rows_dev(const void *src_dev, int64_t ld, int nrows, int elem_bytes, const int32_t *ids_dev, int64_t n_ids, void *dst_dev, void *hip_stream);
/* REHEARSAL ON ONE GPU (tests and tools; never a production path).  RCCL refuses two ranks on one card, but it accepts
 * ncclSend / ncclRecv with peer == self inside one group.  mpg_comm_virtual makes virtual rank v_rank of v_nranks on top of
 * `real`, the ONE-rank communicator of the process; every virtual rank is driven by its own host thread and makes the calls a
 * real rank makes (mpg_comm_allgather, mpg_halo_build, mpg_halo_exchange_dev, mpg_gather_rows).  Each collective step is a
 * rendezvous of those threads; the last to arrive issues, for all of them, the very RCCL calls the real ranks would issue --
 * same entry points, same device pointers and byte counts from each rank's own schedule, ordered against each rank's stream
 * by events -- with every peer mapped to rank 0 of the real communicator.  Two ranks whose schedules disagree (a send that meets a receive
 * of another size) fail the step.  What it cannot show is bytes crossing xGMI.  A thread that never arrives ends the others'
 * wait with MPG_ERR_TIMEOUT after MPG_COMM_TIMEOUT_S.  mpg_comm_virtual_stats: groups, sends, receives and all-gathers the
 * group has really put through RCCL (any pointer may be NULL).  Destroy the virtual ranks before `real`. */
int mpg_comm_virtual(mpg_comm real, int v_rank, int v_nranks, mpg_comm *out);
int mpg_comm_virtual_stats(mpg_comm comm, int64_t *groups, int64_t *sends, int64_t *recvs, int64_t *allgathers);
/* rows_dev: this rank's [nlev][j1 - j0][nx] block of an [nlev][ny][nx] field; dst_dev (root only): the whole field */
int mpg_gather_rows(mpg_comm comm, const void *rows_dev, int64_t j0, int64_t j1, int64_t nx, int64_t ny, int nlev, int elem_bytes,
                    void *dst_dev, int root, void *hip_stream);
/* needed[q]: rank q's sorted unique needed ids (n_needed[q] of them).  Outputs for `rank` (arrays of nranks entries unless
 * noted): send_count; send_a = start of the range inside the own block (range form, -1 in compact form); recv_a / recv_b =
 * destination range in the local space; compact form: send_ids_flat (capacity send_ids_cap) + send_ids_off [nranks + 1]. */
int mpg_halo_plan_host(int rank, int nranks, int64_t n_cells, int ownership, const int64_t *n_needed, const int32_t *const *needed, int *mode,
                       int64_t *n_local, int64_t *own, int64_t *base, int64_t *own_pos, int64_t *send_count, int64_t *send_a, int64_t *recv_a,
                       int64_t *recv_b, int32_t *send_ids_flat, int64_t send_ids_cap, int64_t *send_ids_off);
/* the owned form's schedule as a pure function: per peer q (self included) send_flat[send_off[q] .. send_off[q + 1]) = offsets into
 * `rank`'s owned list in the order sent, recv_flat[recv_off[q] ..) = destination positions in its local space in the order received */
int mpg_halo_plan_owned_host(int rank, int nranks, const int64_t *n_needed, const int32_t *const *needed, const int64_t *n_owned,
                             const int32_t *const *owned, int64_t *n_local, int32_t *send_flat, int64_t send_cap, int64_t *send_off, int32_t *recv_flat,
                             int64_t recv_cap, int64_t *recv_off);

/* kernel-selection knobs for benchmarking and the A/B tests (defaults are the tuned production values; DESIGN.md s4.1 has
 * the measurements behind every default).  They select among kernels that produce identical bits:
 *   "a3_staged"   cell-fast 3-point Regrid: -1 per-handle choice (default), -2 lane-gather kernel, 0 / 1 / 2 the LDS-staged
 *                 kernel on 64x8-point tiles / 64x16 on 256 threads / 64x16 on 512 threads
 *   "lf_variant"  level-fast (file-order) 3-point Regrid: -1 per-handle choice (default), 0 row gather on linear aligned
 *                 tiles, 1 LDS-staged in 16-level chunks, 2 row gather on grid-row tiles (the capacity fallback)
 *   "nn_variant"  nearest-neighbour search: 1 wave-cooperative (default), 0 one thread per point
 *   "field_band"  order of the (field, tile) work items of a bundle Regrid: -1 each kernel's own choice (default: bands of
 *                 1024 tiles for the level-fast row gather, field-major for the staged kernels), 0 field-major, n > 0 all
 *                 fields of a band of n tiles before the next band
 *   "store_boxes" Stores on a grid that knows its projection: 1 (default) candidates through the grid's index space, 0 the
 *                 hierarchical search always
 *   "compose_block_rows"  mpg_handle_compose: 0 (default) blocks of destination rows by the byte budget alone, n > 0 of at most n rows
 *                 as well (tests force many blocks at toy size; the composite is the same)
 * and one that does NOT (it selects between two readings of ESMF's undocumented-here behaviour):
 *   "bilinear_linetype"   Mesh -> Grid bilinear Store: 0 (default) the target point meets the plane of its source triangle
 *                 along the ray from the sphere's centre; 1 along the plane's normal (ESMF_LINETYPE_CART read literally).
 *                 In force at mpg_regrid_store time; the two differ by O(h^2) of the triangle size
 *   "lfu_min_reuse_x10"   threshold (x10) of the per-handle level-fast choice (default 35)
 *   "lfu_npf"     row slots per thread of the staged level-fast kernel: 0 (default) = by the handle's longest tile list (2 / 4 / 8 / 16),
 *                 16 = the fixed shape of rounds 1-4 (A/B measurements; the results are the same bits)
 *   "lf_rows_store", "staged_store"   how results are STORED (never what: the same bits).  A result is [nlev][ny][nx]; level k's plane starts on a
 *                 128-byte line only when ny * nx is a multiple of 32 (float32) / 16 (float64) points, and the kernels' runs of 64 points of a plane
 *                 that does not have a partial line at either end.  Default 0: whole lines non-temporal, partial lines write-back (per lane;
 *                 the row gather's float32 results per level).  "lf_rows_store" 1 / 2 / 3: the file-order row gather plain / non-temporal / per lane;
 *                 "staged_store" 2: the staged cell-fast kernel non-temporal on every lane (what rounds 2-6a shipped).  A/B only
 *                 (profiles/r06_plane_alignment.md: 14-29 % on grids with an odd number of points per level)
 * Unknown keys and out-of-range values return MPG_ERR_INVALID_ARG. */
int mpg_tune(const char *key, int value);

/* timing of the last Store phases in ms (search build, search, finalize); any pointer may be NULL */
int mpg_handle_store_ms(mpg_handle rh, float *ms_total);
/* How the Store found its candidates: 0 = the hierarchical search (pyramid walk over the grid / BVH over the mesh);
 * 1 = through the grid's index space (a grid that knows its projection, mpg_grid_create_proj / mpg_grid_attach_proj, fine
 * enough for the claim to hold -- DESIGN.md s4.2); 2 = nearest only: index space for the points it can vouch for, the BVH for
 * the others.  The weights are the same bits either way; diagnostics only. */
int mpg_handle_store_path(mpg_handle rh, int *candidates);
/* Which data-dependent branches the Store of a Mesh -> Grid handle took: n values (up to 8; the rest 0) into stats_host.  [0] = the
 * store path above.  Then by method --
 *   bilinear:     [1] triangles handed to the wave-per-triangle rasteriser (no usable index near a pole / the projection's cut, or
 *                 more than 16 leaves of the pyramid), [2] triangles in all
 *   nearest:      [1] bin side in grid points (2 where the mesh is as fine as the grid .. 16), [2] bins, [3] points the bins could not
 *                 vouch for (settled by the tree), [4] cells on and around the grid the bin side was sized from
 *   conservative: [1] (cell, destination cell) pairs clipped, [2] polygons with more candidates than their 24-entry list (spilled
 *                 past it into their overflow slot, or counted and listed by a workgroup), [3] polygons whose index box a wavefront
 *                 enumerated (more than 128 box cells), [4] polygons the cooperative count pass walked the pyramid for, [5] lists
 *                 the list pass copied from the spill area instead of walking again, [6] vertex slots per polygon of the clip
 * Diagnostics (the tests use them to assert that a case built to force a branch did take it); the weights do not depend on them. */
int mpg_handle_store_stats(mpg_handle rh, int64_t *stats_host, int n);

/* Test hook: the library's own device-wide primitives (csrc/k_prims.hip; they took rocPRIM's place in round 5) on host arrays --
 * out_host[i] = in_host[0] + ... + in_host[i - 1] (int32, exclusive; out_host may be NULL) and *sum_host = the 64-bit sum (may be NULL).
 * The Stores use them on device counts; this entry exists so that a test can ask them directly at awkward sizes. */
int mpg_debug_scan_i32(const int32_t *in_host, int64_t n, int32_t *out_host, long long *sum_host);

#ifdef __cplusplus
}
#endif
#endif
