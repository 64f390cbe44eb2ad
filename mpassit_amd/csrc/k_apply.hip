// Weight application ("Regrid"): the knobs of its dispatcher, and the wind rotation.
//
// Replace ESMF_Field[Bundle]Regrid at interp.F90:134,219,236,251,268,286,307,325,344,363,382,404,431,
// 443.  Semantics: dst(p,k) = sum_j w_pj * src(c_pj, k) for every level k of the
// ungridded dimension, float64 accumulation; the destination is fully overwritten and unmapped points
// are 0.0 (zeroregion=TOTAL + unmappedaction=IGNORE); nearest-neighbour is a pure copy (bit exact).
//
// Every Regrid entry point, mpg_regrid_dev included, goes through ONE dispatcher, mpg_k_apply_typed (k_apply_typed.hip), to
// the gather kernels there (k_apply3_cf, k_apply3_lf_rows, k_apply3_lf, k_apply_generic_t, k_apply1, k_applyN) and the LDS-staged ones of
// k_apply_lfu.hip (k_apply3_cfu, k_apply3_lfu).  This file keeps what that dispatcher reads and the kernels beside it:
//   "a3_staged", "lf_variant" and the other knobs (mpg_k_tune)
//   mpg_zero_planes   the result of a handle that maps nothing
//   K7  k_rotate      rotate_winds_cgrid (interp.F90:737-748)
//       k_pack        the source rows a list of cell ids names, packed (mpg_pack_dev)
#include <string.h>

#include "geom.h"
#include "mpg_internal.h"

static int g_a3_staged = -1;  // "a3_staged" knob: -2 lane-gather only, -1 per-handle choice (default), 0..2 that LDS-staged variant

// "lf_variant" knob: -1 per-handle choice (default) between 0 and 1; 0 row gather on linear aligned tiles
// (k_apply3_lf_rows), 1 level-chunked LDS-staged kernel (k_apply_lfu.hip), 2 row gather on grid-row tiles (k_apply3_lf:
// the capacity fallback)
static int g_lf_variant = -1;

// rotate_winds_cgrid (interp.F90:737-748); evaluated exactly as written (no FMA) -> bit-identical to the oracle
__global__ __launch_bounds__(256) void k_rotate(int64_t npts, int nlev, const double *__restrict__ cosa,
                                                const double *__restrict__ sina, double *__restrict__ u, double *__restrict__ v) {
#pragma clang fp contract(off)
  int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p >= npts) return;
  double ca = cosa[p], sa = sina[p];
  double tana = sa / ca;
  double den = ca + sa * tana;
  for (int k = 0; k < nlev; ++k) {
    int64_t q = (int64_t)k * npts + p;
    double uo = u[q], vo = v[q];
    double t1 = vo * tana;
    double un = (uo + t1) / den;
    double t2 = un * sa;
    double vn = (vo - t2) / ca;
    u[q] = un;
    v[q] = vn;
  }
}

// The adjoint of k_rotate: the reverse mode of interp.F90:737-748 as the header states the forward, in place on the incoming gradients of
// (un, vn); evaluated exactly as written (no FMA), as the forward is
__global__ __launch_bounds__(256) void k_rotate_t(int64_t npts, int nlev, const double *__restrict__ cosa,
                                                  const double *__restrict__ sina, double *__restrict__ gu, double *__restrict__ gv) {
#pragma clang fp contract(off)
  int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p >= npts) return;
  double ca = cosa[p], sa = sina[p];
  double tana = sa / ca;
  double den = ca + sa * tana;
  for (int k = 0; k < nlev; ++k) {
    int64_t q = (int64_t)k * npts + p;
    double gun = gu[q], gvn = gv[q];
    double a = gvn / ca;
    double t = a * sa;
    double b = gun - t;
    double guo = b / den;
    double pp = guo * tana;
    double gvo = a + pp;
    gu[q] = guo;
    gv[q] = gvo;
  }
}

__global__ __launch_bounds__(256) void k_pack(const double *__restrict__ src, int64_t nsrc, int nlev,
                                              const int32_t *__restrict__ ids, int64_t nids, double *__restrict__ dst) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= nids) return;
  int32_t c = ids[i];
  for (int k = 0; k < nlev; ++k) dst[(int64_t)k * nids + i] = src[(int64_t)k * nsrc + c];
}

static int g_store_boxes = 1;
int mpg_store_boxes() { return g_store_boxes; }
static int g_bilinear_linetype = 0;
int mpg_bilinear_linetype() { return g_bilinear_linetype; }
static int g_node_fan_origin = 0;
int mpg_node_fan_origin() { return g_node_fan_origin; }
static int g_grid_inside_tol_exp = 10;
int mpg_grid_inside_tol_exp() { return g_grid_inside_tol_exp; }
int mpg_a3_staged() { return g_a3_staged; }
int mpg_lf_variant() { return g_lf_variant; }

int mpg_k_tune(const char *key, int value) {
  if (!strcmp(key, "lf_variant")) {
    if (value < -1 || value > 2) return MPG_ERR_INVALID_ARG;
    g_lf_variant = value;
    return MPG_SUCCESS;
  }
  if (!strcmp(key, "a3_staged")) {
    if (value < -2 || value >= mpg_cfu_num_variants()) return MPG_ERR_INVALID_ARG;
    g_a3_staged = value;
    return MPG_SUCCESS;
  }
  if (!strcmp(key, "bilinear_linetype")) {   // Mesh -> Grid bilinear Store: where the target point meets the triangle's plane
    if (value != 0 && value != 1) return MPG_ERR_INVALID_ARG;
    g_bilinear_linetype = value;
    return MPG_SUCCESS;
  }
  if (!strcmp(key, "node_fan_origin")) {   // node-located bilinear Store: which listed vertex of a polygon is the apex of its fan (-1: the last one)
    if (value < -8 || value > 15) return MPG_ERR_INVALID_ARG;
    g_node_fan_origin = value;
    return MPG_SUCCESS;
  }
  if (!strcmp(key, "grid_inside_tol_exp")) {   // Grid -> Grid Store: a stagger point is inside a quad of centres within 10^-value of its parametric range
    if (value < 3 || value > 16) return MPG_ERR_INVALID_ARG;
    g_grid_inside_tol_exp = value;
    return MPG_SUCCESS;
  }
  if (!strcmp(key, "store_boxes")) {   // Stores on projection-built grids: candidates from the inverse projection (1) or the pyramid walk (0)
    if (value != 0 && value != 1) return MPG_ERR_INVALID_ARG;
    g_store_boxes = value;
    return MPG_SUCCESS;
  }
  if (!strcmp(key, "nn_variant")) {   // nearest-neighbour Store: 1 = wave-cooperative search, 0 = one thread per point
    if (value != 0 && value != 1) return MPG_ERR_INVALID_ARG;
    mpg_set_nearest_variant(value);
    return MPG_SUCCESS;
  }
  if (!strcmp(key, "field_band")) {
    if (value < -1 || value > 65536) return MPG_ERR_INVALID_ARG;
    mpg_set_field_band(value);
    return MPG_SUCCESS;
  }
  if (!strcmp(key, "lfu_npf")) {   // row slots per thread of the staged level-fast kernel: 0 = by each tile's own list (round 6); 2 .. 32 = at least that many for every tile (A/B: 16 = rounds 1-4)
    if (value != 0 && value != 2 && value != 4 && value != 8 && value != 16 && value != 32) return MPG_ERR_INVALID_ARG;
    mpg_lfu_set_npf(value);
    return MPG_SUCCESS;
  }
  if (!strcmp(key, "staged_lds_pad_kb")) {   // A/B only: extra dynamic LDS (KB) for the staged Regrid kernels = fewer workgroups per CU (the kernels live on L2 keeping what
    if (value < -1 || value > 128) return MPG_ERR_INVALID_ARG;   // they stream, profiles/r06_src_nt_loads.txt: does a smaller in-flight working set pay for the latency hiding it costs?)
    mpg_set_staged_lds_pad_kb(value < 0 ? 0 : value);
    return MPG_SUCCESS;
  }
  if (!strcmp(key, "staged_store")) {   // A/B only: stores of the staged cell-fast kernel: 0 = per lane (geom.h stream_store_lane), 2 = every lane non-temporal
    if (value != 0 && value != 2) return MPG_ERR_INVALID_ARG;
    mpg_set_staged_store(value);
    return MPG_SUCCESS;
  }
  if (!strcmp(key, "lf_rows_store")) {   // store policy of the level-fast row gather: 0 = float32 results per level by the alignment of its plane, float64 per lane (geom.h); 1 = plain, 2 = non-temporal, 3 = per lane (A/B)
    if (value < 0 || value > 3) return MPG_ERR_INVALID_ARG;
    mpg_set_lf_rows_store(value);
    return MPG_SUCCESS;
  }
  if (!strcmp(key, "compose_block_rows")) {   // mpg_handle_compose: 0 = blocks of destination rows by the byte budget alone, n > 0 = of at most n rows as well (the same result)
    if (value < 0) return MPG_ERR_INVALID_ARG;
    mpg_set_compose_block_rows(value);
    return MPG_SUCCESS;
  }
  if (!strcmp(key, "lfu_min_reuse_x10")) {
    if (value < 0 || value > 1000) return MPG_ERR_INVALID_ARG;
    mpg_lfu_set_min_reuse_x10(value);
    return MPG_SUCCESS;
  }
  return MPG_ERR_INVALID_ARG;
}

int mpg_zero_planes(void *dst, size_t esz, int64_t P, int64_t nplanes, int64_t ld, hipStream_t s) {
  if (ld == P) MPG_HIP(hipMemsetAsync(dst, 0, esz * (size_t)P * (size_t)nplanes, s));
  else MPG_HIP(hipMemset2DAsync(dst, esz * (size_t)ld, 0, esz * (size_t)P, (size_t)nplanes, s));
  return MPG_SUCCESS;
}

int mpg_k_rotate(int64_t npts, int nlev, const double *cosa, const double *sina, double *u, double *v, hipStream_t s) {
  if (npts == 0 || nlev == 0) return MPG_SUCCESS;
  k_rotate<<<(unsigned)((npts + 255) / 256), 256, 0, s>>>(npts, nlev, cosa, sina, u, v);
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

int mpg_k_rotate_transpose(int64_t npts, int nlev, const double *cosa, const double *sina, double *gu, double *gv, hipStream_t s) {
  if (npts == 0 || nlev == 0) return MPG_SUCCESS;
  k_rotate_t<<<(unsigned)((npts + 255) / 256), 256, 0, s>>>(npts, nlev, cosa, sina, gu, gv);
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

int mpg_k_pack(const double *src, int64_t n_src, int nlev, const int32_t *ids, int64_t n_ids, double *dst, hipStream_t s) {
  if (n_ids == 0 || nlev == 0) return MPG_SUCCESS;
  k_pack<<<(unsigned)((n_ids + 255) / 256), 256, 0, s>>>(src, n_src, nlev, ids, n_ids, dst);
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_apply() { return (const void *)k_rotate; }
