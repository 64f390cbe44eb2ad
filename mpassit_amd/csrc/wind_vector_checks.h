// The argument checks of mpg_sphere_frames_dev, mpg_wind_vector_weights_dev and mpg_wind_vector_dev and the LDS bytes k_wind_vector.hip
// puts in front of its result tiles.  Plain C++17 without HIP: mpg_api.hip calls them with what it reads from the handle, and
// tests/c/wind_vector_checks_test.cpp runs the same text on the host (under -fsanitize=address,undefined: tests/test_wind_vector_checks.py).
// A check returns MPG_SUCCESS or the refusal's code with its message in `err` (the call's name and the way out).
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "../../include/mpassit_amd.h"

#define WV_LB 4                       // levels a wave of k_wind_vector carries at a time
#define WV_CHUNK 384                  // entries of a block's run resident in LDS
#define WV_ROWS 64                    // destination points of a workgroup (apply_mesh.h AM_CELLS)
#define WV_RP (WV_ROWS + 4)           // row pointers of the run, padded so that what lies behind them stays 8-byte aligned
// bytes of LDS in front of the tiles with nout (1 or 2) results: 2 nout coefficient planes, col, the row pointers
static inline size_t wv_lds_head(int nout) {
  return (size_t)WV_CHUNK * (2 * (size_t)nout * sizeof(double) + sizeof(int32_t)) + WV_RP * sizeof(int32_t);
}

struct WvErr {
  char msg[512];
  int fail(int rc, const char *who, const char *what) {
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return rc;
  }
};

// what the checks read from a handle (mpg_handle_s in mpg_internal.h)
struct WvHandle {
  bool csr;
  int64_t n_pole, n_src, n_dst, nnz;
};

static inline bool wv_overlap(const void *p, uintptr_t np, const void *q, uintptr_t nq) {
  return p && q && (uintptr_t)p < (uintptr_t)q + nq && (uintptr_t)q < (uintptr_t)p + np;
}

static inline int wv_check_frames(int64_t n, const double *lon, const double *lat, const double *c, const double *s, const double *frames, WvErr &e) {
  const char *who = "mpg_sphere_frames";
  if (n < 0) return e.fail(MPG_ERR_INVALID_ARG, who, "n must be >= 0");
  if (!(lon && lat && frames)) return e.fail(MPG_ERR_INVALID_ARG, who, "NULL array (lon_dev, lat_dev and frames_dev are required)");
  if ((c == nullptr) != (s == nullptr)) return e.fail(MPG_ERR_INVALID_ARG, who, "c_dev and s_dev come together (both NULL: east and north)");
  if (n > INT64_MAX / (int64_t)(6 * sizeof(double))) return e.fail(MPG_ERR_INVALID_ARG, who, "six planes of n points cannot be addressed");
  const uintptr_t nf = 6 * (uintptr_t)n * sizeof(double), na = (uintptr_t)n * sizeof(double);
  for (const double *in : {lon, lat, c, s})
    if (wv_overlap(frames, nf, in, na))
      return e.fail(MPG_ERR_INVALID_ARG, who, "frames_dev may not alias an input: give the frames their own array of 6 * n doubles");
  return MPG_SUCCESS;
}

// the handle of the two vector calls: a CSR one without pole terms (h == nullptr: a NULL handle)
static inline int wv_check_handle(const char *who, const WvHandle *h, WvErr &e) {
  if (!h) return e.fail(MPG_ERR_INVALID_ARG, who, "NULL handle");
  if (h->n_pole > 0)   // (whatever its kind: the message that helps is the one about the pole terms)
    return e.fail(MPG_ERR_UNSUPPORTED, who, "handles with pole-cap terms (periodic Grid -> Grid, mpg_handle_pole_count > 0) are not supported; "
                                            "mpg_regrid_typed_dev on each component, then the rotation, serves them");
  if (!h->csr)
    return e.fail(MPG_ERR_UNSUPPORTED, who, "fixed 1-, 3- and 4-slot handles are not supported: this call takes a CSR handle. "
                                            "mpg_handle_get_weights, then mpg_handle_from_weights, makes a CSR handle of a fixed one.");
  return MPG_SUCCESS;
}

// *nothing: the handle has no entries, success without a launch
static inline int wv_check_weights(const WvHandle *h, const double *src_frames, const double *dst_frames, const double *m, bool *nothing, WvErr &e) {
  const char *who = "mpg_wind_vector_weights";
  *nothing = false;
  int rc = wv_check_handle(who, h, e);
  if (rc) return rc;
  if (h->nnz == 0) {
    *nothing = true;
    return MPG_SUCCESS;
  }
  if (!(src_frames && dst_frames && m)) return e.fail(MPG_ERR_INVALID_ARG, who, "NULL array (src_frames_dev, dst_frames_dev and m_dev are required)");
  const uintptr_t nm = 4 * (uintptr_t)h->nnz * sizeof(double);
  const uintptr_t ns = 6 * (uintptr_t)h->n_src * sizeof(double), nd = 6 * (uintptr_t)h->n_dst * sizeof(double);
  if (wv_overlap(m, nm, src_frames, ns) || wv_overlap(m, nm, dst_frames, nd))
    return e.fail(MPG_ERR_INVALID_ARG, who, "m_dev may not alias the frames: give the blocks their own array of 4 * nnz doubles");
  return MPG_SUCCESS;
}

// The checks of the CSR wind calls for ONE handle and its blocks in place of the angles; out: the level strides in elements.
static inline int wv_check_apply(const WvHandle *h, const double *m, const void *u, const void *v, int src_type, int64_t u_level_stride,
                                 int64_t v_level_stride, int nlev, const void *r0, const void *r1, int dst_type, int dst_layout, int64_t *ldu,
                                 int64_t *ldv, WvErr &e) {
  const char *who = "mpg_wind_vector";
  if (!h) return e.fail(MPG_ERR_INVALID_ARG, who, "NULL handle");
  if (!(((u && v) || h->n_src == 0) && (r0 || h->n_dst == 0) && (m || h->nnz == 0)))
    return e.fail(MPG_ERR_INVALID_ARG, who, "NULL array (m_dev, u_dev, v_dev and r0_dev are required; r1_dev may be NULL: r0 alone)");
  if (nlev < 1) return e.fail(MPG_ERR_INVALID_ARG, who, "nlev must be >= 1");
  if (dst_layout != MPG_LAYOUT_CELL_FAST && dst_layout != MPG_LAYOUT_LEV_FAST) return e.fail(MPG_ERR_INVALID_ARG, who, "bad dst_layout");
  if (!(src_type >= 0 && src_type <= 3 && dst_type >= 0 && dst_type <= 3))
    return e.fail(MPG_ERR_INVALID_ARG, who, "src_type / dst_type must be MPG_TYPE_F64 or MPG_TYPE_F32");
  if ((src_type | dst_type) & MPG_TYPE_BE)
    return e.fail(MPG_ERR_UNSUPPORTED, who, "big-endian values (MPG_TYPE_BE) are not supported; mpg_bswap_dev swaps an array in place before or after the call");
  int rc = wv_check_handle(who, h, e);
  if (rc) return rc;
  const int es = (src_type & MPG_TYPE_F32) ? 4 : 8, ed = (dst_type & MPG_TYPE_F32) ? 4 : 8;
  int64_t ld[2] = {u_level_stride, v_level_stride};
  const char *ldname[2] = {"u_level_stride", "v_level_stride"};
  for (int i = 0; i < 2; ++i) {   // a source's level stride: 0 = dense, else at least the plane, and nlev planes of it addressable
    if (ld[i] == 0) ld[i] = h->n_src;
    if (ld[i] < h->n_src) {
      snprintf(e.msg, sizeof e.msg, "%s: %s %lld is below the source plane of %lld points (0 = dense)", who, ldname[i], (long long)ld[i], (long long)h->n_src);
      return MPG_ERR_INVALID_ARG;
    }
    if (ld[i] > 0 && (int64_t)nlev > (INT64_MAX / es) / ld[i]) {
      snprintf(e.msg, sizeof e.msg, "%s: %d planes of %s %lld cannot be addressed", who, nlev, ldname[i], (long long)ld[i]);
      return MPG_ERR_INVALID_ARG;
    }
  }
  if (h->n_dst > 0 && (int64_t)nlev > (INT64_MAX / ed) / h->n_dst) return e.fail(MPG_ERR_INVALID_ARG, who, "nlev planes of n_dst results cannot be addressed");
  // more 64-point blocks than one launch holds
  if (((uint64_t)h->n_dst + WV_ROWS - 1) / WV_ROWS > 0x7fffffffull) {
    snprintf(e.msg, sizeof e.msg, "%s: %lld points exceed one launch", who, (long long)h->n_dst);
    return MPG_ERR_OVERFLOW;
  }
  // neither result may alias the other, a source or the blocks (a workgroup's stores would race another's loads)
  const uintptr_t nb = (uintptr_t)nlev * (uintptr_t)h->n_dst * (uintptr_t)ed;
  const uintptr_t nm = (r1 ? 4 : 2) * (uintptr_t)h->nnz * sizeof(double);
  const uintptr_t nu = (uintptr_t)nlev * (uintptr_t)ld[0] * (uintptr_t)es, nv = (uintptr_t)nlev * (uintptr_t)ld[1] * (uintptr_t)es;
  if (wv_overlap(r0, nb, r1, nb)) return e.fail(MPG_ERR_INVALID_ARG, who, "r0_dev and r1_dev alias each other: give each result its own array");
  for (const void *r : {r0, r1}) {
    if (wv_overlap(r, nb, u, nu) || wv_overlap(r, nb, v, nv))
      return e.fail(MPG_ERR_INVALID_ARG, who, "a result may not alias a source (u_dev, v_dev): give each result its own array");
    if (wv_overlap(r, nb, m, nm)) return e.fail(MPG_ERR_INVALID_ARG, who, "a result may not alias the blocks (m_dev): give each result its own array");
  }
  *ldu = ld[0];
  *ldv = ld[1];
  return MPG_SUCCESS;
}
