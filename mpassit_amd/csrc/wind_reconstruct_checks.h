// The argument checks of mpg_reconstruct_store, mpg_reconstruct_weights_dev and mpg_wind_reconstruct_dev and the LDS bytes
// k_wind_reconstruct.hip puts in front of its result tiles.  Plain C++17 without HIP, in the manner of wind_vector_checks.h (whose WvErr,
// wv_overlap and wv_check_handle it uses): mpg_api.hip calls them with what it reads from the handle, and
// tests/c/wind_reconstruct_checks_test.cpp runs the same text on the host (under -fsanitize=address,undefined:
// tests/test_wind_reconstruct_checks.py).  A check returns MPG_SUCCESS or the refusal's code with its message in `err`.
#pragma once
#include "wind_vector_checks.h"

#define WR_LB 4                       // levels a wave carries at a time on [lev][edge] sources
#define WR_UNROLL 4                   // elements of the block's run a thread carries at a time on [edge][lev] sources
#define WR_CHUNK 512                  // entries of a block's run resident in LDS
#define WR_ROWS 64                    // cells of a workgroup (apply_mesh.h AM_CELLS)
#define WR_RP (WR_ROWS + 4)           // row pointers of the run, padded so that what lies behind them stays 8-byte aligned
// bytes of LDS in front of the tiles with nout (2 or 3) results: nout coefficient planes, col, the row pointers
static inline size_t wr_lds_head(int nout) {
  return (size_t)WR_CHUNK * ((size_t)nout * sizeof(double) + sizeof(int32_t)) + WR_RP * sizeof(int32_t);
}

// what the checks read from a handle: WvHandle and the longest row as the Store took it on the host (-1: the handle does not know it)
struct WrHandle : WvHandle {
  int64_t max_row;
};

// The pattern of mpg_reconstruct_store; out: the entries and the longest row.  Only host arrays are read.
static inline int wr_check_store(int64_t nCells, int64_t nEdges, int maxEdges, const int32_t *nEdgesOnCell, const int32_t *edgesOnCell,
                                 const void *out, int64_t *nnz, int64_t *max_row, WvErr &e) {
  const char *who = "mpg_reconstruct_store";
  if (!(nEdgesOnCell && edgesOnCell && out)) return e.fail(MPG_ERR_INVALID_ARG, who, "NULL argument (nEdgesOnCell_host, edgesOnCell_host and out are required)");
  if (!(nCells >= 1 && nEdges >= 1 && maxEdges >= 0)) return e.fail(MPG_ERR_INVALID_ARG, who, "bad sizes (nCells >= 1, nEdges >= 1, maxEdges >= 0)");
  if (nCells >= 0x7fffffff || nEdges >= 0x7fffffff) return e.fail(MPG_ERR_OVERFLOW, who, "nCells or nEdges beyond int32");
  int64_t n = 0, longest = 0;
  for (int64_t c = 0; c < nCells; ++c) {
    const int32_t len = nEdgesOnCell[c];
    if (len < 0 || len > maxEdges) {
      snprintf(e.msg, sizeof e.msg, "%s: cell %lld has nEdgesOnCell %d outside [0, maxEdges = %d]", who, (long long)c, len, maxEdges);
      return MPG_ERR_INVALID_ARG;
    }
    for (int32_t i = 0; i < len; ++i) {
      const int32_t id = edgesOnCell[c * (int64_t)maxEdges + i];
      if (id < 1 || id > nEdges) {
        snprintf(e.msg, sizeof e.msg, "%s: cell %lld slot %d has edge id %d outside [1, nEdges = %lld] (ids are 1-based)", who, (long long)c, i, id,
                 (long long)nEdges);
        return MPG_ERR_INVALID_ARG;
      }
    }
    n += len;
    if (len > longest) longest = len;
    if (n >= 0x7fffffff) return e.fail(MPG_ERR_OVERFLOW, who, "more than 2^31 - 2 entries");
  }
  *nnz = n;
  *max_row = longest;
  return MPG_SUCCESS;
}

// *nothing: the handle has no entries, success without a launch
static inline int wr_check_weights(const WrHandle *h, int maxEdges, const double *coeffs, const double *dst_frames, const double *m, bool *nothing,
                                   WvErr &e) {
  const char *who = "mpg_reconstruct_weights";
  *nothing = false;
  int rc = wv_check_handle(who, h, e);
  if (rc) return rc;
  if (maxEdges < 0) return e.fail(MPG_ERR_INVALID_ARG, who, "maxEdges must be >= 0");
  if (h->max_row < 0)
    return e.fail(MPG_ERR_INVALID_ARG, who, "the handle does not record its longest row: this call takes a handle of mpg_reconstruct_store "
                                            "(or of mpg_handle_from_weights)");
  if (h->max_row > maxEdges) {
    snprintf(e.msg, sizeof e.msg, "%s: the handle's longest row has %lld entries, which exceeds maxEdges = %d: coeffs_dev [nCells][maxEdges][3] "
                                  "has no slot for them", who, (long long)h->max_row, maxEdges);
    return MPG_ERR_INVALID_ARG;
  }
  if (h->nnz == 0) {
    *nothing = true;
    return MPG_SUCCESS;
  }
  if (!(coeffs && m)) return e.fail(MPG_ERR_INVALID_ARG, who, "NULL array (coeffs_dev and m_dev are required; dst_frames_dev may be NULL: X, Y, Z)");
  if (h->n_dst > (INT64_MAX / 24) / (maxEdges > 0 ? maxEdges : 1)) return e.fail(MPG_ERR_INVALID_ARG, who, "coeffs_dev [nCells][maxEdges][3] cannot be addressed");
  const uintptr_t nm = (dst_frames ? 2 : 3) * (uintptr_t)h->nnz * sizeof(double);
  const uintptr_t nc = 3 * (uintptr_t)maxEdges * (uintptr_t)h->n_dst * sizeof(double), nd = 6 * (uintptr_t)h->n_dst * sizeof(double);
  if (wv_overlap(m, nm, coeffs, nc) || wv_overlap(m, nm, dst_frames, nd))
    return e.fail(MPG_ERR_INVALID_ARG, who, "m_dev may not alias an input (coeffs_dev, dst_frames_dev): give the blocks their own array of nout * nnz doubles");
  return MPG_SUCCESS;
}

// The checks of the apply; out: the source's level stride in elements ([lev][edge] sources; n_src otherwise).
static inline int wr_check_apply(const WrHandle *h, const double *m, int nout, const void *u, int src_type, int src_layout, int64_t u_level_stride,
                                 int nlev, const void *r0, const void *r1, const void *r2, int dst_type, int dst_layout, int64_t *ldu, WvErr &e) {
  const char *who = "mpg_wind_reconstruct";
  if (!h) return e.fail(MPG_ERR_INVALID_ARG, who, "NULL handle");
  if (nout == 1)
    return e.fail(MPG_ERR_INVALID_ARG, who, "nout must be 2 or 3; one result is a scalar Regrid: mpg_regrid_csr_to_mesh_dev / mpg_regrid_csr_rows_dev "
                                            "of a from-weights handle serve it");
  if (nout != 2 && nout != 3) return e.fail(MPG_ERR_INVALID_ARG, who, "nout must be 2 or 3");
  if ((r2 != nullptr) != (nout == 3)) return e.fail(MPG_ERR_INVALID_ARG, who, "r2_dev is given exactly when nout == 3");
  if (!((u || h->n_src == 0) && ((r0 && r1) || h->n_dst == 0) && (m || h->nnz == 0)))
    return e.fail(MPG_ERR_INVALID_ARG, who, "NULL array (m_dev, u_dev, r0_dev and r1_dev are required)");
  if (nlev < 1) return e.fail(MPG_ERR_INVALID_ARG, who, "nlev must be >= 1");
  if (dst_layout != MPG_LAYOUT_CELL_FAST && dst_layout != MPG_LAYOUT_LEV_FAST) return e.fail(MPG_ERR_INVALID_ARG, who, "bad dst_layout");
  if (src_layout != MPG_LAYOUT_CELL_FAST && src_layout != MPG_LAYOUT_LEV_FAST) return e.fail(MPG_ERR_INVALID_ARG, who, "bad src_layout");
  if (!(src_type >= 0 && src_type <= 3 && dst_type >= 0 && dst_type <= 3))
    return e.fail(MPG_ERR_INVALID_ARG, who, "src_type / dst_type must be MPG_TYPE_F64 or MPG_TYPE_F32");
  if ((src_type | dst_type) & MPG_TYPE_BE)
    return e.fail(MPG_ERR_UNSUPPORTED, who, "big-endian values (MPG_TYPE_BE) are not supported; mpg_bswap_dev swaps an array in place before or after the call");
  int rc = wv_check_handle(who, h, e);
  if (rc) return rc;
  const int es = (src_type & MPG_TYPE_F32) ? 4 : 8, ed = (dst_type & MPG_TYPE_F32) ? 4 : 8;
  int64_t ld = u_level_stride;
  if (src_layout == MPG_LAYOUT_LEV_FAST) {   // u[nEdges][nlev], file order: dense
    if (ld != 0) return e.fail(MPG_ERR_INVALID_ARG, who, "u_level_stride must be 0 with MPG_LAYOUT_LEV_FAST sources (u[nEdges][nlev] is dense)");
    ld = h->n_src;
  } else {
    if (ld == 0) ld = h->n_src;
    if (ld < h->n_src) {
      snprintf(e.msg, sizeof e.msg, "%s: u_level_stride %lld is below the source plane of %lld edges (0 = dense)", who, (long long)ld, (long long)h->n_src);
      return MPG_ERR_INVALID_ARG;
    }
  }
  if (ld > 0 && (int64_t)nlev > (INT64_MAX / es) / ld) {
    snprintf(e.msg, sizeof e.msg, "%s: %d planes of u_level_stride %lld cannot be addressed", who, nlev, (long long)ld);
    return MPG_ERR_INVALID_ARG;
  }
  if (h->n_dst > 0 && (int64_t)nlev > (INT64_MAX / ed) / h->n_dst) return e.fail(MPG_ERR_INVALID_ARG, who, "nlev planes of n_dst results cannot be addressed");
  // more 64-row blocks than one launch holds
  if (((uint64_t)h->n_dst + WR_ROWS - 1) / WR_ROWS > 0x7fffffffull) {
    snprintf(e.msg, sizeof e.msg, "%s: %lld cells exceed one launch", who, (long long)h->n_dst);
    return MPG_ERR_OVERFLOW;
  }
  // no result may alias another, the source or the blocks (a workgroup's stores would race another's loads)
  const uintptr_t nb = (uintptr_t)nlev * (uintptr_t)h->n_dst * (uintptr_t)ed;
  const uintptr_t nm = (uintptr_t)nout * (uintptr_t)h->nnz * sizeof(double);
  const uintptr_t nu = (uintptr_t)nlev * (uintptr_t)ld * (uintptr_t)es;
  if (wv_overlap(r0, nb, r1, nb) || wv_overlap(r0, nb, r2, nb) || wv_overlap(r1, nb, r2, nb))
    return e.fail(MPG_ERR_INVALID_ARG, who, "results alias each other: give each result its own array");
  for (const void *r : {r0, r1, r2}) {
    if (wv_overlap(r, nb, u, nu)) return e.fail(MPG_ERR_INVALID_ARG, who, "a result may not alias the source (u_dev): give each result its own array");
    if (wv_overlap(r, nb, m, nm)) return e.fail(MPG_ERR_INVALID_ARG, who, "a result may not alias the blocks (m_dev): give each result its own array");
  }
  *ldu = ld;
  return MPG_SUCCESS;
}
