// The argument checks of mpg_handle_compose and mpg_compose_weights_dev and the block plan of k_compose.hip's symbolic job.  Plain C++17
// without HIP, in the manner of wind_vector_checks.h (whose WvErr and wv_overlap it uses): mpg_api.hip calls the checks with what it
// reads from the handles, k_compose.hip plans its blocks of destination rows with co_next_block, and tests/c/compose_checks_test.cpp runs
// the same text on the host (under -fsanitize=address,undefined: tests/test_compose_checks.py).  A check returns MPG_SUCCESS or the
// refusal's code with its message in `err` (the call's name and the way out).
#pragma once
#include "wind_vector_checks.h"

#define CO_MAX_NNZ 0x7ffffffell               // entries of a composite (2^31 - 2): rowptr is int32
#define CO_MAX_BLOCK_CAND 0x7ffffffell        // candidates of one block of destination rows: the block's offsets are int32
#define CO_BUDGET_BYTES (1ll << 30)           // temporaries of the symbolic job, per block ...
#define CO_BYTES_PER_CAND 40ll                // ... at two 64-bit keys, two int32 (heads, positions) and the sort's own buffers per candidate
#define CO_BLOCK_CAND (CO_BUDGET_BYTES / CO_BYTES_PER_CAND)   // candidates a block takes before it is closed (a single longer row is a block)
#define CO_BLOCK_ROWS_MAX 0x7fffffff          // "compose_block_rows" knob: 0 = by the budget alone, n > 0 = at most n rows per block as well
// Entries of a row that a workgroup of the symbolic job would sort in LDS.  0: there is no per-row LDS stage; every row, short or long,
// goes through the device-wide sort of (row, column) keys, so no row length takes another path.
#define CO_LDS_ROW_ENTRIES 0
#define CO_MAX_PLANES 4                       // value planes of mpg_compose_weights_dev

// what the checks read from a handle (mpg_handle_s in mpg_internal.h)
struct CoHandle {
  bool csr;
  int64_t n_pole, n_src, n_dst, nnz;
};

static inline int co_check_pole(const char *who, const char *which, const CoHandle *h, WvErr &e) {
  if (h->n_pole > 0) {
    snprintf(e.msg, sizeof e.msg, "%s: `%s` has pole-cap terms (periodic Grid -> Grid, mpg_handle_pole_count > 0), which are not entries of "
                                  "its matrix; to_esmf_weights' (row, col, S) of such a handle, given to mpg_handle_from_weights, is a CSR handle "
                                  "that composes", who, which);
    return MPG_ERR_UNSUPPORTED;
  }
  return MPG_SUCCESS;
}

// mpg_handle_compose: C = outer . inner
static inline int co_check_compose(const CoHandle *outer, const CoHandle *inner, const void *out, WvErr &e) {
  const char *who = "mpg_handle_compose";
  if (!(outer && inner && out)) return e.fail(MPG_ERR_INVALID_ARG, who, "NULL argument (outer, inner and out are required)");
  if (inner->n_dst != outer->n_src) {
    snprintf(e.msg, sizeof e.msg, "%s: the handles do not chain: inner has n_dst = %lld, outer has n_src = %lld (a localized or rebased outer "
                                  "indexes a packed source: compose first, then localize the composite)", who, (long long)inner->n_dst,
             (long long)outer->n_src);
    return MPG_ERR_INVALID_ARG;
  }
  int rc = co_check_pole(who, "outer", outer, e);
  if (!rc) rc = co_check_pole(who, "inner", inner, e);
  return rc;
}

// The next block of destination rows of the symbolic job: rows [r0, *r1) with *ncand candidates.  cnt[i] is row i's candidate count
// before de-duplication, a 64-bit quantity; a block closes before the row that would take it past `cap` candidates or `block_rows` rows
// (0: no row limit) and always holds at least one row, so a row longer than `cap` is a block of its own -- up to CO_MAX_BLOCK_CAND.
static inline int co_next_block(const int64_t *cnt, int64_t n, int64_t r0, int64_t cap, int64_t block_rows, int64_t *r1, int64_t *ncand, WvErr &e) {
  const char *who = "mpg_handle_compose";
  if (cap > CO_MAX_BLOCK_CAND) cap = CO_MAX_BLOCK_CAND;
  int64_t r = r0, sum = 0;
  while (r < n && (block_rows <= 0 || r - r0 < block_rows)) {
    const int64_t c = cnt[r];
    if (c < 0 || c > CO_MAX_BLOCK_CAND) {
      snprintf(e.msg, sizeof e.msg, "%s: destination row %lld alone reaches %lld (outer entry, inner entry) pairs, beyond the 2^31 - 2 one "
                                    "block of rows sorts; split that row of `outer` over two handles", who, (long long)r, (long long)c);
      return MPG_ERR_OVERFLOW;
    }
    if (r > r0 && c > cap - sum) break;   // (sum <= cap here, so cap - sum cannot wrap)
    sum += c;
    ++r;
    if (sum >= cap) break;
  }
  *r1 = r;
  *ncand = sum;
  return MPG_SUCCESS;
}

// the composite's entry count so far (after de-duplication): rowptr is int32
static inline int co_check_nnz(int64_t nnz, WvErr &e) {
  if (nnz < 0 || nnz > CO_MAX_NNZ) {
    snprintf(e.msg, sizeof e.msg, "mpg_handle_compose: the composite has more than 2^31 - 2 entries (%lld so far) and rowptr is int32; compose "
                                  "blocks of `outer`'s destination rows into separate handles", (long long)nnz);
    return MPG_ERR_OVERFLOW;
  }
  return MPG_SUCCESS;
}

// mpg_compose_weights_dev; *nothing: the composite has no entries, success without a launch
static inline int co_check_weights(const CoHandle *composed, const CoHandle *outer, const CoHandle *inner, int nplanes, const double *inner_m,
                                   const double *m, bool *nothing, WvErr &e) {
  const char *who = "mpg_compose_weights";
  *nothing = false;
  if (!(composed && outer && inner)) return e.fail(MPG_ERR_INVALID_ARG, who, "NULL handle (composed, outer and inner are required)");
  if (nplanes < 1 || nplanes > CO_MAX_PLANES) {
    snprintf(e.msg, sizeof e.msg, "%s: nplanes = %d is outside 1..%d; more planes take several calls", who, nplanes, CO_MAX_PLANES);
    return MPG_ERR_INVALID_ARG;
  }
  int rc = co_check_pole(who, "composed", composed, e);
  if (!rc) rc = co_check_pole(who, "outer", outer, e);
  if (!rc) rc = co_check_pole(who, "inner", inner, e);
  if (rc) return rc;
  if (!inner->csr)
    return e.fail(MPG_ERR_UNSUPPORTED, who, "`inner` is a fixed 1-, 3- or 4-slot handle and the planes are defined on CSR entries. "
                                            "mpg_handle_get_weights, then mpg_handle_from_weights, makes a CSR handle of a fixed one.");
  if (!composed->csr) return e.fail(MPG_ERR_UNSUPPORTED, who, "`composed` is a fixed handle: this call takes the CSR handle of mpg_handle_compose");
  if (composed->n_dst != outer->n_dst || composed->n_src != inner->n_src || inner->n_dst != outer->n_src) {
    snprintf(e.msg, sizeof e.msg, "%s: the sizes do not chain: composed is %lld x %lld, outer %lld x %lld, inner %lld x %lld (n_dst x n_src); "
                                  "give the two handles `composed` was made of", who, (long long)composed->n_dst, (long long)composed->n_src,
             (long long)outer->n_dst, (long long)outer->n_src, (long long)inner->n_dst, (long long)inner->n_src);
    return MPG_ERR_INVALID_ARG;
  }
  if (composed->nnz == 0) {
    *nothing = true;
    return MPG_SUCCESS;
  }
  if (!(m && (inner_m || inner->nnz == 0))) return e.fail(MPG_ERR_INVALID_ARG, who, "NULL array (inner_m_dev and m_dev are required)");
  const uintptr_t nb = (uintptr_t)nplanes * (uintptr_t)inner->nnz * sizeof(double), nc = (uintptr_t)nplanes * (uintptr_t)composed->nnz * sizeof(double);
  if (wv_overlap(m, nc, inner_m, nb))
    return e.fail(MPG_ERR_INVALID_ARG, who, "m_dev may not alias inner_m_dev: give the composite's planes their own array of nplanes * nnz doubles");
  return MPG_SUCCESS;
}
