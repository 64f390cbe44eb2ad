// Store-time masks on a finished handle (mpg_handle_mask): static source / destination masks applied to a route handle's pattern, as a
// NEW handle of the same shape (include/mpassit_amd.h states the contract).  It needs no geometry.  Three passes, one thread per row:
//
//   pass 1  k_hm_flag      per row: bydst (the destination mask unmaps a mapped row), bysrc (the source rule does), the output length and the
//                          stored entries the row loses.  MPG_MASKRULE_ROW: a row is unmapped when a stored entry (index >= 0, whatever its
//                          weight) references a masked source.  MPG_MASKRULE_ENTRY (CSR): hm_entry_row (handle_mask.h) without outputs.
//   pass 2  mpg_sum_i32_i64 of the three counters (the statistics), mpg_scan_excl_i32 of the lengths (a CSR output's rowptr)
//   pass 3  k_hm_fill_fixed   every row copied; an unmapped row as the Stores write one: every index -1, every weight +0.0
//           k_hm_fill_csr     mapped rows through hm_entry_row (ENTRY) or copied (ROW), unmapped rows empty; dst_frac carried where the
//                             input has one; the longest row recorded (an integer maximum)
// No floating-point atomics, no LDS: the same bytes from run to run.
#include "mpg_internal.h"
#include "handle_mask.h"

#define HM_MAX_SLOTS 4   // slots per row of a fixed handle (3, 4 or 1)

struct HmIn {
  const int32_t *rowptr;   // CSR row pointers; nullptr: fixed slots
  const int32_t *col;      // CSR columns, or idx [nz][n] (-1 = none)
  const double *val;       // CSR values, or w [nz][n]; nullptr: a nearest handle without weights
  const double *frac;      // dst_frac [n] or nullptr
  int nz;                  // slots of a fixed handle
  int64_t n;               // rows
  const uint8_t *src_mask, *dst_mask;   // either may be nullptr
  int entry;               // MPG_MASKRULE_ENTRY (CSR only)
  int norm_type;
};

static inline unsigned hm_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

// all four arrays have n + 1 elements, element n = 0 (the scan's last entry is the count)
__global__ __launch_bounds__(256) void k_hm_flag(HmIn in, int32_t *__restrict__ bysrc, int32_t *__restrict__ bydst, int32_t *__restrict__ lost,
                                                 int32_t *__restrict__ len) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > in.n) return;
  int had = 0, now = 0, fs = 0, fd = 0;
  if (i < in.n) {
    const bool dm = in.dst_mask && in.dst_mask[i];
    if (in.rowptr) {
      const int64_t b = in.rowptr[i];
      had = in.rowptr[i + 1] - (int32_t)b;
      if (dm) now = 0;
      else if (in.entry) {
        double f;
        now = hm_entry_row(in.col + b, in.val + b, had, in.src_mask, in.norm_type, 0.0, nullptr, nullptr, &f);
      } else {
        bool hit = false;
        if (in.src_mask)
          for (int q = 0; q < had; ++q) hit |= in.src_mask[in.col[b + q]] != 0;
        now = hit ? 0 : had;
      }
    } else {
      bool hit = false;
      for (int s = 0; s < in.nz; ++s) {
        const int32_t c = in.col[(int64_t)s * in.n + i];
        if (c < 0) continue;
        ++had;
        if (in.src_mask) hit |= in.src_mask[c] != 0;
      }
      now = (dm || hit) ? 0 : had;
    }
    fd = dm && had > 0;
    fs = !dm && had > 0 && now == 0;
  }
  bysrc[i] = fs;
  bydst[i] = fd;
  lost[i] = had - now;
  len[i] = now;
}

__global__ __launch_bounds__(256) void k_hm_fill_fixed(HmIn in, const int32_t *__restrict__ bysrc, const int32_t *__restrict__ bydst,
                                                       int32_t *__restrict__ out_idx, double *__restrict__ out_w) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= in.n) return;
  const bool gone = bysrc[i] | bydst[i];
#pragma unroll
  for (int s = 0; s < HM_MAX_SLOTS; ++s)
    if (s < in.nz) {
      const int64_t at = (int64_t)s * in.n + i;
      out_idx[at] = gone ? -1 : in.col[at];
      if (out_w) out_w[at] = gone ? 0.0 : in.val[at];
    }
}

__global__ __launch_bounds__(256) void k_hm_fill_csr(HmIn in, const int32_t *__restrict__ rowptr, int32_t *__restrict__ col, double *__restrict__ val,
                                                     double *__restrict__ frac_out, int32_t *__restrict__ longest) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int32_t len = 0;
  if (i < in.n) {
    const int64_t at = rowptr[i], b = in.rowptr[i];
    len = rowptr[i + 1] - (int32_t)at;
    const int had = in.rowptr[i + 1] - (int32_t)b;
    const double fin = in.frac ? in.frac[i] : 0.0;
    double f = fin;
    if (in.dst_mask && in.dst_mask[i]) {
      f = 0.0;
    } else if (in.entry) {
      hm_entry_row(in.col + b, in.val + b, had, in.src_mask, in.norm_type, fin, col + at, val + at, &f);
    } else if (len == had) {
      for (int q = 0; q < len; ++q) {
        col[at + q] = in.col[b + q];
        val[at + q] = in.val[b + q];
      }
    } else {
      f = 0.0;   // (the ROW rule emptied a row of a handle that carries a fraction)
    }
    if (frac_out) frac_out[i] = f;
  }
  for (int o = 32; o > 0; o >>= 1) len = max(len, __shfl_down(len, o));
  if ((threadIdx.x & 63) == 0 && len > 0) atomicMax(longest, len);   // (an integer maximum: the order does not matter)
}

// in: the handle to mask; out: shape and method set by the caller, arrays empty.  entry: the resolved rule.  Blocking.
int mpg_k_handle_mask(mpg_handle_s *in, const uint8_t *src_mask, const uint8_t *dst_mask, bool entry, int norm_type, mpg_handle_s *out,
                      hipStream_t s) {
  int rc;
  const int64_t n = in->n_dst;
  const bool csr = in->kind == MPG_KIND_CSR;
  if (!csr && in->nnz_per_row > HM_MAX_SLOTS) {
    mpg_set_error("mpg_handle_mask: a fixed handle of %d slots per row is not served (%d at most)", in->nnz_per_row, HM_MAX_SLOTS);
    return MPG_ERR_UNSUPPORTED;
  }
  HmIn I;
  I.rowptr = csr ? in->rowptr.p : nullptr;
  I.col = csr ? in->col.p : in->idx.p;
  I.val = csr ? in->val.p : in->w.p;
  I.frac = in->dst_frac.p;
  I.nz = csr ? 0 : in->nnz_per_row;
  I.n = n;
  I.src_mask = src_mask;
  I.dst_mask = dst_mask;
  I.entry = entry;
  I.norm_type = norm_type;
  // pass 1
  TmpBuf<int32_t> bysrc, bydst, lost, len, longest;
  TmpBuf<long long> sums;
  if ((rc = bysrc.alloc((size_t)n + 1, s)) || (rc = bydst.alloc((size_t)n + 1, s)) || (rc = lost.alloc((size_t)n + 1, s)) ||
      (rc = len.alloc((size_t)n + 1, s)) || (rc = sums.alloc(4, s)) || (rc = longest.alloc(1, s)))
    return rc;
  k_hm_flag<<<hm_grid(n + 1), 256, 0, s>>>(I, bysrc.p, bydst.p, lost.p, len.p);
  MPG_HIP(hipGetLastError());
  // pass 2
  if ((rc = mpg_sum_i32_i64(bysrc.p, n + 1, sums.p, s)) || (rc = mpg_sum_i32_i64(bydst.p, n + 1, sums.p + 1, s)) ||
      (rc = mpg_sum_i32_i64(lost.p, n + 1, sums.p + 2, s)) || (rc = mpg_sum_i32_i64(len.p, n + 1, sums.p + 3, s)))
    return rc;
  long long h[4] = {0, 0, 0, 0};
  MPG_HIP(hipMemcpyAsync(h, sums.p, sizeof h, hipMemcpyDeviceToHost, s));
  MPG_HIP(hipStreamSynchronize(s));
  out->store_stats[1] = h[0];
  out->store_stats[2] = h[1];
  out->store_stats[3] = h[2];
  if (in->dst_frac.p && (rc = out->dst_frac.alloc((size_t)n))) return rc;
  // pass 3
  if (!csr) {
    const int nz = in->nnz_per_row;
    out->kind = MPG_KIND_FIXED;
    out->nnz_per_row = nz;
    out->nnz = in->nnz;
    if ((rc = out->idx.alloc((size_t)nz * (size_t)n))) return rc;
    if (in->w.p && (rc = out->w.alloc((size_t)nz * (size_t)n))) return rc;
    if (n > 0) {
      k_hm_fill_fixed<<<hm_grid(n), 256, 0, s>>>(I, bysrc.p, bydst.p, out->idx.p, out->w.p);
      MPG_HIP(hipGetLastError());
      if (out->dst_frac.p) MPG_HIP(hipMemcpyAsync(out->dst_frac.p, in->dst_frac.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, s));
    }
    MPG_HIP(hipStreamSynchronize(s));   // the temporaries may go
    return MPG_SUCCESS;
  }
  const long long nnz = h[3];   // (never above the input's: nothing can overflow here)
  out->kind = MPG_KIND_CSR;
  out->nnz_per_row = 0;
  out->nnz = nnz;
  if ((rc = out->rowptr.alloc((size_t)n + 1)) || (rc = out->col.alloc((size_t)nnz + 1)) || (rc = out->val.alloc((size_t)nnz + 1))) return rc;
  if ((rc = mpg_scan_excl_i32(len.p, out->rowptr.p, n + 1, s))) return rc;
  MPG_HIP(hipMemsetAsync(longest.p, 0, sizeof(int32_t), s));
  if (n > 0) {
    k_hm_fill_csr<<<hm_grid(n), 256, 0, s>>>(I, out->rowptr.p, out->col.p, out->val.p, out->dst_frac.p, longest.p);
    MPG_HIP(hipGetLastError());
  }
  int32_t max_row = 0;
  MPG_HIP(hipMemcpyAsync(&max_row, longest.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipStreamSynchronize(s));
  out->max_row = max_row;
  return MPG_SUCCESS;
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_handle_mask() { return (const void *)&k_hm_flag; }
