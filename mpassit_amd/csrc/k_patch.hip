// Patch regridding (mpg_handle_patch): a fixed bilinear handle of S = 3 or 4 slots turned into the CSR handle of second-degree patch
// recovery (include/mpassit_amd.h states the rule, patch.h is its arithmetic).  A Store-time family of three passes:
//
//   node pass   k_pt_node    one thread per source node: N1, on a mesh N2 when A fails, the attempt ladder (pt_attempt) -> one attempt byte
//                            per node.  The 21-double factor is NOT kept: the row passes recompute it per (row, slot) -- a node serves about
//                            two slots per row pass, and a per-node table of factor, frame and h (31 doubles) would be 0.8 GB on a 3 M-cell mesh.
//   count pass  k_pt_count   one thread per row: the patches of its slots under their nodes' attempts (pt_slot_ids) merged into the ascending
//                            distinct columns (pt_set_add) -> len[i]; the (row, slot) pairs per attempt, the rows written and the longest
//                            row are counted with integer atomics.  mpg_sum_i32_i64 -> the entry count, the call's one host round trip
//                            (the statistics travel with it) -> mpg_scan_excl_i32 -> rowptr.
//   fill pass   k_pt_fill    one thread per row: per slot pt_slot (frame, h, G, Cholesky, the two solves, L_k) and pt_row_add straight into
//                            the row's own col / val range, which the count pass sized: the candidate list of the merge lives in the output.
// A row is one lane's work: its slots share most of their patches, so lanes of a wave run the same instruction stream on neighbouring
// points and their gathers hit the same lines.  G / R and the solves sit in registers (compile-time indices throughout patch.h), and so do
// the two patch id lists of 32 ints (the compiler keeps them in VGPRs: no scratch in the node and fill passes); the count pass's 128
// candidate ids are runtime-indexed and live in scratch, 528 bytes a lane (profiles/r29_patch.md has the resource table).  No LDS.  No
// floating-point atomics: the same bytes from run to run.
#pragma clang fp contract(off)
#include "mpg_internal.h"
#include "patch.h"

struct PtIn {
  const int32_t *idx;   // [nz][n], -1 = none
  const double *w;      // [nz][n]
  int nz;               // 3 or 4
  int64_t n;            // rows
};

// stats_dev: [0] rows written, [1 .. 4] (row, slot) pairs served by A, B, C, D, [5] the longest row
enum { PT_ST_ROWS = 0, PT_ST_ATT = 1, PT_ST_LONGEST = 5, PT_ST_N = 6 };

static inline unsigned pt_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

__global__ __launch_bounds__(256) void k_pt_node(PtSrc src, int64_t n_src, uint8_t *__restrict__ att) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n_src) return;
  int32_t ids[PT_MAX_PNTS], tmp[PT_MAX_PNTS];
  att[c] = (uint8_t)pt_attempt(src, (int32_t)c, ids, tmp);
}

__device__ __forceinline__ int pt_wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

// len[i] for i < n, len[n] = 0 (so that the scan of n + 1 lengths ends in the entry count)
__global__ __launch_bounds__(256) void k_pt_count(PtIn in, PtSrc src, int64_t n_src, const uint8_t *__restrict__ att, int32_t *__restrict__ len,
                                                  unsigned long long *__restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int n = 0, na[4] = {0, 0, 0, 0};
  if (i < in.n && in.idx[i] >= 0) {
    int32_t list[PT_MAX_SLOTS * PT_MAX_PNTS], ids[PT_MAX_PNTS], tmp[PT_MAX_PNTS];
    for (int s = 0; s < in.nz; ++s) {
      const int32_t c = in.idx[(int64_t)s * in.n + i];
      if (c < 0 || c >= n_src) continue;
      const int a = att[c] & 3;
      const int m = pt_slot_ids(src, c, a, ids, tmp);
      for (int k = 0; k < m; ++k) (void)pt_set_add(list, n, PT_MAX_SLOTS * PT_MAX_PNTS, ids[k]);
      na[0] += a == PT_ATT_A;
      na[1] += a == PT_ATT_B;
      na[2] += a == PT_ATT_C;
      na[3] += a == PT_ATT_D;
    }
  }
  if (i <= in.n) len[i] = n;
  int longest = n;
  for (int o = 32; o > 0; o >>= 1) longest = max(longest, __shfl_down(longest, o));
  const int rows = pt_wave_sum(n > 0);
#pragma unroll
  for (int k = 0; k < 4; ++k) na[k] = pt_wave_sum(na[k]);
  if ((threadIdx.x & 63) == 0 && rows > 0) {   // (integer sums and an integer maximum: the order does not matter)
    atomicAdd(&stats[PT_ST_ROWS], (unsigned long long)rows);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (na[k]) atomicAdd(&stats[PT_ST_ATT + k], (unsigned long long)na[k]);
    atomicMax(&stats[PT_ST_LONGEST], (unsigned long long)longest);
  }
}

__global__ __launch_bounds__(256) void k_pt_fill(PtIn in, PtSrc src, int64_t n_src, const uint8_t *__restrict__ att,
                                                 const double *__restrict__ px, const double *__restrict__ py, const double *__restrict__ pz,
                                                 const int32_t *__restrict__ rowptr, int32_t *col, double *val) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= in.n) return;
  const int64_t at = rowptr[i];
  const int cap = rowptr[i + 1] - (int32_t)at;
  if (cap <= 0) return;
  const double P[3] = {px[i], py[i], pz[i]};
  int32_t ids[PT_MAX_PNTS], tmp[PT_MAX_PNTS];
  int n = 0;
  for (int s = 0; s < in.nz; ++s) {
    const int32_t c = in.idx[(int64_t)s * in.n + i];
    if (c < 0 || c >= n_src) continue;
    const double b = in.w[(int64_t)s * in.n + i];
    pt_slot(src, c, att[c] & 3, P, ids, tmp, [&](int32_t id, double L) { (void)pt_row_add(col + at, val + at, n, cap, id, b * L); });
  }
}

// in: a fixed bilinear handle of 3 or 4 slots with weights; src: its source points (patch.h); dst: its in->n_dst destination points.
// out: shape and method set by the caller, arrays empty.  Arguments checked by the API entry point; blocking.
int mpg_k_patch(mpg_handle_s *in, const PtSrc &src, const PointSet &dst, mpg_handle_s *out, hipStream_t s) {
  int rc;
  const int64_t n = in->n_dst, n_src = in->n_src;
  PtIn I;
  I.idx = in->idx.p; I.w = in->w.p; I.nz = in->nnz_per_row; I.n = n;
  out->kind = MPG_KIND_CSR;
  out->nnz_per_row = 0;
  TmpBuf<uint8_t> att;
  TmpBuf<int32_t> len;
  TmpBuf<unsigned long long> stats;
  TmpBuf<long long> total;
  if ((rc = att.alloc((size_t)n_src + 1, s)) || (rc = len.alloc((size_t)n + 1, s)) || (rc = stats.alloc(PT_ST_N, s)) || (rc = total.alloc(1, s)))
    return rc;
  if ((rc = out->rowptr.alloc((size_t)n + 1))) return rc;
  MPG_HIP(hipMemsetAsync(stats.p, 0, sizeof(unsigned long long) * PT_ST_N, s));
  if (n_src > 0) k_pt_node<<<pt_grid(n_src), 256, 0, s>>>(src, n_src, att.p);
  k_pt_count<<<pt_grid(n + 1), 256, 0, s>>>(I, src, n_src, att.p, len.p, stats.p);
  MPG_HIP(hipGetLastError());
  if ((rc = mpg_sum_i32_i64(len.p, n + 1, total.p, s))) return rc;
  long long nnz = 0;
  unsigned long long st[PT_ST_N];
  MPG_HIP(hipMemcpyAsync(&nnz, total.p, sizeof(long long), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipMemcpyAsync(st, stats.p, sizeof(st), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipStreamSynchronize(s));
  if (nnz > 0x7ffffffeLL) {
    mpg_set_error("mpg_handle_patch: the patch handle would have %lld entries, more than 2^31 - 2 (rowptr is int32): patch the parts of "
                  "the destination separately", nnz);
    return MPG_ERR_OVERFLOW;
  }
  if ((rc = mpg_scan_excl_i32(len.p, out->rowptr.p, n + 1, s))) return rc;
  if ((rc = out->col.alloc((size_t)nnz + 1)) || (rc = out->val.alloc((size_t)nnz + 1))) return rc;
  out->nnz = nnz;
  if (n > 0 && nnz > 0) {
    k_pt_fill<<<pt_grid(n), 256, 0, s>>>(I, src, n_src, att.p, dst.x.p, dst.y.p, dst.z.p, out->rowptr.p, out->col.p, out->val.p);
    MPG_HIP(hipGetLastError());
  }
  out->store_stats[1] = (int64_t)st[PT_ST_ROWS];
  for (int k = 0; k < 4; ++k) out->store_stats[2 + k] = (int64_t)st[PT_ST_ATT + k];
  out->store_stats[6] = (int64_t)st[PT_ST_LONGEST];
  out->max_row = (int64_t)st[PT_ST_LONGEST];
  MPG_HIP(hipStreamSynchronize(s));   // the temporaries may go
  return MPG_SUCCESS;
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_patch() { return (const void *)&k_pt_node; }
