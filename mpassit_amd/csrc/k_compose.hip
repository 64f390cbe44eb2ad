// Handle composition (mpg_handle_compose, mpg_compose_weights_dev): C = A . B of two route handles as ONE CSR handle, a device
// sparse-matrix x sparse-matrix product with a stated pattern and a stated summation order (include/mpassit_amd.h).  A Store-time family:
//
//   symbolic job  (pattern: rowptr, col)   per block of destination rows, planned on the host from the rows' 64-bit candidate counts
//                                          (compose_checks.h co_next_block: a fixed byte budget, every block's count within int32)
//     k_compose_expand<G, false>   candidates of every row: sum over A's entries p of the length of B's row col_A[p]           (once)
//     k_compose_expand<G, true>    the block's candidates as keys (local row << 32 | column of B), G lanes per row of A, a row's entries
//                                  G at a time with a scan of the reached rows' lengths: no row is too long, none sits in LDS
//     mpg_sort_pairs_u64_i32       the keys, device-wide (the row id leads, so rows stay together and columns ascend inside a row)
//     k_compose_heads              1 where a key differs from the one before; mpg_scan_excl_i32 of that numbers the distinct entries
//     k_compose_compact            the distinct columns, in order;  k_compose_rowptr: a row's first entry by a search of the sorted keys
//   The pattern is a set, so it cannot depend on the blocks; "compose_block_rows" (mpg_tune) forces small blocks for the tests.
//   mpg_k_compose_pattern is the same job for a caller with a bare CSR pattern as the inner operand and a value pass of its own
//   (k_conserve2nd.hip: the stencils of the source cells); mpg_k_compose is that job with k_compose_values behind it.
//
//   numeric job  (values)   k_compose_values<K, OWN>: one lane per entry (i, e) of C.  The lane finds its row by a search of C's rowptr,
//     walks A's row i in stored order and, inside each entry, B's row col_A[p] in stored order, and adds a_p * b_q where col_B[q] == e:
//     the summation order by construction, every product and sum rounded on its own (fp contract(off)), no atomics, the same bytes from
//     run to run.  OWN: b_q are B's own values (a fixed B's weights, or 1.0 of a nearest handle); otherwise K caller-owned planes
//     [K][nnz_B] -- mpg_compose_weights_dev, which launches this kernel and nothing else (no allocation, no host synchronisation).
//
// Operands are read through CoOp: CSR, or fixed slots [nz][n] whose idx -1 entries do not exist.  A column of A outside B's rows
// contributes nothing (memory-safe for any handles whose sizes chain).  No kernel here uses scratch or LDS beyond the scans' (profiles/r24_compose.md).
#include <vector>

#include "compose_checks.h"
#include "mpg_internal.h"

static int g_compose_block_rows = 0;   // "compose_block_rows" knob: 0 = blocks by the byte budget alone
void mpg_set_compose_block_rows(int v) { g_compose_block_rows = v; }

struct CoOp {
  const int32_t *rowptr;   // CSR row pointers; nullptr: fixed slots
  const int32_t *col;      // CSR columns, or idx [nz][n] (-1 = none)
  const double *val;       // CSR values, or w [nz][n]; nullptr: every value 1.0 (nearest)
  int nz;                  // slots of a fixed handle
  int64_t n;               // rows
};

static CoOp co_op(const mpg_handle_s *h) {
  CoOp o;
  if (h->kind == MPG_KIND_CSR) {
    o.rowptr = h->rowptr.p; o.col = h->col.p; o.val = h->val.p; o.nz = 0;
  } else {
    o.rowptr = nullptr; o.col = h->idx.p; o.val = h->w.p; o.nz = h->nnz_per_row;
  }
  o.n = h->n_dst;
  return o;
}

// row i: its first slot and its slots (a fixed row's slots may hold -1)
__device__ __forceinline__ void co_row(const CoOp &o, int64_t i, int64_t &b, int &len) {
  if (o.rowptr) {
    b = o.rowptr[i];
    len = o.rowptr[i + 1] - (int32_t)b;
  } else {
    b = i;
    len = o.nz;
  }
}
__device__ __forceinline__ int32_t co_col(const CoOp &o, int64_t b, int k) { return o.rowptr ? o.col[b + k] : o.col[(int64_t)k * o.n + b]; }
__device__ __forceinline__ double co_val(const CoOp &o, int64_t b, int k) {
  return !o.val ? 1.0 : o.rowptr ? o.val[b + k] : o.val[(int64_t)k * o.n + b];
}

// G lanes per row of A.  EXPAND false: cnt[g] = the row's candidates.  true: the candidates as keys from keys[off[g]] on, in A's then
// B's stored order (the sort that follows does not need that order, but it makes the kernel's output a function of its input alone)
template <int G, bool EXPAND>
__global__ __launch_bounds__(256) void k_compose_expand(CoOp A, CoOp B, int64_t r0, int64_t nrows, long long *__restrict__ cnt,
                                                        const int32_t *__restrict__ off, unsigned long long *__restrict__ keys) {
  const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
  const int lane = threadIdx.x % G;
  if (g >= nrows) return;   // (a group's lanes leave together)
  int64_t ab;
  int alen;
  co_row(A, r0 + g, ab, alen);
  long long run = 0;
  for (int p0 = 0; p0 < alen; p0 += G) {
    const int p = p0 + lane;
    int64_t bb = 0;
    int blen = 0, valid = 0;
    if (p < alen) {
      const int32_t ca = co_col(A, ab, p);
      if (ca >= 0 && (int64_t)ca < B.n) {
        co_row(B, ca, bb, blen);
        if (B.rowptr) {
          valid = blen;
        } else {
          for (int q = 0; q < blen; ++q) valid += co_col(B, bb, q) >= 0;
        }
      }
    }
    long long inc = valid;
    if (G > 1) {
      for (int o = 1; o < G; o <<= 1) {
        const long long t = __shfl_up(inc, o, G);
        if (lane >= o) inc += t;
      }
    }
    const long long total = G > 1 ? __shfl(inc, G - 1, G) : inc;
    if (EXPAND) {
      int64_t at = (int64_t)off[g] + run + inc - valid;
      const unsigned long long hi = (unsigned long long)(uint32_t)g << 32;
      for (int q = 0; q < blen; ++q) {
        const int32_t cb = co_col(B, bb, q);
        if (cb >= 0) keys[at++] = hi | (uint32_t)cb;
      }
    }
    run += total;
  }
  if (!EXPAND && lane == 0) cnt[g] = run;
}

__global__ __launch_bounds__(256) void k_compose_narrow(const long long *__restrict__ cnt, int64_t n, int32_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (int32_t)cnt[i];   // (the plan has checked that a block's sum, hence every count in it, fits)
}

__global__ __launch_bounds__(256) void k_compose_heads(const unsigned long long *__restrict__ keys, int64_t n, int32_t *__restrict__ flag) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < n) flag[k] = k == 0 || keys[k] != keys[k - 1];
}

__global__ __launch_bounds__(256) void k_compose_compact(const unsigned long long *__restrict__ keys, const int32_t *__restrict__ flag,
                                                         const int32_t *__restrict__ pos, int64_t n, int32_t *__restrict__ col) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < n && flag[k]) col[pos[k]] = (int32_t)(uint32_t)keys[k];
}

// rowptr[g] = base + the distinct entries of the block in front of local row g: pos of the first key of a row >= g (a head), or all nu
__global__ __launch_bounds__(256) void k_compose_rowptr(const unsigned long long *__restrict__ keys, const int32_t *__restrict__ pos, int64_t ncand,
                                                        int32_t nu, int64_t nrows, int32_t base, int32_t *__restrict__ rowptr) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= nrows) return;
  const unsigned long long want = (unsigned long long)g << 32;
  int64_t lo = 0, hi = ncand;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < want) lo = mid + 1;
    else hi = mid;
  }
  rowptr[g] = base + (lo < ncand ? pos[lo] : nu);
}

__global__ void k_compose_set(int32_t *end, int32_t nnz, int32_t *longest) {   // rowptr[n] and the maximum's start
  *end = nnz;
  *longest = 0;
}

__global__ __launch_bounds__(256) void k_compose_max_row(const int32_t *__restrict__ rowptr, int64_t n, int32_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int32_t v = i < n ? rowptr[i + 1] - rowptr[i] : 0;
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_down(v, o));
  if ((threadIdx.x & 63) == 0 && v > 0) atomicMax(out, v);   // (an integer maximum: the order does not matter)
}

// One lane per entry of C; bm: K planes ldb apart in B's CSR entry order (OWN: B's own values), m: K planes ldc apart in C's entry order
template <int K, bool OWN>
__global__ __launch_bounds__(256) void k_compose_values(CoOp A, CoOp B, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                        int64_t nrows, int64_t nnz, const double *__restrict__ bm, int64_t ldb,
                                                        double *__restrict__ m, int64_t ldc) {
#pragma clang fp contract(off)
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= nnz) return;
  int64_t lo = 0, hi = nrows;   // the first row whose end lies behind j
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)rowptr[mid + 1] <= j) lo = mid + 1;
    else hi = mid;
  }
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  if (lo < nrows) {
    const int32_t e = col[j];
    int64_t ab;
    int alen;
    co_row(A, lo, ab, alen);
    for (int p = 0; p < alen; ++p) {
      const int32_t ca = co_col(A, ab, p);
      if (ca < 0 || (int64_t)ca >= B.n) continue;
      const double a = co_val(A, ab, p);
      int64_t bb;
      int blen;
      co_row(B, ca, bb, blen);
      for (int q = 0; q < blen; ++q) {
        if (co_col(B, bb, q) != e) continue;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const double b = OWN ? co_val(B, bb, q) : bm[(int64_t)k * ldb + bb + q];
          const double t = a * b;
          acc[k] = acc[k] + t;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) m[(int64_t)k * ldc + j] = acc[k];
}

static inline unsigned co_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

template <bool EXPAND>
static void co_launch_expand(int G, const CoOp &A, const CoOp &B, int64_t r0, int64_t nrows, long long *cnt, const int32_t *off,
                             unsigned long long *keys, hipStream_t s) {
  const unsigned nb = co_grid(nrows * G);
  if (G == 4) k_compose_expand<4, EXPAND><<<nb, 256, 0, s>>>(A, B, r0, nrows, cnt, off, keys);
  else if (G == 16) k_compose_expand<16, EXPAND><<<nb, 256, 0, s>>>(A, B, r0, nrows, cnt, off, keys);
  else k_compose_expand<64, EXPAND><<<nb, 256, 0, s>>>(A, B, r0, nrows, cnt, off, keys);
}

// the values of `c` (the pattern of a . b): nplanes planes bm [nplanes][nnz_b] -> m [nplanes][nnz_c]; bm == nullptr: b's own values, one plane
int mpg_k_compose_values(mpg_handle_s *c, mpg_handle_s *a, mpg_handle_s *b, int nplanes, const double *bm, double *m, hipStream_t s) {
  if (c->nnz == 0) return MPG_SUCCESS;
  const CoOp A = co_op(a), B = co_op(b);
  const unsigned nb = co_grid(c->nnz);
  const int64_t n = c->n_dst, nnz = c->nnz, ldb = b->nnz, ldc = c->nnz;
  if (!bm) k_compose_values<1, true><<<nb, 256, 0, s>>>(A, B, c->rowptr.p, c->col.p, n, nnz, nullptr, 0, m, ldc);
  else if (nplanes == 1) k_compose_values<1, false><<<nb, 256, 0, s>>>(A, B, c->rowptr.p, c->col.p, n, nnz, bm, ldb, m, ldc);
  else if (nplanes == 2) k_compose_values<2, false><<<nb, 256, 0, s>>>(A, B, c->rowptr.p, c->col.p, n, nnz, bm, ldb, m, ldc);
  else if (nplanes == 3) k_compose_values<3, false><<<nb, 256, 0, s>>>(A, B, c->rowptr.p, c->col.p, n, nnz, bm, ldb, m, ldc);
  else k_compose_values<4, false><<<nb, 256, 0, s>>>(A, B, c->rowptr.p, c->col.p, n, nnz, bm, ldb, m, ldc);
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

namespace {
struct Chunk {
  DevBuf<int32_t> col;
  int64_t at = 0;   // its first entry in the composite
};
struct ChunkList {   // the blocks' distinct columns until the composite's size is known; freed on every way out
  std::vector<Chunk> v;
  ~ChunkList() {
    for (Chunk &c : v) c.col.free();
  }
};
}  // namespace

static int co_refused(int rc, const WvErr &e) {
  mpg_set_error("%s", e.msg);
  return rc;
}

// The symbolic job and what frames it: c (shape set by the caller, arrays empty) <- the pattern of A . B -- rowptr, col, nnz, max_row --
// with val allocated; `values` is called once the pattern stands and launches whatever fills c->val on stream s.  Blocking.
static int co_compose(const mpg_handle_s *a, const CoOp &A, const CoOp &B, mpg_handle_s *c, hipStream_t s, const std::function<int()> &values) {
  const int64_t n = a->n_dst;
  int rc;
  if ((rc = c->rowptr.alloc((size_t)n + 1))) return rc;
  // lanes per row of A: by its average row (a long row among short ones takes more turns of the same loop)
  const int64_t avg = a->kind == MPG_KIND_CSR ? (n > 0 ? a->nnz / n : 0) : a->nnz_per_row;
  const int G = avg <= 4 ? 4 : avg <= 16 ? 16 : 64;
  std::vector<int64_t> cnt_host((size_t)n);
  TmpBuf<long long> cnt;
  if ((rc = cnt.alloc((size_t)n, s))) return rc;
  if (n > 0) {
    co_launch_expand<false>(G, A, B, 0, n, cnt.p, nullptr, nullptr, s);
    MPG_HIP(hipGetLastError());
    MPG_HIP(hipMemcpyAsync(cnt_host.data(), cnt.p, sizeof(long long) * (size_t)n, hipMemcpyDeviceToHost, s));
    MPG_HIP(hipStreamSynchronize(s));
  }
  ChunkList chunks;
  WvErr e;
  int64_t nnz = 0;
  for (int64_t r0 = 0; r0 < n;) {
    int64_t r1, ncand;
    if ((rc = co_next_block(cnt_host.data(), n, r0, CO_BLOCK_CAND, g_compose_block_rows, &r1, &ncand, e))) return co_refused(rc, e);
    const int64_t nrows = r1 - r0;
    int32_t nu = 0;
    TmpBuf<unsigned long long> keys, sorted;
    TmpBuf<int32_t> off, flag, pos;
    if (ncand > 0) {
      if ((rc = keys.alloc((size_t)ncand, s)) || (rc = sorted.alloc((size_t)ncand, s)) || (rc = off.alloc((size_t)nrows, s)) ||
          (rc = flag.alloc((size_t)ncand, s)) || (rc = pos.alloc((size_t)ncand, s)))
        return rc;
      k_compose_narrow<<<co_grid(nrows), 256, 0, s>>>(cnt.p + r0, nrows, off.p);
      if ((rc = mpg_scan_excl_i32(off.p, off.p, nrows, s))) return rc;
      co_launch_expand<true>(G, A, B, r0, nrows, nullptr, off.p, keys.p, s);
      MPG_HIP(hipGetLastError());
      // (the sort carries a payload nobody reads: flag / pos are free until the heads are taken)
      if ((rc = mpg_sort_pairs_u64_i32(keys.p, sorted.p, flag.p, pos.p, ncand, s))) return rc;
      k_compose_heads<<<co_grid(ncand), 256, 0, s>>>(sorted.p, ncand, flag.p);
      if ((rc = mpg_scan_excl_i32(flag.p, pos.p, ncand, s))) return rc;
      int32_t last[2] = {0, 0};
      MPG_HIP(hipMemcpyAsync(&last[0], pos.p + (ncand - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
      MPG_HIP(hipMemcpyAsync(&last[1], flag.p + (ncand - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
      MPG_HIP(hipStreamSynchronize(s));
      nu = last[0] + last[1];
      if ((rc = co_check_nnz(nnz + nu, e))) return co_refused(rc, e);
      chunks.v.emplace_back();
      Chunk &ch = chunks.v.back();
      ch.at = nnz;
      if ((rc = ch.col.alloc((size_t)nu))) return rc;
      k_compose_compact<<<co_grid(ncand), 256, 0, s>>>(sorted.p, flag.p, pos.p, ncand, ch.col.p);
    }
    k_compose_rowptr<<<co_grid(nrows), 256, 0, s>>>(sorted.p, pos.p, ncand, nu, nrows, (int32_t)nnz, c->rowptr.p + r0);
    MPG_HIP(hipGetLastError());
    nnz += nu;
    r0 = r1;
  }
  TmpBuf<int32_t> longest;
  if ((rc = longest.alloc(1, s))) return rc;
  k_compose_set<<<1, 1, 0, s>>>(c->rowptr.p + n, (int32_t)nnz, longest.p);
  if ((rc = c->col.alloc((size_t)nnz + 1)) || (rc = c->val.alloc((size_t)nnz + 1))) return rc;
  for (Chunk &ch : chunks.v)
    if (ch.col.n) MPG_HIP(hipMemcpyAsync(c->col.p + ch.at, ch.col.p, sizeof(int32_t) * ch.col.n, hipMemcpyDeviceToDevice, s));
  c->nnz = nnz;
  if (n > 0) k_compose_max_row<<<co_grid(n), 256, 0, s>>>(c->rowptr.p, n, longest.p);
  MPG_HIP(hipGetLastError());
  if ((rc = values())) return rc;
  int32_t max_row = 0;
  MPG_HIP(hipMemcpyAsync(&max_row, longest.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipStreamSynchronize(s));   // (also: the chunks may go)
  c->max_row = max_row;
  return MPG_SUCCESS;
}

// c (shape set by the caller, arrays empty) <- the composite of a and b: rowptr, col, val, nnz, max_row.  Blocking.
int mpg_k_compose(mpg_handle_s *a, mpg_handle_s *b, mpg_handle_s *c, hipStream_t s) {
  return co_compose(a, co_op(a), co_op(b), c, s, [&]() { return mpg_k_compose_values(c, a, b, 1, nullptr, c->val.p, s); });
}

// the same with a bare CSR pattern of b_rows rows as the inner operand and the caller's own value pass (k_conserve2nd.hip)
int mpg_k_compose_pattern(mpg_handle_s *a, const int32_t *b_rowptr, const int32_t *b_col, int64_t b_rows, mpg_handle_s *c, hipStream_t s,
                          const std::function<int()> &values) {
  CoOp B;
  B.rowptr = b_rowptr; B.col = b_col; B.val = nullptr; B.nz = 0; B.n = b_rows;
  return co_compose(a, co_op(a), B, c, s, values);
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_compose() { return (const void *)&k_compose_values<1, true>; }
