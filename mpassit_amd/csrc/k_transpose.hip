// Transpose Regrid (ESMF_FieldRegridStore's transposeRoutehandle applied with ESMF_FieldRegrid): mesh_out = A^T grid_in.
//
// A is exactly what the forward Regrid applies: every stored entry idx >= 0 of a fixed-nnz handle (weight 1 for nearest),
// every CSR entry, and the pole caps of a periodic Grid -> Grid handle (destination pole_dst[q] adds pole_w[q] * mean of one
// CENTER row).  The transpose is the ADJOINT of that operator, not an inverse: A^T A != I.
//
// Transposed index (built on the first call of a handle, dropped with its tile lists whenever its indices are rewritten):
// a counting sort by source -- int32 histogram (integer atomics: the counts do not depend on arrival order), exclusive scan
// (mpg_scan_excl_i32), a fill whose positions inside a segment DO depend on arrival order, then every segment put into
// ascending (destination point, slot) order by ranking: one lane per segment of at most TR_SHORT entries, one wave per longer
// segment (each lane ranks entries against the whole segment, so the cost is quadratic in the segment length; C4 bilinear has
// 1.9 entries per cell on average).  The sources with more than TR_SHORT entries are listed (ascending) for the apply.
//
// Apply (gather form, no floating-point atomics): out[c][k] = sum over the segment of c, in ascending (point, slot) order,
// of fma(w_j, g[k][row_j], acc) from acc = 0, float64 arithmetic, one rounding at the store.  Three launches in stream order:
//   k_tr_short  one lane per source: the segment's (row, weight) pairs are loaded once into registers and reused for every
//               level.  Cell-fast: consecutive lanes store consecutive cells of a level.  Level-fast: a tile of 64 cells x up
//               to 64 levels is computed into LDS and leaves as whole [cell][lev] rows (the mirror of k_apply3_lf_rows).
//               Sources with a longer segment get a 0 placeholder here.
//   k_tr_long   one wave per listed source (nearest / conservative handles from a coarse mesh: hundreds of entries): lanes are
//               levels, each runs the same ascending sum.
//   k_tr_pole   pole caps: one workgroup per (field, level) reduces sum_q w_pole[q] * g[pole_dst[q]] for both rows in a fixed
//               order (strided partial sums, LDS tree, as k_pole_fix), then rewrites the sources of the two CENTER rows as
//               segment sum + term / row_len (the pole term added last).
// Every source's value is computed by the same expression in every kernel and layout, so the bits do not depend on the layout,
// on nfields, on the input type (float32 widens exactly) or on scheduling.
#include <algorithm>
#include <vector>

#include "apply_mesh.h"
#include "transpose_seg.h"   // TR_SHORT: the longest segment served by one lane (registers); longer ones go to k_tr_long

#define TR_LF_CELLS 64
#define TR_LF_LEVS 64

// ---- build ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tr_count_fixed(const int32_t *__restrict__ idx, int64_t ne, int64_t n_src, int32_t *__restrict__ cnt) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < ne; e += (int64_t)gridDim.x * blockDim.x) {
    const int32_t c = idx[e];
    if (c >= 0 && c < n_src) atomicAdd(&cnt[c], 1);
  }
}
__global__ __launch_bounds__(256) void k_tr_count_csr(const int32_t *__restrict__ col, int64_t ne, int64_t n_src, int32_t *__restrict__ cnt) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < ne; e += (int64_t)gridDim.x * blockDim.x) {
    const int32_t c = col[e];
    if (c >= 0 && c < n_src) atomicAdd(&cnt[c], 1);
  }
}

// st[0] sources with an entry, st[1] longest segment, st[2] sources listed in `lng` (more than TR_SHORT entries).  The two
// statistics are reduced across the wave first: one atomic per wave, not per source (3 M same-address atomics took 1 ms)
__global__ __launch_bounds__(256) void k_tr_classify(const int32_t *__restrict__ cnt, int64_t n_src, int32_t *__restrict__ st, int32_t *__restrict__ lng) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t end = (n_src + stride - 1) / stride * stride;   // every lane of a wave runs the same number of rounds (shuffles below)
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < end; c += stride) {
    const int32_t n = c < n_src ? cnt[c] : 0;
    int32_t nz = n > 0, mx = n;
    for (int o = 32; o > 0; o >>= 1) {
      nz += __shfl_xor(nz, o);
      mx = max(mx, __shfl_xor(mx, o));
    }
    if ((threadIdx.x & 63) == 0) {
      if (nz) atomicAdd(&st[0], nz);
      atomicMax(&st[1], mx);
    }
    if (n > TR_SHORT) lng[atomicAdd(&st[2], 1)] = (int32_t)c;
  }
}

// fixed-nnz handle: entry e = q * P + p has the sort key p * npr + q
__global__ __launch_bounds__(256) void k_tr_fill_fixed(const int32_t *__restrict__ idx, const double *__restrict__ w, int64_t P, int npr,
                                                       int64_t n_src, const int32_t *__restrict__ ptr, int32_t *__restrict__ cur,
                                                       int32_t *__restrict__ key, double *__restrict__ wt) {
  const int64_t ne = P * npr;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < ne; e += (int64_t)gridDim.x * blockDim.x) {
    const int32_t c = idx[e];
    if (c < 0 || c >= n_src) continue;
    const int64_t q = e / P, p = e - q * P;
    const int32_t pos = ptr[c] + atomicAdd(&cur[c], 1);
    key[pos] = (int32_t)(p * npr + q);
    wt[pos] = w ? w[e] : 1.0;
  }
}
// CSR handle: one thread per destination row; the entry number is the key (rows ascending, slots ascending inside a row)
__global__ __launch_bounds__(256) void k_tr_fill_csr(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const double *__restrict__ val,
                                                     int64_t P, int64_t n_src, const int32_t *__restrict__ ptr, int32_t *__restrict__ cur,
                                                     int32_t *__restrict__ key, double *__restrict__ wt) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < P; p += (int64_t)gridDim.x * blockDim.x) {
    for (int32_t e = rowptr[p]; e < rowptr[p + 1]; ++e) {
      const int32_t c = col[e];
      if (c < 0 || c >= n_src) continue;
      const int32_t pos = ptr[c] + atomicAdd(&cur[c], 1);
      key[pos] = e;
      wt[pos] = val[e];
    }
  }
}

// keys are unique: entry i goes to position b + #{j : key_j < key_i}.  Destination point of a key: key / div (div = npr for a
// fixed-nnz handle), or csr_row[key] (CSR: the row of entry `key`, looked up by binary search in rowptr)
__device__ __forceinline__ int32_t tr_key_point(int32_t key, int div, const int32_t *rowptr, int64_t P) {
  if (!rowptr) return key / div;
  int64_t lo = 0, hi = P;   // last p with rowptr[p] <= key
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (rowptr[mid] <= key) lo = mid;
    else hi = mid;
  }
  return (int32_t)lo;
}
__global__ __launch_bounds__(256) void k_tr_sort_short(const int32_t *__restrict__ ptr, int64_t n_src, const int32_t *__restrict__ key,
                                                       const double *__restrict__ wt, int div, const int32_t *__restrict__ rowptr, int64_t P,
                                                       int32_t *__restrict__ rows, double *__restrict__ w) {
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < n_src; c += (int64_t)gridDim.x * blockDim.x) {
    const int32_t b = ptr[c], n = ptr[c + 1] - b;
    if (n > TR_SHORT) continue;
    for (int32_t i = 0; i < n; ++i) {
      const int32_t ki = key[b + i];
      int32_t r = 0;
      for (int32_t j = 0; j < n; ++j) r += key[b + j] < ki;
      rows[b + r] = tr_key_point(ki, div, rowptr, P);
      w[b + r] = wt[b + i];
    }
  }
}
__global__ __launch_bounds__(256) void k_tr_sort_long(const int32_t *__restrict__ ptr, const int32_t *__restrict__ lng, int nlong,
                                                      const int32_t *__restrict__ key, const double *__restrict__ wt, int div,
                                                      const int32_t *__restrict__ rowptr, int64_t P, int32_t *__restrict__ rows,
                                                      double *__restrict__ w) {
  const int li = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (li >= nlong) return;
  const int32_t c = lng[li], b = ptr[c], n = ptr[c + 1] - b;
  for (int32_t i = lane; i < n; i += 64) {
    const int32_t ki = key[b + i];
    int32_t r = 0;
    for (int32_t j = 0; j < n; ++j) r += key[b + j] < ki;   // the same key for every lane: one broadcast load
    rows[b + r] = tr_key_point(ki, div, rowptr, P);
    w[b + r] = wt[b + i];
  }
}

static unsigned grid_for(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 8192)); }

int mpg_k_transpose_build(mpg_handle_s *h, hipStream_t s) {
  if (h->tr_built) return MPG_SUCCESS;
  h->free_transpose();   // what a failed earlier build left
  const int64_t n_src = h->n_src, P = h->n_dst;
  const bool csr = h->kind == MPG_KIND_CSR;
  const int64_t ne = csr ? h->nnz : (int64_t)h->nnz_per_row * P;
  if (ne >= INT32_MAX || n_src >= INT32_MAX) {
    mpg_set_error("mpg_regrid_transpose_dev: %lld entries / %lld sources do not fit the int32 transposed index", (long long)ne, (long long)n_src);
    return MPG_ERR_UNSUPPORTED;
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  MPG_HIP(hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) {
    (void)hipEventDestroy(e0);
    mpg_set_error("hipEventCreate failed in the transposed index build");
    return MPG_ERR_HIP;
  }
  struct Ev { hipEvent_t a, b; ~Ev() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } ev{e0, e1};
  MPG_HIP(hipEventRecord(e0, s));
  int rc;
  TmpBuf<int32_t> cnt, lng, st, key;
  TmpBuf<double> wt;
  if ((rc = cnt.alloc((size_t)n_src + 1, s)) || (rc = lng.alloc((size_t)n_src + 1, s)) || (rc = st.alloc(4, s))) return rc;
  if ((rc = h->tr_ptr.alloc((size_t)n_src + 1))) return rc;
  MPG_HIP(hipMemsetAsync(cnt.p, 0, sizeof(int32_t) * (n_src + 1), s));
  MPG_HIP(hipMemsetAsync(st.p, 0, sizeof(int32_t) * 4, s));
  if (ne > 0) {
    if (csr) k_tr_count_csr<<<grid_for(ne), 256, 0, s>>>(h->col.p, ne, n_src, cnt.p);
    else k_tr_count_fixed<<<grid_for(ne), 256, 0, s>>>(h->idx.p, ne, n_src, cnt.p);
  }
  if ((rc = mpg_scan_excl_i32(cnt.p, h->tr_ptr.p, n_src + 1, s))) return rc;
  if (n_src > 0) k_tr_classify<<<grid_for(n_src), 256, 0, s>>>(cnt.p, n_src, st.p, lng.p);
  MPG_HIP(hipGetLastError());
  int32_t hst[4] = {0, 0, 0, 0}, nnzt = 0;
  MPG_HIP(hipMemcpyAsync(hst, st.p, sizeof(hst), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipMemcpyAsync(&nnzt, h->tr_ptr.p + n_src, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipStreamSynchronize(s));
  const int nlong = hst[2];
  std::vector<int32_t> hl((size_t)nlong);
  if (nlong) {
    MPG_HIP(hipMemcpy(hl.data(), lng.p, sizeof(int32_t) * nlong, hipMemcpyDeviceToHost));
    std::sort(hl.begin(), hl.end());   // the atomic append's order is arbitrary; ascending ids keep neighbouring sources together
  }
  if ((rc = h->tr_row.alloc((size_t)nnzt + 1)) || (rc = h->tr_w.alloc((size_t)nnzt + 1)) || (rc = h->tr_long.alloc((size_t)nlong + 1))) return rc;
  if (nlong) MPG_HIP(hipMemcpyAsync(h->tr_long.p, hl.data(), sizeof(int32_t) * nlong, hipMemcpyHostToDevice, s));
  if (nnzt > 0) {
    if ((rc = key.alloc((size_t)nnzt, s)) || (rc = wt.alloc((size_t)nnzt, s))) return rc;
    MPG_HIP(hipMemsetAsync(cnt.p, 0, sizeof(int32_t) * (n_src + 1), s));   // now the fill's cursors
    if (csr) k_tr_fill_csr<<<grid_for(P), 256, 0, s>>>(h->rowptr.p, h->col.p, h->val.p, P, n_src, h->tr_ptr.p, cnt.p, key.p, wt.p);
    else k_tr_fill_fixed<<<grid_for(ne), 256, 0, s>>>(h->idx.p, h->w.p, P, h->nnz_per_row, n_src, h->tr_ptr.p, cnt.p, key.p, wt.p);
    const int div = csr ? 1 : h->nnz_per_row;
    const int32_t *rp = csr ? h->rowptr.p : nullptr;
    k_tr_sort_short<<<grid_for(n_src), 256, 0, s>>>(h->tr_ptr.p, n_src, key.p, wt.p, div, rp, P, h->tr_row.p, h->tr_w.p);
    if (nlong) k_tr_sort_long<<<(unsigned)((nlong + 3) / 4), 256, 0, s>>>(h->tr_ptr.p, h->tr_long.p, nlong, key.p, wt.p, div, rp, P, h->tr_row.p, h->tr_w.p);
    MPG_HIP(hipGetLastError());
  }
  MPG_HIP(hipEventRecord(e1, s));
  MPG_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  h->tr_nnz = nnzt;
  h->tr_nref = hst[0];
  h->tr_max = hst[1];
  h->tr_nlong = nlong;
  h->tr_build_ms = ms;
  h->tr_built = true;
  return MPG_SUCCESS;
}

// ---- apply ------------------------------------------------------------------------------------------------------------
// the segment sum itself -- tr_load_seg, tr_seg_regs, tr_seg_mem -- is transpose_seg.h: one text for this file and k_wind_transpose.hip
// cell-fast: out [f][lev][cell]; 256 consecutive sources per workgroup, every level
template <typename TS, typename TD>
__global__ __launch_bounds__(256) void k_tr_short_cf(const int32_t *__restrict__ ptr, const int32_t *__restrict__ rows, const double *__restrict__ wts,
                                                     const TS *__restrict__ src, TD *__restrict__ dst, int64_t n_src, int64_t ld, int nlev, int nblk) {
  const int blk = blockIdx.x % nblk, f = blockIdx.x / nblk;
  const int64_t c = (int64_t)blk * 256 + threadIdx.x;
  int32_t r[TR_SHORT];
  double w[TR_SHORT];
  const int n = tr_load_seg<TS>(ptr, rows, wts, c, c < n_src, r, w);
  const int nmax = tr_wave_max(n);
  if (c >= n_src) return;
  const TS *sf = src + (int64_t)f * nlev * ld;
  TD *df = dst + (int64_t)f * nlev * n_src + c;
#pragma unroll 2
  for (int k = 0; k < nlev; ++k) df[(int64_t)k * n_src] = (TD)tr_seg_regs<TS>(r, w, n, nmax, sf + (int64_t)k * ld);
}

// level-fast: out [f][cell][lev]; a tile of TR_LF_CELLS sources, levels in chunks of TR_LF_LEVS through LDS.  Wave v of the four
// computes levels k0 + v, k0 + v + 4, .. of its lane's source; the tile then leaves as consecutive [cell][lev] elements (one
// contiguous block when nlev <= TR_LF_LEVS)
template <typename TS, typename TD>
__global__ __launch_bounds__(256) void k_tr_short_lf(const int32_t *__restrict__ ptr, const int32_t *__restrict__ rows, const double *__restrict__ wts,
                                                     const TS *__restrict__ src, TD *__restrict__ dst, int64_t n_src, int64_t ld, int nlev, int ntile) {
  __shared__ TD tile[TR_LF_CELLS][TR_LF_LEVS + 1];
  const int t = blockIdx.x % ntile, f = blockIdx.x / ntile;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t c0 = (int64_t)t * TR_LF_CELLS, c = c0 + lane;
  const int ncell = (int)std::min<int64_t>(TR_LF_CELLS, n_src - c0);
  int32_t r[TR_SHORT];
  double w[TR_SHORT];
  const int n = tr_load_seg<TS>(ptr, rows, wts, c, c < n_src, r, w);
  const int nmax = tr_wave_max(n);
  const TS *sf = src + (int64_t)f * nlev * ld;
  TD *df = dst + ((int64_t)f * n_src + c0) * nlev;
  for (int k0 = 0; k0 < nlev; k0 += TR_LF_LEVS) {
    const int kc = std::min(TR_LF_LEVS, nlev - k0);
    for (int kk = wv; kk < kc; kk += 4) tile[lane][kk] = (TD)tr_seg_regs<TS>(r, w, n, nmax, sf + (int64_t)(k0 + kk) * ld);
    __syncthreads();
    const int tot = ncell * kc;
    for (int e = threadIdx.x; e < tot; e += 256) {
      const int cc = e / kc, kk = e - cc * kc;
      df[(int64_t)cc * nlev + k0 + kk] = tile[cc][kk];
    }
    __syncthreads();
  }
}

// one wave per listed (long) source, lanes = levels
template <typename TS, typename TD, bool LEVF>
__global__ __launch_bounds__(256) void k_tr_long(const int32_t *__restrict__ ptr, const int32_t *__restrict__ rows, const double *__restrict__ wts,
                                                 const int32_t *__restrict__ lng, int nlong, int ngrp, const TS *__restrict__ src, TD *__restrict__ dst,
                                                 int64_t n_src, int64_t ld, int nlev) {
  const int g = blockIdx.x % ngrp, f = blockIdx.x / ngrp;
  const int li = g * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (li >= nlong) return;
  const int64_t c = lng[li];
  const int32_t b = ptr[c], e = ptr[c + 1];
  const TS *sf = src + (int64_t)f * nlev * ld;
  TD *df = dst + (int64_t)f * nlev * n_src;
  for (int k = lane; k < nlev; k += 64) {
    const double v = tr_seg_mem<TS>(rows, wts, b, e, sf + (int64_t)k * ld);
    df[LEVF ? c * nlev + k : (int64_t)k * n_src + c] = (TD)v;
  }
}

// pole caps: one workgroup per (field, level)
template <typename TS, typename TD, bool LEVF>
__global__ __launch_bounds__(256) void k_tr_pole(const int32_t *__restrict__ ptr, const int32_t *__restrict__ rows, const double *__restrict__ wts,
                                                 const int32_t *__restrict__ pole_dst, const int32_t *__restrict__ pole_src0,
                                                 const double *__restrict__ pole_w, int n_pole, int row_len, const TS *__restrict__ src,
                                                 TD *__restrict__ dst, int64_t n_src, int64_t ld, int nlev) {
  __shared__ double red[2][256];
  const int k = blockIdx.x % nlev, f = blockIdx.x / nlev;
  const TS *sf = src + ((int64_t)f * nlev + k) * ld;
  TD *df = dst + (int64_t)f * nlev * n_src;
  double s0 = 0.0, s1 = 0.0;
  for (int q = threadIdx.x; q < n_pole; q += 256) {
    const double wp = pole_w[q];
    if (wp == 0.0) continue;
    const double v = wp * (double)sf[pole_dst[q]];
    if (pole_src0[q] == 0) s0 += v;
    else s1 += v;
  }
  red[0][threadIdx.x] = s0;
  red[1][threadIdx.x] = s1;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      red[0][threadIdx.x] += red[0][threadIdx.x + st];
      red[1][threadIdx.x] += red[1][threadIdx.x + st];
    }
    __syncthreads();
  }
  const double t0 = red[0][0] / (double)row_len, t1 = red[1][0] / (double)row_len;
  const int64_t row1 = n_src - row_len;
  const int64_t nrow = 2 * (int64_t)row_len >= n_src ? n_src : 2 * (int64_t)row_len;   // the two rows, or every source when they meet
  for (int64_t i = threadIdx.x; i < nrow; i += 256) {
    const int64_t c = nrow == n_src ? i : (i < row_len ? i : row1 + (i - row_len));
    double v = tr_seg_mem<TS>(rows, wts, ptr[c], ptr[c + 1], sf);
    if (c < row_len) v += t0;
    if (c >= row1) v += t1;
    df[LEVF ? c * nlev + k : (int64_t)k * n_src + c] = (TD)v;
  }
}

template <typename TS, typename TD>
static int launch_tr(mpg_handle_s *h, const void *src_v, int64_t ld, int nlev, int nfields, void *dst_v, bool levf, hipStream_t s) {
  const TS *src = (const TS *)src_v;
  TD *dst = (TD *)dst_v;
  const int64_t n_src = h->n_src;
  if (levf) {
    const int ntile = (int)((n_src + TR_LF_CELLS - 1) / TR_LF_CELLS);
    k_tr_short_lf<TS, TD><<<(unsigned)ntile * nfields, 256, 0, s>>>(h->tr_ptr.p, h->tr_row.p, h->tr_w.p, src, dst, n_src, ld, nlev, ntile);
  } else {
    const int nblk = (int)((n_src + 255) / 256);
    k_tr_short_cf<TS, TD><<<(unsigned)nblk * nfields, 256, 0, s>>>(h->tr_ptr.p, h->tr_row.p, h->tr_w.p, src, dst, n_src, ld, nlev, nblk);
  }
  if (h->tr_nlong) {
    const int ngrp = (h->tr_nlong + 3) / 4;
    auto fn = levf ? k_tr_long<TS, TD, true> : k_tr_long<TS, TD, false>;
    fn<<<(unsigned)ngrp * nfields, 256, 0, s>>>(h->tr_ptr.p, h->tr_row.p, h->tr_w.p, h->tr_long.p, h->tr_nlong, ngrp, src, dst, n_src, ld, nlev);
  }
  if (h->n_pole) {
    auto fn = levf ? k_tr_pole<TS, TD, true> : k_tr_pole<TS, TD, false>;
    fn<<<(unsigned)(nlev * nfields), 256, 0, s>>>(h->tr_ptr.p, h->tr_row.p, h->tr_w.p, h->pole_dst.p, h->pole_src0.p, h->pole_w.p, (int)h->n_pole,
                                                 h->pole_len, src, dst, n_src, ld, nlev);
  }
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

int mpg_k_transpose(mpg_handle_s *h, const void *src, int src_type, int64_t ld, int nlev, int nfields, void *dst, int dst_type, int layout,
                    hipStream_t s) {
  if (h->n_src == 0 || nlev == 0 || nfields == 0) return MPG_SUCCESS;
  const size_t esz = (dst_type & MPG_TYPE_F32) ? 4 : 8;
  if (h->n_dst == 0) return mpg_zero_planes(dst, esz, h->n_src, (int64_t)nlev * nfields, h->n_src, s);   // nothing maps: all sources 0
  if (h->n_pole && (h->kind != MPG_KIND_FIXED || h->pole_len <= 0 || h->pole_len > h->n_src)) {
    mpg_set_error("mpg_regrid_transpose_dev: pole terms on a handle that is not a Grid -> Grid bilinear one");
    return MPG_ERR_INVALID_ARG;
  }
  int rc = mpg_k_transpose_build(h, s);
  if (rc) return rc;
  if (ld == 0) ld = h->n_dst;
  const bool levf = layout == MPG_LAYOUT_LEV_FAST && nlev > 1;   // (a single level is the same memory in both layouts)
  return mpg_dispatch_types(src_type, dst_type, [&](auto ts, auto td) {   // (apply_mesh.h)
    return launch_tr<decltype(ts), decltype(td)>(h, src, ld, nlev, nfields, dst, levf, s);
  });
}

// The pole term alone, for a caller that has computed the segment sums itself (k_wind_transpose.hip): k_tr_pole rewrites the sources of
// the two CENTER rows of dst [nlev][n_src] float64 as segment sum + term / row_len -- the launch launch_tr ends with, the same bits.
// The handle's transposed index must be built.
int mpg_k_transpose_pole(mpg_handle_s *h, const void *src, int src_type, int64_t ld, int nlev, double *dst, hipStream_t s) {
  if (!h->n_pole || nlev == 0) return MPG_SUCCESS;
  if (h->kind != MPG_KIND_FIXED || h->pole_len <= 0 || h->pole_len > h->n_src || !h->tr_built) {
    mpg_set_error("mpg_k_transpose_pole: pole terms on a handle that is not a Grid -> Grid bilinear one with a transposed index");
    return MPG_ERR_INVALID_ARG;
  }
  if (src_type & MPG_TYPE_F32)
    k_tr_pole<float, double, false><<<(unsigned)nlev, 256, 0, s>>>(h->tr_ptr.p, h->tr_row.p, h->tr_w.p, h->pole_dst.p, h->pole_src0.p, h->pole_w.p,
                                                                  (int)h->n_pole, h->pole_len, (const float *)src, dst, h->n_src, ld, nlev);
  else
    k_tr_pole<double, double, false><<<(unsigned)nlev, 256, 0, s>>>(h->tr_ptr.p, h->tr_row.p, h->tr_w.p, h->pole_dst.p, h->pole_src0.p, h->pole_w.p,
                                                                   (int)h->n_pole, h->pole_len, (const double *)src, dst, h->n_src, ld, nlev);
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_transpose() { return (const void *)&k_tr_short_cf<double, double>; }
