// The segment sum of the transposed index (mpg_handle_s::tr_ptr / tr_row / tr_w): ONE text for every kernel that applies a transpose --
// k_transpose.hip (mpg_regrid_transpose_dev) and k_wind_transpose.hip (mpg_wind_destagger_transpose_dev) -- so that a source's value is
// the same expression, and the same bits, wherever it is computed:
//   acc = fma(w_j, (double)g[row_j], acc) from +0.0 over the segment in stored (ascending (destination point, slot)) order.
// Only explicit fma() and selects: the sum does not depend on the including file's fp-contract setting.
#pragma once
#include "mpg_internal.h"

#define TR_SHORT 16   // k_transpose.hip: longest segment served by one lane (registers); longer ones are summed from memory (tr_seg_mem)

// N, the length of the register form, is the caller's (the arrays' size, at least 4): the sum is the same chain whatever holds the segment

// the 4-slot form in two steps, so that a kernel with several segments can issue every gather of a level ahead of the first fma
template <typename TS, int N>
__device__ __forceinline__ void tr_seg_gather4(const int32_t (&r)[N], const TS *__restrict__ sf, double (&v)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = (double)sf[r[j]];
}
template <int N>
__device__ __forceinline__ double tr_seg_sum4(const double (&w)[N], const double (&v)[4], int n) {
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) acc = j < n ? fma(w[j], v[j], acc) : acc;
  return acc;
}

// sum over one segment held in registers, ascending order; sf = the level's source plane.  nmax: the longest segment in the wave
// (uniform).  Slots past a lane's own n load a valid row (tr_load_seg fills them with row 0) and are dropped by a select, so the loads
// carry no branches and issue back to back; most handles (C4 bilinear: 4 at most) take the 4-slot form.
template <typename TS, int N>
__device__ __forceinline__ double tr_seg_regs(const int32_t (&r)[N], const double (&w)[N], int n, int nmax, const TS *__restrict__ sf) {
  if (nmax <= 4) {
    double v[4];
    tr_seg_gather4<TS, N>(r, sf, v);
    return tr_seg_sum4(w, v, n);
  }
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < N; ++j)
    if (j < nmax) {
      const double v = (double)sf[r[j]];
      acc = j < n ? fma(w[j], v, acc) : acc;
    }
  return acc;
}
// the same sum read from memory (any length)
template <typename TS>
__device__ __forceinline__ double tr_seg_mem(const int32_t *__restrict__ rows, const double *__restrict__ wts, int32_t b, int32_t e,
                                             const TS *__restrict__ sf) {
  double acc = 0.0;
  for (int32_t j = b; j < e; ++j) acc = fma(wts[j], (double)sf[rows[j]], acc);
  return acc;
}

// one lane per source: its segment into registers.  A segment longer than N is not loaded and counts 0 here (the caller serves it
// from memory: k_tr_long / k_tr_pole, or tr_seg_mem in the lane itself)
template <typename TS, int N>
__device__ __forceinline__ int tr_load_seg(const int32_t *__restrict__ ptr, const int32_t *__restrict__ rows, const double *__restrict__ wts,
                                           int64_t c, bool act, int32_t (&r)[N], double (&w)[N]) {
  int n = 0;
  int32_t b = 0;
  if (act) {
    b = ptr[c];
    n = ptr[c + 1] - b;
    if (n > N) n = 0;
  }
#pragma unroll
  for (int j = 0; j < N; ++j) {
    r[j] = 0;
    w[j] = 0.0;
    if (j < n) {
      r[j] = rows[b + j];
      w[j] = wts[b + j];
    }
  }
  return n;
}
__device__ __forceinline__ int tr_wave_max(int n) {
  for (int o = 32; o > 0; o >>= 1) n = max(n, __shfl_xor(n, o));
  return n;
}
