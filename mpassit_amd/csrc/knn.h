// The K nearest items of a box tree, and the extrapolation weights made of their distances (mpg_handle_extrapolate, k_extrapolate.hip).
//
// KBest<K>: the K best (d2, id) pairs seen so far in ascending lexicographic order -- ties in d2 go to the lower id at every rank, the
// last included.  Insertion is one fully unrolled compare-and-shift chain: every index is a compile-time constant, so the list lives in
// registers (a runtime-indexed private array would go to scratch).  Empty places hold (INFINITY, INT32_MAX), which no real item follows.
// knn_search: walk_nearest (tree_walk.h) with `best` = the K-th d2 once the list is full and INFINITY before.  The walk opens a box whose
// bound EQUALS best -- a tie with a lower id may hide inside -- which is exactly what the K-th rank needs.  `items(node, f)` is the
// caller's leaf body: it calls f(d2, id) for every item of leaf `node` (8 sorted sites of a SiteBvhView, or a 4 x 4 block of points).
// knn_weights: the value rule of include/mpassit_amd.h, every operation rounded on its own.  The kernels and tests/c/knn_test.cpp compile
// this same text.  Plain C++ without HIP intrinsics, as tree_walk.h.
#pragma once
#include <math.h>
#include <stdint.h>

#include "tree_walk.h"

#define MPG_KNN_MAX 8   // MPG_EXTRAP_MAX_PNTS of include/mpassit_amd.h

template <int K>
struct KBest {
  double d2[K];
  int32_t id[K];
  int n;   // real entries, <= K
  TW_FN void clear() {
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int k = 0; k < K; ++k) {
      d2[k] = INFINITY;
      id[k] = 0x7fffffff;
    }
    n = 0;
  }
  TW_FN double bound() const { return d2[K - 1]; }   // INFINITY until the list is full
  TW_FN void insert(double d, int32_t i) {
    n += n < K;
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int k = 0; k < K; ++k) {   // the newcomer takes the first place it is below; what it displaces moves on down the chain
      const bool lt = d < d2[k] || (d == d2[k] && i < id[k]);
      const double td = d2[k];
      const int32_t ti = id[k];
      d2[k] = lt ? d : td;
      id[k] = lt ? i : ti;
      d = lt ? td : d;
      i = lt ? ti : i;
    }
  }
};

template <class Tree, int K, class Bound, class Items>
TW_FN void knn_search(const Tree &t, Bound bound, Items items, KBest<K> &list, int *deepest = nullptr) {
  list.clear();
  double best = INFINITY;
  walk_nearest(
      t, bound, best,
      [&](int node) {
        items(node, [&](double d, int32_t i) { list.insert(d, i); });
        best = list.bound();
        return false;
      },
      deepest);
}

// A CSR handle's rowptr is int32 and its last value is the entry count: 2^31 - 2 entries at most (mpg_handle_extrapolate's MPG_ERR_OVERFLOW)
TW_FN bool knn_nnz_fits(long long nnz) { return nnz >= 0 && nnz <= 0x7fffffffll - 1; }

// The weights of the k nearest (d2 ascending, k = the list's n) -> w[0 .. return value).  idavg == false (nearest source to destination) or
// a coincident nearest point (d2[0] == 0): ONE entry of weight 1.  Otherwise r_i = d2[0] / d2[i], t_i = r_i (e == 2) or pow(r_i, e / 2),
// S = ((t_0 + t_1) + ...) left to right, w_i = t_i / S: (1 / d^e) / sum(1 / d^e) with the nearest distance divided out, so that nothing
// overflows (t_i in [0, 1], t_0 == 1) and a far neighbour may underflow to weight 0.
template <int K>
TW_FN int knn_weights(const double (&d2)[K], int k, bool idavg, double e, double (&w)[K]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (k <= 0) return 0;
  if (!idavg || k == 1 || d2[0] == 0.0) {
    w[0] = 1.0;
    return 1;
  }
  const double he = 0.5 * e;
  double t[K];
  double S = 0.0;
#ifdef __HIPCC__
#pragma unroll
#endif
  for (int i = 0; i < K; ++i) {
    t[i] = 0.0;
    if (i < k) {
      const double r = d2[0] / d2[i];
      t[i] = e == 2.0 ? r : pow(r, he);
      S = i == 0 ? t[0] : S + t[i];
    }
  }
#ifdef __HIPCC__
#pragma unroll
#endif
  for (int i = 0; i < K; ++i)
    if (i < k) w[i] = t[i] / S;
  return k;
}
