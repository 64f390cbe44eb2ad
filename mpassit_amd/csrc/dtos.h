// Nearest destination to source (mpg_regrid_store_nearest_dtos, k_store_dtos.hip): the per-source search and the mean's value rule.
//
// The sources are the queries and the DESTINATION's tree is walked: dtos_nearest is knn_search (knn.h) with KBest<1>, so the answer is the
// smallest (d2, id) pair in lexicographic order -- a tie goes to the lower destination id, because the walk opens a box whose bound
// EQUALS the best distance.  dtos_nearest_masked walks the AliveTree of knn_mask.h: only unmasked destinations are candidates, and a
// dead root -- every destination masked -- is no search at all.  `bound(box)` is the caller's lower bound of a box, `items(node, f)` its
// leaf body (knn_src.h on the device).  The best pair stays in registers; the only scratch is the walk's stack.
// dtos_value: the value of every entry of a row of `len` entries.
// Plain C++ without HIP intrinsics, as knn.h: the kernels and tests/c/dtos_test.cpp compile this same text.
#pragma once
#include <stdint.h>

#include "knn.h"
#include "knn_mask.h"

#define DTOS_SUM 0    // MPG_DTOS_* of include/mpassit_amd.h
#define DTOS_MEAN 1

// -> the destination id, or -1 when the tree holds no item
template <class Tree, class Bound, class Items>
TW_FN int32_t dtos_nearest(const Tree &t, Bound bound, Items items, int *deepest = nullptr) {
  KBest<1> best;
  knn_search(t, bound, items, best, deepest);
  return best.n > 0 ? best.id[0] : -1;
}

// ... over the unmasked destinations alone; -1 when every destination is masked
template <class Tree, class Bound, class Items>
TW_FN int32_t dtos_nearest_masked(const Tree &t, const uint8_t *alive, Bound bound, Items items, int *deepest = nullptr) {
  KBest<1> best;
  knn_search_masked(t, alive, bound, items, best, deepest);
  return best.n > 0 ? best.id[0] : -1;
}

// MPG_DTOS_SUM: 1.0.  MPG_DTOS_MEAN: 1.0 / (double)len, one division rounded once (len >= 1: an entry belongs to a row that has it)
TW_FN double dtos_value(int norm, int32_t len) { return norm == DTOS_MEAN ? 1.0 / (double)len : 1.0; }
