// The row rule of mpg_handle_mask's MPG_MASKRULE_ENTRY (include/mpassit_amd.h states it): masked source cells do not take part in a
// conservative row.  ONE function for the length pass (out_col == nullptr: nothing is written), the fill pass of k_handle_mask.hip and the
// host test (tests/c/knn_mask_test.cpp), every operation rounded on its own.  Plain C++ without HIP intrinsics, as knn.h.
#pragma once
#include <stdint.h>

#include "tree_walk.h"   // TW_FN

#define HM_NORM_DSTAREA 0    // MPG_NORM_DSTAREA / MPG_NORM_FRACAREA of include/mpassit_amd.h
#define HM_NORM_FRACAREA 1

// Row of `len` entries (col, val), src_mask over the columns (nullptr: nothing masked) -> the row's new length.
//   kept: the entries q with src_mask[col[q]] == 0, in stored order; Wk = ((0.0 + v_0) + v_1) + ... over the kept values, left to right.
//   nothing masked       the row verbatim, *frac_out = frac_in
//   kept == 0 or !(Wk > 0)   an empty row, *frac_out = +0.0   (a NaN sum maps nothing either)
//   MPG_NORM_DSTAREA     w' = w,      *frac_out = Wk
//   MPG_NORM_FRACAREA    w' = w / Wk, *frac_out = frac_in * Wk
// frac_in is read only where the rule names it; a handle without dst_frac passes 0.0 and drops *frac_out.
TW_FN int hm_entry_row(const int32_t *col, const double *val, int len, const uint8_t *src_mask, int norm_type, double frac_in,
                       int32_t *out_col, double *out_val, double *frac_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  int kept = 0;
  double Wk = 0.0;
  for (int q = 0; q < len; ++q)
    if (!src_mask || !src_mask[col[q]]) {
      Wk = Wk + val[q];
      ++kept;
    }
  if (kept == len) {
    if (out_col)
      for (int q = 0; q < len; ++q) {
        out_col[q] = col[q];
        out_val[q] = val[q];
      }
    *frac_out = frac_in;
    return len;
  }
  if (kept == 0 || !(Wk > 0.0)) {
    *frac_out = 0.0;
    return 0;
  }
  const bool fracarea = norm_type == HM_NORM_FRACAREA;
  if (out_col) {
    int at = 0;
    for (int q = 0; q < len; ++q)
      if (!src_mask[col[q]]) {
        out_col[at] = col[q];
        out_val[at] = fracarea ? val[q] / Wk : val[q];
        ++at;
      }
  }
  *frac_out = fracarea ? frac_in * Wk : Wk;
  return kept;
}
