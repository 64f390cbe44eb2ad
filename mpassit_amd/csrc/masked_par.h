// The per-call parameters of the masked Regrid and its test for a missing value: ONE text for k_apply_masked.hip
// (mpg_regrid_masked_dev) and k_transpose_masked.hip (mpg_regrid_masked_transpose_dev), so that valid(q) is the same decision in
// the forward and in its adjoint.
#pragma once
#include "mpg_internal.h"

struct MaskPar {            // by value in the kernels' argument block
  const uint8_t *mask;      // [n_src] non-zero = never use, or nullptr
  double missing, frac, fill, scale, offset;
  int use_nan, use_val;
};

__device__ __forceinline__ bool mk_missing(double x, const MaskPar &m) {
  return (m.use_nan && __builtin_isnan(x)) || (m.use_val && x == m.missing);
}
