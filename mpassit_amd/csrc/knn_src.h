// The two searched sets of the nearest searches (k_extrapolate.hip: the sources of mpg_handle_extrapolate; k_store_dtos.hip: the destinations
// of mpg_regrid_store_nearest_dtos): the tree, and the leaf body that hands every item of a leaf to f(d2, id) with the pinned distance
// arithmetic (dist2_nofma).  ExMeshSrc: a mesh's site BVH built whole, a leaf = MPG_BVH_LEAF sorted sites.  ExGridSrc: a stagger's point
// pyramid, a leaf = an MPG_PYR_B0 x MPG_PYR_B0 block of points.  leaf_masked / leaf_alive serve the masked walk of knn_mask.h.
#pragma once
#include "geom.h"
#include "mpg_internal.h"

struct ExMeshSrc {
  typedef BvhTree Tree;
  SiteBvhView b;
  __device__ __forceinline__ Tree tree() const { return BvhTree{b}; }
  template <class F>
  __device__ __forceinline__ void leaf(int node, double X, double Y, double Z, F f) const {
    const int64_t e1 = min(b.n, ((int64_t)node + 1) * MPG_BVH_LEAF);
    for (int64_t i = (int64_t)node * MPG_BVH_LEAF; i < e1; ++i) f(dist2_nofma(X, Y, Z, b.sx[i], b.sy[i], b.sz[i]), b.sid[i]);
  }
  // ... every UNMASKED item: the mask is read first, a masked item costs no distance
  template <class F>
  __device__ __forceinline__ void leaf_masked(int node, double X, double Y, double Z, const uint8_t *__restrict__ mask, F f) const {
    const int64_t e1 = min(b.n, ((int64_t)node + 1) * MPG_BVH_LEAF);
    for (int64_t i = (int64_t)node * MPG_BVH_LEAF; i < e1; ++i) {
      const int32_t c = b.sid[i];
      if (mask[c]) continue;
      f(dist2_nofma(X, Y, Z, b.sx[i], b.sy[i], b.sz[i]), c);
    }
  }
  __device__ __forceinline__ bool leaf_alive(int node, const uint8_t *__restrict__ mask) const {
    const int64_t e1 = min(b.n, ((int64_t)node + 1) * MPG_BVH_LEAF);
    bool a = false;
    for (int64_t i = (int64_t)node * MPG_BVH_LEAF; i < e1; ++i) a |= mask[b.sid[i]] == 0;
    return a;
  }
};
struct ExGridSrc {
  typedef PyrTree Tree;
  PyramidView pyr;
  int snx, sny;
  const double *sx, *sy, *sz;
  __device__ __forceinline__ Tree tree() const { return PyrTree{pyr}; }
  template <class F>
  __device__ __forceinline__ void leaf(int node, double X, double Y, double Z, F f) const {
    const int bi = node % pyr.nx[0], bj = node / pyr.nx[0];
    const int i1 = min(bi * MPG_PYR_B0 + MPG_PYR_B0, snx), j1 = min(bj * MPG_PYR_B0 + MPG_PYR_B0, sny);
    for (int j = bj * MPG_PYR_B0; j < j1; ++j)
      for (int i = bi * MPG_PYR_B0; i < i1; ++i) {
        const int c = j * snx + i;
        f(dist2_nofma(X, Y, Z, sx[c], sy[c], sz[c]), c);
      }
  }
  template <class F>
  __device__ __forceinline__ void leaf_masked(int node, double X, double Y, double Z, const uint8_t *__restrict__ mask, F f) const {
    const int bi = node % pyr.nx[0], bj = node / pyr.nx[0];
    const int i1 = min(bi * MPG_PYR_B0 + MPG_PYR_B0, snx), j1 = min(bj * MPG_PYR_B0 + MPG_PYR_B0, sny);
    for (int j = bj * MPG_PYR_B0; j < j1; ++j)
      for (int i = bi * MPG_PYR_B0; i < i1; ++i) {
        const int c = j * snx + i;
        if (mask[c]) continue;
        f(dist2_nofma(X, Y, Z, sx[c], sy[c], sz[c]), c);
      }
  }
  __device__ __forceinline__ bool leaf_alive(int node, const uint8_t *__restrict__ mask) const {
    const int bi = node % pyr.nx[0], bj = node / pyr.nx[0];
    const int i1 = min(bi * MPG_PYR_B0 + MPG_PYR_B0, snx), j1 = min(bj * MPG_PYR_B0 + MPG_PYR_B0, sny);
    bool a = false;
    for (int j = bj * MPG_PYR_B0; j < j1; ++j)
      for (int i = bi * MPG_PYR_B0; i < i1; ++i) a |= mask[j * snx + i] == 0;
    return a;
  }
};
