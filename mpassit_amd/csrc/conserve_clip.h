// The pieces of the conservative Stores that more than one translation unit uses (k_store_conserve.hip: Mesh -> Grid and Grid -> Mesh;
// k_store_conserve_mesh.hip: Mesh -> Mesh): the polygon buffer of the clip in LDS, the in-place Sutherland-Hodgman step and the area of
// a mesh cell.  Every handle's bits depend on this arithmetic as it stands.  Include it AFTER `#pragma clang fp contract(off)`.
#pragma once
#include "geom.h"

#define CONS_MAXV 12   // max source polygon vertices handled (MPAS maxEdges is 6..10)
#define CLIP_NT 64
struct LdsPoly {   // vertex i of polygon buffer `buf` of this lane
  double *base;    // lds + lane
  int cb;
  __device__ __forceinline__ dv3 get(int buf, int i) const {
    const double *p = base + (size_t)((buf * cb + i) * 3) * CLIP_NT;
    return dv3{p[0], p[CLIP_NT], p[2 * CLIP_NT]};
  }
  __device__ __forceinline__ void set(int buf, int i, dv3 v) const {
    double *p = base + (size_t)((buf * cb + i) * 3) * CLIP_NT;
    p[0] = v.x;
    p[CLIP_NT] = v.y;
    p[2 * CLIP_NT] = v.z;
  }
};
// Sutherland-Hodgman step IN PLACE, the polygon in LDS.  The output of edge i goes to slots <= i + 1 and those have been
// read by then: vertex i+1 is in registers as X2, and a CONVEX polygon meets the plane at most twice with at least one
// vertex outside between the two crossings, so the write index never passes i + 1 (the first vertex, needed again for the
// closing edge, is kept in registers).  One buffer instead of two halves the LDS of the clip kernel: 8 instead of 4
// wavefronts per CU.  The arithmetic and its order are those of the two-buffer form: the same bits.  A non-convex cell can
// break the bound or outgrow `cap` = maxEdges + 4 slots; either is reported through *trunc (the Store then fails with
// MPG_ERR_OVERFLOW), never a silently wrong polygon.
__device__ __forceinline__ int clip_halfspace_lds(int n, const LdsPoly &L, dv3 nrm, int cap, int *trunc) {
  int m = 0;
  double eps = 1e-15 * sqrt(dot3(nrm, nrm));
  const dv3 first = L.get(0, 0);
  dv3 X1 = first;
  const double dfirst = dot3(nrm, first);
  double d1 = dfirst;
  for (int i = 0; i < n; ++i) {
    const dv3 X2 = (i + 1 == n) ? first : L.get(0, i + 1);
    const double d2 = (i + 1 == n) ? dfirst : dot3(nrm, X2);   // (the same product as the next edge's d1: computed once)
    bool in1 = d1 >= -eps, in2 = d2 >= -eps;
    if (in1) {
      if (m < cap && m <= i + 1) L.set(0, m++, X1);
      else *trunc = 1;
    }
    if (in1 != in2) {
      dv3 X = X1 * d2 - X2 * d1;
      double sgn = (d2 - d1) > 0.0 ? 1.0 : -1.0;
      double nn = sqrt(dot3(X, X));
      if (nn > 0.0) {
        if (m < cap && m <= i + 1) L.set(0, m++, X * (sgn / nn));
        else *trunc = 1;
      }
    }
    X1 = X2;
    d1 = d2;
  }
  return m;
}
// area(c): the fan of the cell's vertices in listed order, as the candidate pass forms it, its sign dropped
__device__ __forceinline__ double cell_fan_area(int64_t c, int maxEdges, const int32_t *__restrict__ voc, const double *__restrict__ vx,
                                                const double *__restrict__ vy, const double *__restrict__ vz) {
  dv3 first = dv3{0, 0, 0}, prev = first;
  int n = 0;
  double area = 0.0;
  for (int j = 0; j < maxEdges && n < CONS_MAXV; ++j) {
    const int32_t v = voc[c * maxEdges + j];
    if (v <= 0) continue;
    const dv3 x = dv3{vx[v - 1], vy[v - 1], vz[v - 1]};
    if (n == 0) first = x;
    else if (n >= 2) area += sph_tri_area(first, prev, x);
    prev = x;
    ++n;
  }
  return n < 3 ? 0.0 : fabs(area);
}
