// Mesh -> Mesh weight generation: ESMF_FieldRegridStore(srcField on a Mesh's elements, dstField on another Mesh's location).
//
// Sources are the cell centres of the source mesh (source index = cell id), destinations the cell centres or vertices of the
// destination mesh -- a plain list of points on the unit sphere, as in k_store_to_mesh.hip.
//   bilinear   source "cells" are the source mesh's dual (Delaunay) triangles, mpg_mesh_s::tri; a point belongs to the triangle with the
//              LOWEST id (= vertex id) for which the line type's weight function (geom.h tri_weights / tri_weights_normal, MPG_TOL)
//              passes; slots are the triangle's cells in tri's stored order, weights dA / S, dB / S, dC / S.  A point in no triangle is
//              unmapped: idx -1, weights 0.
//   nearest    the cell centre at the smallest chord distance, the lowest cell id on ties (k_store_nearest.hip: the exact search over the
//              source mesh's site BVH, one thread per point); every point is mapped.
// The Mesh -> Grid Store rasterises triangles into the grid's points with atomicMin; a point list has no such frame, so the bilinear
// Store here searches per point: a Morton-ordered BVH over the source mesh's triangles (built once per mesh, kept on it like `bvh`), leaf
// boxes = the hulls of the triangles' corners widened by everything a passing point can lie outside the hull, and one thread per
// point that walks every node whose box holds it and tests every triangle of every leaf it reaches.  The boxes are conservative -- they
// remove no triangle that would pass -- and the answer is the minimum id over ALL passing triangles, so it depends on the two meshes
// and the line type only: not on the order of the walk, not on how the tree was cut.
// How far outside the hull of A, B, C a passing point P can lie (d: the hull's diagonal, >= the longest side):
//   ray from the centre   P = Q / |Q| with Q = sum w_i V_i in the (tolerance-widened) planar triangle; |Q|^2 = 1 - sum_{i<j} w_i w_j
//                         |V_i - V_j|^2 >= 1 - d^2 / 3, so |P - Q| = 1 - |Q| <= d^2 / 3
//   along the normal      P = F + s n with the foot F in the triangle, 1 - |F|^2 = delta <= d^2 / 3 and the plane at distance h from the
//                         centre: s = sqrt(h^2 + delta) - h, which is <= d^2 / 2 for every triangle with h >= 1/3 and up to d / sqrt(3)
//                         for a sliver whose plane passes near the centre
//   tolerance             w_i >= -tol moves Q (or F) out of the triangle by <= 2 tol d
// pad = max(d^2 / 2, sqrt(h^2 + d^2 / 3) - h) + 2 tol d + 1e-9 covers both line types, so one tree serves either setting of the knob.
// No floating-point contraction in this translation unit (see k_store_conserve.hip).
#pragma clang fp contract(off)
#include <math.h>

#include "geom.h"
#include "mpg_internal.h"

#define MM_STACK 96   // 7 siblings pushed per level, <= MPG_BVH_MAXLEV levels (tree_walk.h: 77 entries at most)

// key of triangle t = Morton code of its corners' centroid; a triangle without three cells sorts behind every real one
static_assert(MM_STACK >= WalkCap<BvhTree>::FILTER, "the stack holds the walk's proven bound (tree_walk.h): its guard is never taken");
__global__ __launch_bounds__(256) void k_tri_morton(int64_t nV, const int32_t *__restrict__ tri, const double *__restrict__ cx,
                                                    const double *__restrict__ cy, const double *__restrict__ cz,
                                                    unsigned long long *__restrict__ key, int32_t *__restrict__ id) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= nV) return;
  const int32_t a = tri[t], b = tri[nV + t], c = tri[2 * nV + t];
  id[t] = (int32_t)t;
  if (a < 0 || b < 0 || c < 0) {
    key[t] = (1ull << 63) - 1;
    return;
  }
  const double third = 1.0 / 3.0;
  key[t] = morton63((cx[a] + cx[b] + cx[c]) * third, (cy[a] + cy[b] + cy[c]) * third, (cz[a] + cz[b] + cz[c]) * third);
}

__global__ __launch_bounds__(256) void k_tbvh_leaf(int64_t n, int64_t nleaf, const int32_t *__restrict__ sid, const int32_t *__restrict__ tri,
                                                   int64_t nV, const double *__restrict__ cx, const double *__restrict__ cy,
                                                   const double *__restrict__ cz, double tol, double *__restrict__ box) {
  const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (b >= nleaf) return;
  double lo[3] = {2, 2, 2}, hi[3] = {-2, -2, -2};
  const int64_t e = min(n, (b + 1) * MPG_BVH_LEAF);
  for (int64_t i = b * MPG_BVH_LEAF; i < e; ++i) {
    const int32_t t = sid[i];
    const int32_t ia = tri[t], ib = tri[nV + t], ic = tri[2 * nV + t];
    if (ia < 0 || ib < 0 || ic < 0) continue;
    const dv3 A = ld3(cx, cy, cz, ia), B = ld3(cx, cy, cz, ib), C = ld3(cx, cy, cz, ic);
    const double lx = fmin(A.x, fmin(B.x, C.x)), hx = fmax(A.x, fmax(B.x, C.x));
    const double ly = fmin(A.y, fmin(B.y, C.y)), hy = fmax(A.y, fmax(B.y, C.y));
    const double lz = fmin(A.z, fmin(B.z, C.z)), hz = fmax(A.z, fmax(B.z, C.z));
    const double d2 = (hx - lx) * (hx - lx) + (hy - ly) * (hy - ly) + (hz - lz) * (hz - lz);
    const dv3 nrm = cross3(B - A, C - A);
    const double nn = dot3(nrm, nrm);
    const double h = nn > 0.0 ? fabs(dot3(A, nrm)) / sqrt(nn) : 0.0;
    const double pad = fmax(0.5 * d2, sqrt(h * h + d2 * (1.0 / 3.0)) - h) + 2.0 * tol * sqrt(d2) + 1e-9;
    lo[0] = fmin(lo[0], lx - pad); hi[0] = fmax(hi[0], hx + pad);
    lo[1] = fmin(lo[1], ly - pad); hi[1] = fmax(hi[1], hy + pad);
    lo[2] = fmin(lo[2], lz - pad); hi[2] = fmax(hi[2], hz + pad);
  }
  double *o = box + 6 * b;
  o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = hi[0]; o[4] = hi[1]; o[5] = hi[2];
}

static int build_tri_bvh(mpg_mesh_s *m, hipStream_t s) {
  TriBvh &b = m->tbvh;
  if (b.built) return MPG_SUCCESS;
  const int64_t n = m->nVertices;
  const double *cx = m->cell.x.p, *cy = m->cell.y.p, *cz = m->cell.z.p;
  const int rc = mpg_bvh_build(
      b, n, "mpg_regrid_store_mesh",
      [&](unsigned long long *key, int32_t *id) {
        k_tri_morton<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(n, m->tri.p, cx, cy, cz, key, id);
        return MPG_SUCCESS;
      },
      [&]() {
        k_tbvh_leaf<<<(unsigned)((b.nnodes[0] + 255) / 256), 256, 0, s>>>(n, b.nnodes[0], b.sorted_id.p, m->tri.p, n, cx, cy, cz, MPG_TOL, b.box.p);
        return MPG_SUCCESS;
      },
      s);
  if (rc) b.free();
  return rc;
}

// One thread per destination point: depth-first over the nodes whose box holds the point (its own loop, not walk_filter of tree_walk.h: on the helper the
// Store was slower, profiles/r17_store_walks.md; the node to visit next in a register, only siblings on the stack), every valid triangle of every leaf reached is tested, the lowest passing id is kept.
template <bool NORMAL>
__global__ __launch_bounds__(256) void k_mesh_bilinear(int64_t n, const double *__restrict__ px, const double *__restrict__ py,
                                                       const double *__restrict__ pz, const int32_t *__restrict__ tri, int64_t nV,
                                                       const double *__restrict__ cx, const double *__restrict__ cy,
                                                       const double *__restrict__ cz, BvhView b, double tol, int32_t *__restrict__ idx,
                                                       double *__restrict__ w, int32_t *__restrict__ overflow) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p >= n) return;
  const dv3 P = dv3{px[p], py[p], pz[p]};
  int32_t id[3] = {-1, -1, -1};
  double ww[3] = {0, 0, 0};
  int32_t best = 0x7fffffff;
  auto holds = [&](int lev, int64_t node) -> bool {
    const double *bx = b.box + 6 * (b.off[lev] + node);
    return !(P.x < bx[0] || P.x > bx[3] || P.y < bx[1] || P.y > bx[4] || P.z < bx[2] || P.z > bx[5]);
  };
  int stack[MM_STACK];
  int sp = 0;
  const int top = b.nlev - 1;
  int cur = holds(top, 0) ? (top << 27) : -1;
  for (;;) {
    if (cur < 0) {
      if (sp == 0) break;
      cur = stack[--sp];
    }
    const int e = cur;
    cur = -1;
    const int lev = e >> 27;
    const int64_t node = e & ((1 << 27) - 1);
    if (lev == 0) {
      const int64_t i1 = min(b.n, (node + 1) * MPG_BVH_LEAF);
      for (int64_t i = node * MPG_BVH_LEAF; i < i1; ++i) {
        const int32_t t = b.sid[i];
        if (t >= best) continue;
        const int32_t ia = tri[t], ib = tri[nV + t], ic = tri[2 * nV + t];
        if (ia < 0 || ib < 0 || ic < 0) continue;
        const dv3 A = ld3(cx, cy, cz, ia), B = ld3(cx, cy, cz, ib), C = ld3(cx, cy, cz, ic);
        double tw[3];
        if (NORMAL ? tri_weights_normal(P, A, B, C, tol, tw) : tri_weights(P, A, B, C, tol, tw)) {
          best = t;
          id[0] = ia; id[1] = ib; id[2] = ic;
          ww[0] = tw[0]; ww[1] = tw[1]; ww[2] = tw[2];
        }
      }
      continue;
    }
    const int64_t c0 = node * MPG_BVH_FAN, c1 = min(b.nnodes[lev - 1], c0 + MPG_BVH_FAN);
    for (int64_t c = c0; c < c1; ++c) {
      if (!holds(lev - 1, c)) continue;
      const int enc = ((lev - 1) << 27) | (int)c;
      if (cur < 0) cur = enc;
      else if (sp < MM_STACK) stack[sp++] = enc;
      else atomicOr(overflow, 1);   // cannot happen (see MM_STACK); reported, never silently dropped
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    idx[k * n + p] = id[k];
    w[k * n + p] = ww[k];
  }
}

int mpg_k_store_mesh(mpg_mesh_s *src, mpg_mesh_s *dst, int dst_meshloc, int method, mpg_handle_s *h, hipStream_t s) {
  int rc;
  const PointSet &pts = dst_meshloc == MPG_MESHLOC_ELEMENT ? dst->cell : dst->vert;
  const int64_t n = dst_meshloc == MPG_MESHLOC_ELEMENT ? dst->nCells : dst->nVertices;
  const bool nearest = method == MPG_REGRIDMETHOD_NEAREST_STOD;
  h->kind = MPG_KIND_FIXED;
  h->nnz_per_row = nearest ? 1 : 3;
  h->n_src = src->nCells;
  h->n_dst = n;
  h->nx_dst = (int)n;
  h->ny_dst = 1;
  h->nnz = (int64_t)h->nnz_per_row * n;
  if ((rc = h->idx.alloc((size_t)h->nnz_per_row * (size_t)n))) return rc;
  if (!nearest && (rc = h->w.alloc(3 * (size_t)n))) return rc;
  // mpg_handle_store_stats: [2] points in all, [3] microseconds of GPU time this Store spent building the source mesh's triangle BVH
  // (0: the mesh had it already, or the method needs none)
  h->store_path = 0;
  h->store_stats[2] = n;
  if (nearest) {
    if ((rc = mpg_k_nearest_points(src, pts, n, h->idx.p, s))) return rc;
    MPG_HIP(hipStreamSynchronize(s));
    return MPG_SUCCESS;
  }
  const bool had = src->tbvh.built;
  if ((rc = build_tri_bvh(src, s))) return rc;
  if (!had) h->store_stats[3] = (int64_t)(src->tbvh.build_ms * 1e3f);
  BvhView v;
  mpg_bvh_view(src->tbvh, v);
  TmpBuf<int32_t> ovf;
  if ((rc = ovf.alloc(1, s))) return rc;
  MPG_HIP(hipMemsetAsync(ovf.p, 0, sizeof(int32_t), s));
  auto query = mpg_bilinear_linetype() ? k_mesh_bilinear<true> : k_mesh_bilinear<false>;
  query<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(n, pts.x.p, pts.y.p, pts.z.p, src->tri.p, src->nVertices, src->cell.x.p, src->cell.y.p,
                                                    src->cell.z.p, v, MPG_TOL, h->idx.p, h->w.p, ovf.p);
  MPG_HIP(hipGetLastError());
  int32_t h_ovf = 0;
  MPG_HIP(hipMemcpyAsync(&h_ovf, ovf.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipStreamSynchronize(s));
  if (h_ovf) {
    mpg_set_error("mpg_regrid_store_mesh: the traversal stack of the triangle search overflowed");
    return MPG_ERR_OVERFLOW;
  }
  return MPG_SUCCESS;
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_store_mesh() { return (const void *)k_mesh_bilinear<false>; }
