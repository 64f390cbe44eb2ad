// Grid -> Mesh weight generation: ESMF_FieldRegridStore(srcField on a Grid stagger, dstField on a Mesh location).
//
// Sources are the snx x sny points of one stagger of a structured grid (source index j * snx + i), destinations the cell centres
// or vertices of an MPAS mesh -- a plain list of points on the unit sphere.
//   bilinear   source cells are the quads of four neighbouring stagger points A = (b, a), B = (b, a + 1), C = (b + 1, a + 1),
//              D = (b + 1, a); a mesh point belongs to the quad with the LOWEST id b * (snx - 1) + a for which quad_solve succeeds and
//              xi, eta lie in [-tol, 1 + tol]; slots and weights are those of k_grid_bilinear (k_store_gridbil.hip): A, B, C, D with
//              (1 - xi)(1 - eta), xi (1 - eta), xi eta, (1 - xi) eta.  A point in no quad is unmapped: idx -1, weights 0.
//   nearest    the stagger point at the smallest chord distance (dist2_nofma), the lowest source index on ties; every point is mapped.
// Candidates come by one of two routes that test the same quads with the same code, so their handles are identical bit for bit:
//   index space  on a grid with a usable inverse projection (mpg_grid_has_inverse) the point's own (i, j) names the quads around
//                floor(i), floor(j), within the pad of the other Stores' index boxes (geom.h mpg_box_pad, a figure one unit across);
//                where the inverse hands out NaN the point takes the second route
//   pyramid      one thread per mesh point descends an AABB pyramid over the stagger's quads (k_setup.hip: leaves of 4 x 4 quads
//                bounded by their corner points, boxes widened by the quads' bulge) and tests every leaf quad whose own box
//                holds the point
// A quad is tested only when its box -- the hull of its corners widened by its bulge and the inside tolerance -- holds the point;
// the box is conservative, so it removes no quad that would pass.
// No floating-point contraction in this translation unit (see k_store_conserve.hip).
#pragma clang fp contract(off)
#include <math.h>

#include "geom.h"
#include "mpg_internal.h"
#include "quad_solve.h"

#define TM_STACK 64   // of k_to_mesh_bilinear's own walk; its guard is never taken:
static_assert(TM_STACK >= WalkCap<PyrTree>::FILTER, "the stack holds the walk's proven bound (tree_walk.h)");

// quad (a, b) of the stagger: inside -> its four source ids and weights
__device__ __forceinline__ bool tm_try_quad(dv3 P, int a, int b, int snx, const double *__restrict__ sx, const double *__restrict__ sy,
                                            const double *__restrict__ sz, double tol, int32_t *id, double *ww) {
  const int64_t iA = (int64_t)b * snx + a, iB = iA + 1, iC = iB + snx, iD = iA + snx;
  if (!quad_try(P, ld3(sx, sy, sz, iA), ld3(sx, sy, sz, iB), ld3(sx, sy, sz, iC), ld3(sx, sy, sz, iD), tol, ww)) return false;   // (quad_solve.h)
  id[0] = (int32_t)iA; id[1] = (int32_t)iB; id[2] = (int32_t)iC; id[3] = (int32_t)iD;
  return true;
}

// ij: the points' (i, j) in the grid's 0-based CENTER index space (mpg_k_points_ij) or nullptr; di, dj: offset of the stagger's point
// indices.  pyr: pyramid over the (snx - 1) x (sny - 1) quads.  cnt[0] += points that had an index space and still took the pyramid.
__global__ __launch_bounds__(256) void k_to_mesh_bilinear(int64_t n, const double *__restrict__ px, const double *__restrict__ py,
                                                          const double *__restrict__ pz, int snx, int sny, const double *__restrict__ sx,
                                                          const double *__restrict__ sy, const double *__restrict__ sz,
                                                          const float *__restrict__ ij, float di, float dj, float pad_coef, float pad_latlon,
                                                          PyramidView pyr, double tol, int32_t *__restrict__ idx, double *__restrict__ w,
                                                          unsigned long long *__restrict__ cnt) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p >= n) return;
  const dv3 P = dv3{px[p], py[p], pz[p]};
  const int qnx = snx - 1, qny = sny - 1;
  int32_t id[4] = {-1, -1, -1, -1};
  double ww[4] = {0, 0, 0, 0};
  bool placed = false;
  if (ij) {
    const float fi = ij[2 * p] + di, fj = ij[2 * p + 1] + dj;
    if (fi == fi && fj == fj) {
      placed = true;
      const float pad = mpg_box_pad(1.f, pad_coef, pad_latlon, fabs(P.z));
      const float lim_i = (float)snx + 2.f, lim_j = (float)sny + 2.f;
      const int a0 = max((int)floorf(fminf(fmaxf(fi - pad, -2.f), lim_i)), 0), a1 = min((int)floorf(fminf(fmaxf(fi + pad, -2.f), lim_i)), qnx - 1);
      const int b0 = max((int)floorf(fminf(fmaxf(fj - pad, -2.f), lim_j)), 0), b1 = min((int)floorf(fminf(fmaxf(fj + pad, -2.f), lim_j)), qny - 1);
      bool found = false;
      for (int b = b0; b <= b1 && !found; ++b)          // ascending quad id: the first that passes is the lowest
        for (int a = a0; a <= a1 && !found; ++a) found = tm_try_quad(P, a, b, snx, sx, sy, sz, tol, id, ww);
    } else {
      atomicAdd(cnt, 1ull);
    }
  }
  if (!placed) {
    // depth-first walk over the nodes whose box holds the point: its own loop, child by child, not walk_filter of tree_walk.h (on the
    // helper this Store was 2-4 % slower, profiles/r17_store_walks.md); the node to visit next in a register, only siblings on the
    // stack; the margin covers a point within tol outside a quad the node's pad was not built for
    const double mg = 2.0 * tol;
    auto holds = [&](int lev, int node) -> bool {
      const double *bx = pyr.box + 6 * (pyr.off[lev] + node);
      return !(P.x < bx[0] - mg || P.x > bx[3] + mg || P.y < bx[1] - mg || P.y > bx[4] + mg || P.z < bx[2] - mg || P.z > bx[5] + mg);
    };
    int stack[TM_STACK];
    int sp = 0;
    const int top = pyr.nlev - 1;
    int cur = holds(top, 0) ? (top << 26) : -1;
    int best = 0x7fffffff;
    for (;;) {
      if (cur < 0) {
        if (sp == 0) break;
        cur = stack[--sp];
      }
      const int e = cur;
      cur = -1;
      const int lev = e >> 26, node = e & ((1 << 26) - 1);
      const int bi = node % pyr.nx[lev], bj = node / pyr.nx[lev];
      if (lev == 0) {
        const int a1 = min(bi * MPG_PYR_B0 + MPG_PYR_B0, qnx), b1 = min(bj * MPG_PYR_B0 + MPG_PYR_B0, qny);
        for (int b = bj * MPG_PYR_B0; b < b1; ++b)
          for (int a = bi * MPG_PYR_B0; a < a1; ++a) {
            const int q = b * qnx + a;
            if (q >= best) continue;
            int32_t tid[4];
            double tw[4];
            if (tm_try_quad(P, a, b, snx, sx, sy, sz, tol, tid, tw)) {
              best = q;
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                id[k] = tid[k];
                ww[k] = tw[k];
              }
            }
          }
        continue;
      }
      const int cnx = pyr.nx[lev - 1], cny = pyr.ny[lev - 1];
      for (int dj2 = 0; dj2 < 2; ++dj2)
        for (int di2 = 0; di2 < 2; ++di2) {
          const int ci = 2 * bi + di2, cj = 2 * bj + dj2;
          if (ci >= cnx || cj >= cny) continue;
          const int child = cj * cnx + ci;
          if (!holds(lev - 1, child)) continue;
          const int enc = ((lev - 1) << 26) | child;
          if (cur < 0) cur = enc;
          else if (sp < TM_STACK) stack[sp++] = enc;
        }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    idx[k * n + p] = id[k];
    w[k * n + p] = ww[k];
  }
}

// Nearest stagger point: exact branch and bound over the POINT pyramid (leaves of 4 x 4 points), seeded with the point the inverse
// projection names where there is one (any seed gives the same answer: it only tightens the bound the walk starts with).  Distances
// and box bounds without FMA in a fixed order (geom.h), ties to the lowest source index.
__global__ __launch_bounds__(256) void k_to_mesh_nearest(int64_t n, const double *__restrict__ px, const double *__restrict__ py,
                                                         const double *__restrict__ pz, int snx, int sny, const double *__restrict__ sx,
                                                         const double *__restrict__ sy, const double *__restrict__ sz,
                                                         const float *__restrict__ ij, float di, float dj, PyramidView pyr,
                                                         int32_t *__restrict__ idx) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p >= n) return;
  const double X = px[p], Y = py[p], Z = pz[p];
  double best_d = INFINITY;
  int best = 0x7fffffff;
  if (ij) {
    const float fi = ij[2 * p] + di, fj = ij[2 * p + 1] + dj;
    if (fi == fi && fj == fj) {
      const int si = (int)fminf(fmaxf(rintf(fi), 0.f), (float)(snx - 1)), sj = (int)fminf(fmaxf(rintf(fj), 0.f), (float)(sny - 1));
      best = sj * snx + si;
      best_d = dist2_nofma(X, Y, Z, sx[best], sy[best], sz[best]);
    }
  }
  walk_nearest(
      PyrTree{pyr}, [&](const double *bx) { return boxdist2_nofma(X, Y, Z, bx); }, best_d, [&](int node) {
        const int bi = node % pyr.nx[0], bj = node / pyr.nx[0];
        const int i1 = min(bi * MPG_PYR_B0 + MPG_PYR_B0, snx), j1 = min(bj * MPG_PYR_B0 + MPG_PYR_B0, sny);
        for (int j = bj * MPG_PYR_B0; j < j1; ++j)
          for (int i = bi * MPG_PYR_B0; i < i1; ++i) {
            const int c = j * snx + i;
            const double d = dist2_nofma(X, Y, Z, sx[c], sy[c], sz[c]);
            if (d < best_d || (d == best_d && c < best)) {
              best_d = d;
              best = c;
            }
          }
        return false;
      });
  idx[p] = best;
}

// The Store onto any list of points: `dst` holds n = nx_dst * ny_dst of them (a mesh location: ny_dst = 1; a stagger of another grid: its
// snx x sny).  `who` names the entry point in the messages.
int mpg_k_store_to_points(mpg_grid_s *g, int stagger, const PointSet &dst, int64_t n, int nx_dst, int ny_dst, int method, const char *who,
                          mpg_handle_s *h, hipStream_t s) {
  int rc;
  const PointSet &src = g->pts[stagger];
  const int snx = g->snx[stagger], sny = g->sny[stagger];
  const bool nearest = method == MPG_REGRIDMETHOD_NEAREST_STOD;
  if (!nearest && (snx < 2 || sny < 2)) {
    mpg_set_error("%s: a bilinear Store needs at least 2 x 2 points of stagger %d", who, stagger);
    return MPG_ERR_INVALID_ARG;
  }
  h->kind = MPG_KIND_FIXED;
  h->nnz_per_row = nearest ? 1 : 4;
  h->n_src = (int64_t)snx * sny;
  h->n_dst = n;
  h->nx_dst = nx_dst;
  h->ny_dst = ny_dst;
  h->nnz = (int64_t)h->nnz_per_row * n;
  if ((rc = h->idx.alloc((size_t)h->nnz_per_row * (size_t)n))) return rc;
  if (!nearest && (rc = h->w.alloc(4 * (size_t)n))) return rc;
  if (n == 0) return MPG_SUCCESS;
  // the search structure: the stagger's quads (bilinear) or its points (nearest)
  Pyramid &pyr = nearest ? g->pyr[stagger] : g->quadpyr[stagger];
  if (!pyr.built) {
    rc = nearest ? mpg_k_build_pyramid(src, snx, sny, pyr, s) : mpg_k_build_cell_pyramid(src, snx - 1, sny - 1, pyr, s);
    if (rc) return rc;
  }
  if ((rc = mpg_walk_check<PyrTree>((int64_t)pyr.nx[0] * pyr.ny[0], who))) return rc;
  // index space: bilinear quads only where the Stores' boxes are valid; the nearest seed is good wherever the inverse answers
  TmpBuf<float> ij;
  const bool use_ij = mpg_grid_has_inverse(g, stagger) && mpg_store_boxes();
  if (use_ij) {
    if ((rc = ij.alloc(2 * (size_t)n, s))) return rc;
    if ((rc = mpg_k_points_ij(g, n, dst.x.p, dst.y.p, dst.z.p, ij.p, s, MPG_LATLON_BOX_LIMIT, !(g->periodic & MPG_GRID_PERIODIC_I)))) return rc;
  }
  const float di = (stagger == MPG_STAGGERLOC_EDGE1 || stagger == MPG_STAGGERLOC_CORNER) ? 0.5f : 0.f;
  const float dj = (stagger == MPG_STAGGERLOC_EDGE2 || stagger == MPG_STAGGERLOC_CORNER) ? 0.5f : 0.f;
  TmpBuf<unsigned long long> cnt;
  if ((rc = cnt.alloc(1, s))) return rc;
  MPG_HIP(hipMemsetAsync(cnt.p, 0, sizeof(unsigned long long), s));
  const unsigned nb = (unsigned)((n + 255) / 256);
  if (nearest) {
    k_to_mesh_nearest<<<nb, 256, 0, s>>>(n, dst.x.p, dst.y.p, dst.z.p, snx, sny, src.x.p, src.y.p, src.z.p, use_ij ? ij.p : nullptr, di, dj,
                                         mpg_pyr_view(pyr), h->idx.p);
  } else {
    const double tol = mpg_grid_inside_tol_exp() == 10 ? MPG_TOL : pow(10.0, -(double)mpg_grid_inside_tol_exp());
    k_to_mesh_bilinear<<<nb, 256, 0, s>>>(n, dst.x.p, dst.y.p, dst.z.p, snx, sny, src.x.p, src.y.p, src.z.p, use_ij ? ij.p : nullptr, di, dj,
                                          (float)mpg_grid_box_pad_coef(g), (float)mpg_grid_box_pad_latlon(g), mpg_pyr_view(pyr), tol, h->idx.p,
                                          h->w.p, cnt.p);
  }
  MPG_HIP(hipGetLastError());
  unsigned long long fell = 0;
  MPG_HIP(hipMemcpyAsync(&fell, cnt.p, sizeof(fell), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipStreamSynchronize(s));
  // mpg_handle_store_stats: [1] points whose index was unusable and that took the pyramid walk instead, [2] points in all
  h->store_path = use_ij ? 1 : 0;
  h->store_stats[1] = (int64_t)fell;
  h->store_stats[2] = n;
  return MPG_SUCCESS;
}

int mpg_k_store_to_mesh(mpg_grid_s *g, int stagger, mpg_mesh_s *m, int meshloc, int method, mpg_handle_s *h, hipStream_t s) {
  // the destination points: cells, vertices or (mpg_mesh_set_edges) edges -- nothing else differs between the three
  const PointSet &dst = meshloc == MPG_MESHLOC_EDGE ? m->edge : meshloc == MPG_MESHLOC_ELEMENT ? m->cell : m->vert;
  const int64_t n = meshloc == MPG_MESHLOC_EDGE ? m->edge.n : meshloc == MPG_MESHLOC_ELEMENT ? m->nCells : m->nVertices;
  return mpg_k_store_to_points(g, stagger, dst, n, (int)n, 1, method, "mpg_regrid_store_to_mesh", h, s);
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_store_to_mesh() { return (const void *)k_to_mesh_bilinear; }
