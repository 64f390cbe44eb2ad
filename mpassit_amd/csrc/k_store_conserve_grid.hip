// Conservative Grid -> Grid weight generation: ESMF_FieldRegridStore(regridmethod=CONSERVE, normType=) with the cells of one Grid as the
// source and the cells of another as the destination (mpg_regrid_store_conserve_grid_to_grid).
//
// Polygons on both sides are the grids' cells: cell (i, j), index j * nx + i, is the quadrilateral of CORNER points (i, j), (i + 1, j),
// (i + 1, j + 1), (i, j + 1) with great-circle sides.  I(d, s) is the Mesh -> Mesh Store's (k_store_conserve_mesh.hip) with "cell polygon" read
// as this quadrilateral: the source cell is the subject polygon, made counter-clockwise by the sign of its own fan area (the listed order
// reversed when that is negative); it is clipped by the sides of the destination cell, made counter-clockwise the same way, in their
// order; clip planes have normals in difference form a x (b - a); a side with |b - a|^2 < 1e-24 bounds nothing (the collapsed pole side of
// a lat-lon grid's end row); the area is the sph_tri_area fan from slot 0, clamped at 0.  The clip step and its inside rule are
// conserve_clip.h's, unchanged.  A cell whose fan area is exactly 0 is part of no pair.  Rows are keyed by destination cell and built by
// count -> scan -> ordered insert from each cell's own run of pairs: no atomic decides a stored byte.
//
// Candidates.  The rule: no pair with I > 0 is removed.  One thread per destination cell walks the SOURCE grid's cell pyramid (k_setup.hip:
// leaves of 4 x 4 cells, the hull of their CORNER points padded by half the squared box diagonal + 1e-9) with the destination cell's own box:
// the coordinate hull of its four corners padded by 2 e2 + 1e-9, e2 = max_i |v_i - v_0|^2.  Why nothing is lost: a point of a spherical
// polygon is p = q / |q| with q a convex combination of the vertices, so q lies in the vertices' coordinate hull and |p - q| <= D^2 / 2
// with D the largest chord between two vertices (the proof heads k_store_conserve_mesh.hip).  D <= 2 sqrt(e2), so the destination cell --
// sides AND interior -- lies in its box.  A source cell's vertices lie in its leaf's hull and its D^2 is at most that hull's squared
// diagonal, so the cell lies in the leaf's box, hence in every ancestor's; and it lies in its own box, formed in the leaf as the
// destination's is.  Two cells that share a point therefore pass every test on the way down, and every pair that passes is clipped.
// A count pass, a scan and a fill pass give the pair list grouped by destination cell at exact size: no fixed list length, no spill path.
// The pyramid walk is the only candidate route: store_path is 0.
// One lane per (destination, source) pair clips: the subject polygon in LDS, [vertex][component][lane], CG_SLOTS vertex slots -- a convex
// quadrilateral cut by four planes has at most 4 + 4 vertices --, the destination quadrilateral in registers.
// Shared sides.  Between a parent grid and its nest, or a grid and itself, whole sides of the two cells lie on one great circle, and the
// subject's vertices on that circle fall on either side of the plane by the rounding of one product: the polygon meets the plane four
// times (in, out, in, in, out), which no convex polygon does.  The in-place step of conserve_clip.h then wants to write past the vertex it
// reads next and reports truncation; with it the Store would refuse every such pair of grids.  A pair whose in-place clip reports that is
// clipped again from its stored corners by cg_clip_halfspace_top below: the same arithmetic in the same order -- the bits of the
// two-buffer form, as the in-place step's are wherever it succeeds --, with the polygon moved to the TOP slots first, so that the output,
// which grows from slot 0, has cap - n slots of room before it reaches a vertex not yet read.  Only a polygon that outgrows CG_SLOTS on
// that path too is an error (MPG_ERR_OVERFLOW), never a silently wrong polygon.
// No floating-point contraction in this translation unit (see k_store_conserve.hip).
#pragma clang fp contract(off)
#include <math.h>

#include <algorithm>

#include "geom.h"
#include "mpg_internal.h"
#include "conserve_clip.h"

#define CG_SLOTS 12

struct GridCells {   // the cells of a grid: nx x ny of them over (nx + 1) x (ny + 1) CORNER points
  int nx, ny;
  const double *x, *y, *z;
};

// corners of cell c in listed order
__device__ __forceinline__ void cg_quad(const GridCells &g, int64_t c, dv3 *q) {
  const int i = (int)(c % g.nx), j = (int)(c / g.nx), nxc = g.nx + 1;
  const int64_t k = (int64_t)j * nxc + i;
  q[0] = dv3{g.x[k], g.y[k], g.z[k]};
  q[1] = dv3{g.x[k + 1], g.y[k + 1], g.z[k + 1]};
  q[2] = dv3{g.x[k + nxc + 1], g.y[k + nxc + 1], g.z[k + nxc + 1]};
  q[3] = dv3{g.x[k + nxc], g.y[k + nxc], g.z[k + nxc]};
}

// the padded coordinate hull of a quadrilateral (see the head of this file)
__device__ __forceinline__ void cg_box(const dv3 *q, double *lo, double *hi) {
  lo[0] = hi[0] = q[0].x;
  lo[1] = hi[1] = q[0].y;
  lo[2] = hi[2] = q[0].z;
  double e2 = 0.0;
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    lo[0] = fmin(lo[0], q[k].x); hi[0] = fmax(hi[0], q[k].x);
    lo[1] = fmin(lo[1], q[k].y); hi[1] = fmax(hi[1], q[k].y);
    lo[2] = fmin(lo[2], q[k].z); hi[2] = fmax(hi[2], q[k].z);
    const dv3 d = q[k] - q[0];
    e2 = fmax(e2, dot3(d, d));
  }
  const double pad = 2.0 * e2 + 1e-9;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] -= pad;
    hi[k] += pad;
  }
}

// clip_halfspace_lds of conserve_clip.h, its arithmetic and order unchanged, for a polygon that is not quite convex (see the head of
// this file): the n vertices are moved to slots cap - n .. cap - 1 (back to front: the ranges may overlap), read from there and written
// from slot 0.  Vertex i + 1 is in registers when the output of edge i is written, so a write at slot m is safe while m <= i + 1 + shift.
__device__ __forceinline__ int cg_clip_halfspace_top(int n, const LdsPoly &L, dv3 nrm, int cap, int *trunc) {
  const int shift = cap - n;
  for (int i = n - 1; i >= 0; --i) L.set(0, i + shift, L.get(0, i));
  int m = 0;
  double eps = 1e-15 * sqrt(dot3(nrm, nrm));
  const dv3 first = L.get(0, shift);
  dv3 X1 = first;
  const double dfirst = dot3(nrm, first);
  double d1 = dfirst;
  for (int i = 0; i < n; ++i) {
    const dv3 X2 = (i + 1 == n) ? first : L.get(0, shift + i + 1);
    const double d2 = (i + 1 == n) ? dfirst : dot3(nrm, X2);
    bool in1 = d1 >= -eps, in2 = d2 >= -eps;
    if (in1) {
      if (m < cap && m <= i + 1 + shift) L.set(0, m++, X1);
      else *trunc = 1;
    }
    if (in1 != in2) {
      dv3 X = X1 * d2 - X2 * d1;
      double sgn = (d2 - d1) > 0.0 ? 1.0 : -1.0;
      double nn = sqrt(dot3(X, X));
      if (nn > 0.0) {
        if (m < cap && m <= i + 1 + shift) L.set(0, m++, X * (sgn / nn));
        else *trunc = 1;
      }
    }
    X1 = X2;
    d1 = d2;
  }
  return m;
}

// the subject quadrilateral vs (counter-clockwise, already in slots 0 .. 3 of L) clipped by the sides of the counter-clockwise quadrilateral
// q in their order -> the number of vertices left.  The sides are taken by shifting the register array (constant indices only: an array
// indexed by the side would live in scratch memory).  TOP: cg_clip_halfspace_top instead of the in-place step.
template <bool TOP>
__device__ __forceinline__ int cg_clip_quad(const LdsPoly &L, dv3 q0, dv3 q1, dv3 q2, dv3 q3, int *trunc) {
  int n = 4;
  const dv3 qfirst = q0;
  for (int e = 0; e < 4 && n >= 3; ++e) {
    const dv3 qa = q0, qb = e == 3 ? qfirst : q1;
    q0 = q1;
    q1 = q2;
    q2 = q3;
    const dv3 side = qb - qa;
    if (dot3(side, side) < 1e-24) continue;   // collapsed side: bounds nothing
    n = TOP ? (n <= CG_SLOTS ? cg_clip_halfspace_top(n, L, cross3(qa, side), CG_SLOTS, trunc) : 0)
            : clip_halfspace_lds(n, L, cross3(qa, side), CG_SLOTS, trunc);
  }
  return n;
}

// orientation and area of every cell, once per Store and grid: 0 the listed order is counter-clockwise seen from outside, 1 it is
// clockwise (the clip reverses it), 2 a fan area of exactly 0: never part of a pair.  area = the fan's, its sign dropped.
__global__ __launch_bounds__(256) void k_cg_orient(GridCells g, uint8_t *__restrict__ orient, double *__restrict__ area) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= (int64_t)g.nx * g.ny) return;
  dv3 q[4];
  cg_quad(g, c, q);
  double a = 0.0;
  a += sph_tri_area(q[0], q[1], q[2]);
  a += sph_tri_area(q[0], q[2], q[3]);
  orient[c] = a == 0.0 ? 2 : (a < 0.0 ? 1 : 0);
  area[c] = fabs(a);
}

// One thread per destination cell: the walk of tree_walk.h over the nodes of the source grid's cell pyramid whose box meets the cell's;
// every source cell of every leaf reached whose own box meets it is a candidate.  FILL = false counts them (cnt[d]; the scan's extra
// element cnt[nD] = 0), FILL = true writes them at poff[d] .. in the same order.
template <bool FILL>
__global__ __launch_bounds__(256) void k_cg_candidates(GridCells gd, GridCells gs, const uint8_t *__restrict__ orient_d,
                                                       const uint8_t *__restrict__ orient_s, PyramidView pyr, int32_t *__restrict__ cnt,
                                                       const int32_t *__restrict__ poff, int32_t *__restrict__ pair_s) {
  const int64_t nD = (int64_t)gd.nx * gd.ny;
  const int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (d > nD) return;
  if (d == nD) {
    if (!FILL) cnt[d] = 0;
    return;
  }
  int found = 0;
  if (orient_d[d] != 2) {
    dv3 q[4];
    double lo[3], hi[3];
    cg_quad(gd, d, q);
    cg_box(q, lo, hi);
    const int32_t o = FILL ? poff[d] : 0, oe = FILL ? poff[d + 1] : 0;
    const PyrTree tree{pyr};
    walk_filter(
        tree, walk_enc<PyrTree>(tree.top(), 0), true,
        [&](const double *bx) -> bool {
          return !(bx[0] > hi[0] || bx[3] < lo[0] || bx[1] > hi[1] || bx[4] < lo[1] || bx[2] > hi[2] || bx[5] < lo[2]);
        },
        [&](int node) -> bool {
          const int bi = node % pyr.nx[0], bj = node / pyr.nx[0];
          const int a1 = min(bi * MPG_PYR_B0 + MPG_PYR_B0, gs.nx), b1 = min(bj * MPG_PYR_B0 + MPG_PYR_B0, gs.ny);
          for (int b = bj * MPG_PYR_B0; b < b1; ++b)
            for (int a = bi * MPG_PYR_B0; a < a1; ++a) {
              const int64_t sc = (int64_t)b * gs.nx + a;
              dv3 r[4];
              double slo[3], shi[3];
              cg_quad(gs, sc, r);
              cg_box(r, slo, shi);
              if (slo[0] > hi[0] || shi[0] < lo[0] || slo[1] > hi[1] || shi[1] < lo[1] || slo[2] > hi[2] || shi[2] < lo[2]) continue;
              if (orient_s[sc] == 2) continue;
              if (FILL && o + found < oe) pair_s[o + found] = (int32_t)sc;   // (the count pass walked the same tree: always true)
              ++found;
            }
          return false;
        });
  }
  if (!FILL) cnt[d] = found;
}

// pair t belongs to the destination cell d with poff[d] <= t < poff[d + 1]: one thread per cell writes its run
__global__ __launch_bounds__(256) void k_cg_pair_dst(int64_t nD, const int32_t *__restrict__ poff, int32_t *__restrict__ pair_d) {
  const int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (d >= nD) return;
  for (int t = poff[d]; t < poff[d + 1]; ++t) pair_d[t] = (int32_t)d;
}

// One lane per pair: I(d, s) -> pair_val.  The destination quadrilateral is held in registers in counter-clockwise order.  A pair whose
// in-place clip reports truncation (shared sides: see the head of this file) is clipped again from its corners on the roomier path.
__global__ __launch_bounds__(CLIP_NT) void k_cg_clip_pairs(int64_t npairs, const int32_t *__restrict__ pair_d, const int32_t *__restrict__ pair_s,
                                                           GridCells gd, GridCells gs, const uint8_t *__restrict__ orient_d,
                                                           const uint8_t *__restrict__ orient_s, double *__restrict__ pair_val,
                                                           int32_t *__restrict__ truncated) {
  __shared__ double cg_clip_lds[CG_SLOTS * 3 * CLIP_NT];   // [CG_SLOTS][3][CLIP_NT]
  const int64_t t = blockIdx.x * (int64_t)CLIP_NT + threadIdx.x;
  if (t >= npairs) return;
  const LdsPoly L{cg_clip_lds + threadIdx.x, CG_SLOTS};
  const int64_t d = pair_d[t], c = pair_s[t];
  dv3 vs[4], vd[4];
  cg_quad(gs, c, vs);
  cg_quad(gd, d, vd);
  const bool rev_s = orient_s[c] == 1, rev_d = orient_d[d] == 1;
#pragma unroll
  for (int k = 0; k < 4; ++k) L.set(0, k, rev_s ? vs[3 - k] : vs[k]);
  dv3 q[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = rev_d ? vd[3 - k] : vd[k];
  int trunc = 0;
  int n = cg_clip_quad<false>(L, q[0], q[1], q[2], q[3], &trunc);
  if (trunc) {
    trunc = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) L.set(0, k, rev_s ? vs[3 - k] : vs[k]);
    n = cg_clip_quad<true>(L, q[0], q[1], q[2], q[3], &trunc);
  }
  double ar = 0.0;
  if (n >= 3) {
    double sa = 0.0;
    const dv3 v0 = L.get(0, 0);
    for (int k = 1; k + 1 < n; ++k) sa += sph_tri_area(v0, L.get(0, k), L.get(0, k + 1));
    ar = sa > 0.0 ? sa : 0.0;
  }
  pair_val[t] = ar;
  if (trunc) atomicOr(truncated, 1);   // (a flag for the error path, not a stored byte)
}

// Rows keyed by destination cell, one thread per cell from its own run of pairs: count the entries above the sliver threshold, scan, then
// insert them in ascending source index; frac = the sum in that order / area(d).
__global__ __launch_bounds__(256) void k_cg_row_count(int64_t nD, const double *__restrict__ area_d, const int32_t *__restrict__ poff,
                                                      const double *__restrict__ pair_val, int32_t *__restrict__ cnt) {
  const int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (d > nD) return;
  int n = 0;
  if (d < nD) {
    const double a = area_d[d];
    if (a > 0.0)
      for (int t = poff[d]; t < poff[d + 1]; ++t) n += pair_val[t] > 1e-14 * a;
  }
  cnt[d] = n;   // (the scan's extra element: 0)
}
__global__ __launch_bounds__(256) void k_cg_rows(int64_t nD, const double *__restrict__ area_d, const int32_t *__restrict__ poff,
                                                 const int32_t *__restrict__ pair_s, const double *__restrict__ pair_val,
                                                 const int32_t *__restrict__ rowptr, int norm_type, int32_t *__restrict__ col,
                                                 double *__restrict__ val, double *__restrict__ frac) {
  const int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (d >= nD) return;
  const double a = area_d[d];
  const int b = rowptr[d], e = rowptr[d + 1];
  if (e == b) {
    frac[d] = 0.0;
    return;
  }
  int n = 0;
  for (int t = poff[d]; t < poff[d + 1]; ++t) {
    const double I = pair_val[t];
    if (!(I > 1e-14 * a)) continue;
    const int32_t g = pair_s[t];
    int j = b + n - 1;
    while (j >= b && col[j] > g) {
      col[j + 1] = col[j];
      val[j + 1] = val[j];
      --j;
    }
    col[j + 1] = g;
    val[j + 1] = I;
    ++n;
  }
  double sum = 0.0;
  for (int q = b; q < e; ++q) sum += val[q];   // ascending source index
  frac[d] = sum / a;
  const double div = norm_type == MPG_NORM_FRACAREA ? sum : a;
  for (int q = b; q < e; ++q) val[q] = val[q] / div;
}

int mpg_k_store_conserve_grid(mpg_grid_s *src, mpg_grid_s *dst, int norm_type, mpg_handle_s *h, hipStream_t s) {
  static const char *who = "mpg_regrid_store_conserve_grid_to_grid";
  int rc;
  const PointSet &cs = src->pts[MPG_STAGGERLOC_CORNER], &cd = dst->pts[MPG_STAGGERLOC_CORNER];
  for (const mpg_grid_s *g : {src, dst})
    if (g->nx < 1 || g->ny < 1 || g->pts[MPG_STAGGERLOC_CORNER].n != (int64_t)(g->nx + 1) * (g->ny + 1)) {
      mpg_set_error("%s: a conservative Store needs CORNER-stagger coordinates on the %s grid (its cells are the quadrilaterals of four "
                    "CORNER points): create the grid with them",
                    who, g == src ? "source" : "destination");
      return MPG_ERR_INVALID_ARG;
    }
  const GridCells gs{src->nx, src->ny, cs.x.p, cs.y.p, cs.z.p}, gd{dst->nx, dst->ny, cd.x.p, cd.y.p, cd.z.p};
  const int64_t nS = (int64_t)src->nx * src->ny, nD = (int64_t)dst->nx * dst->ny;
  if (!src->cellpyr.built && (rc = mpg_k_build_cell_pyramid(cs, src->nx, src->ny, src->cellpyr, s))) return rc;
  if ((rc = mpg_walk_check<PyrTree>((int64_t)src->cellpyr.nx[0] * src->cellpyr.ny[0], who))) return rc;
  h->kind = MPG_KIND_CSR;
  h->nnz_per_row = 0;
  h->n_src = nS;
  h->n_dst = nD;
  h->nx_dst = dst->nx;
  h->ny_dst = dst->ny;
  h->store_path = 0;
  if ((rc = h->rowptr.alloc((size_t)nD + 1)) || (rc = h->dst_frac.alloc((size_t)nD))) return rc;
  // (1) orientation and area of both grids' cells
  TmpBuf<uint8_t> orient_s, orient_d;
  TmpBuf<double> area_s, area_d;
  if ((rc = orient_s.alloc((size_t)nS, s)) || (rc = area_s.alloc((size_t)nS, s))) return rc;
  k_cg_orient<<<(unsigned)((nS + 255) / 256), 256, 0, s>>>(gs, orient_s.p, area_s.p);
  const uint8_t *od = orient_s.p;
  const double *ad = area_s.p;
  if (dst != src) {
    if ((rc = orient_d.alloc((size_t)nD, s)) || (rc = area_d.alloc((size_t)nD, s))) return rc;
    k_cg_orient<<<(unsigned)((nD + 255) / 256), 256, 0, s>>>(gd, orient_d.p, area_d.p);
    od = orient_d.p;
    ad = area_d.p;
  }
  MPG_HIP(hipGetLastError());
  // (2) candidates: count, scan, fill -- the pair list grouped by destination cell
  TmpBuf<int32_t> cnt, poff, pair_d, pair_s, truncated;
  TmpBuf<double> pair_val;
  if ((rc = cnt.alloc((size_t)nD + 1, s)) || (rc = poff.alloc((size_t)nD + 1, s)) || (rc = truncated.alloc(1, s))) return rc;
  MPG_HIP(hipMemsetAsync(truncated.p, 0, sizeof(int32_t), s));
  const unsigned nbd1 = (unsigned)((nD + 256) / 256), nbd = (unsigned)((nD + 255) / 256);
  const PyramidView pv = mpg_pyr_view(src->cellpyr);
  k_cg_candidates<false><<<nbd1, 256, 0, s>>>(gd, gs, od, orient_s.p, pv, cnt.p, nullptr, nullptr);
  MPG_HIP(hipGetLastError());
  if ((rc = mpg_scan_excl_i32(cnt.p, poff.p, nD + 1, s))) return rc;
  // the pair count twice -- the int32 scan's last entry and a 64-bit sum (the scan could wrap more than once) -- in ONE round trip
  int32_t npairs = 0;
  long long total = 0;
  {
    TmpBuf<long long> tot;
    if ((rc = tot.alloc(1, s))) return rc;
    if ((rc = mpg_sum_i32_i64(cnt.p, nD, tot.p, s))) return rc;
    MPG_HIP(hipMemcpyAsync(&npairs, poff.p + nD, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MPG_HIP(hipMemcpyAsync(&total, tot.p, sizeof(total), hipMemcpyDeviceToHost, s));
    MPG_HIP(hipStreamSynchronize(s));
    if (npairs < 0 || total != (long long)npairs) {
      mpg_set_error("%s: %lld candidate pairs exceed 2^31; a destination split into row blocks stores fewer each", who, total);
      return MPG_ERR_OVERFLOW;
    }
  }
  if ((rc = pair_d.alloc((size_t)npairs + 1, s)) || (rc = pair_s.alloc((size_t)npairs + 1, s)) || (rc = pair_val.alloc((size_t)npairs + 1, s))) return rc;
  k_cg_candidates<true><<<nbd1, 256, 0, s>>>(gd, gs, od, orient_s.p, pv, nullptr, poff.p, pair_s.p);
  k_cg_pair_dst<<<nbd, 256, 0, s>>>(nD, poff.p, pair_d.p);
  MPG_HIP(hipGetLastError());
  // (3) clip: one lane per pair
  if (npairs > 0)
    k_cg_clip_pairs<<<(unsigned)(((int64_t)npairs + CLIP_NT - 1) / CLIP_NT), CLIP_NT, 0, s>>>(npairs, pair_d.p, pair_s.p, gd, gs, od, orient_s.p,
                                                                                            pair_val.p, truncated.p);
  MPG_HIP(hipGetLastError());
  // (4) rows keyed by destination cell, columns = source cell ids ascending
  k_cg_row_count<<<nbd1, 256, 0, s>>>(nD, ad, poff.p, pair_val.p, cnt.p);
  MPG_HIP(hipGetLastError());
  if ((rc = mpg_scan_excl_i32(cnt.p, h->rowptr.p, nD + 1, s))) return rc;
  int32_t nnz = 0, was_truncated = 0;
  MPG_HIP(hipMemcpyAsync(&nnz, h->rowptr.p + nD, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipMemcpyAsync(&was_truncated, truncated.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipStreamSynchronize(s));
  if (was_truncated) {
    mpg_set_error("%s: a clipped polygon outgrew its %d vertex slots (a non-convex grid cell?)", who, CG_SLOTS);
    return MPG_ERR_OVERFLOW;
  }
  if (nnz < 0) {   // (at most one entry per pair, and the pairs were counted in 64 bits)
    mpg_set_error("%s: the weight matrix exceeds 2^31 entries", who);
    return MPG_ERR_OVERFLOW;
  }
  h->nnz = nnz;
  if ((rc = h->col.alloc((size_t)nnz + 1)) || (rc = h->val.alloc((size_t)nnz + 1))) return rc;
  k_cg_rows<<<nbd, 256, 0, s>>>(nD, ad, poff.p, pair_s.p, pair_val.p, h->rowptr.p, norm_type, h->col.p, h->val.p, h->dst_frac.p);
  MPG_HIP(hipGetLastError());
  MPG_HIP(hipStreamSynchronize(s));
  // mpg_handle_store_stats: [1] pairs clipped, [6] vertex slots of the clip
  h->store_stats[1] = npairs;
  h->store_stats[6] = CG_SLOTS;
  return MPG_SUCCESS;
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_store_conserve_grid() { return (const void *)k_cg_orient; }
