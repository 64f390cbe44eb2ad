// Conservative Mesh -> Mesh weight generation: ESMF_FieldRegridStore(regridmethod=CONSERVE, normType=) with the elements of one Mesh as
// the source and the elements of another as the destination (mpg_regrid_store_conserve_mesh).
//
// Polygons on both sides are Voronoi cells from verticesOnCell with great-circle sides.  I(d, s), the area of source cell s inside
// destination cell d: the source cell is the subject polygon, made counter-clockwise by the sign of its own fan area (the listed order
// reversed when that is negative); it is clipped by the sides of the destination cell, made counter-clockwise the same way, in their
// order; clip planes have normals in difference form a x (b - a); a side with |b - a|^2 < 1e-24 bounds nothing; the area is the
// sph_tri_area fan from slot 0, clamped at 0.  The clip step, its inside rule and the cell area are conserve_clip.h's, unchanged: the
// arithmetic of the Mesh -> Grid and Grid -> Mesh Stores.  Rows are keyed by destination cell and built by the Grid -> Mesh Store's
// count -> scan -> ordered-insert kernels (mpg_k_conserve_rows): no atomic decides a stored byte.
//
// Candidates.  The rule: no pair with I > 0 is removed.  A box tree over the source mesh's cell polygons (Morton order of the cell centres,
// leaf = 8 cells, fan-out 8, built once per mesh and kept on it like the triangle tree) is walked by one thread per destination cell with
// the cell's own box; every source cell whose box meets it becomes a pair.  A count pass, a scan and a fill pass give the pair list
// grouped by destination cell at exact size: no fixed list length, no spill path.
// The box of a cell must hold the whole spherical polygon -- sides AND interior: a small cell wholly inside a large one crosses none of
// its sides.  A point of the polygon is p = q / |q| with q = sum l_i v_i a convex combination of the vertices, so q lies in the
// vertices' coordinate hull; |q|^2 = 1 - sum_{i<j} l_i l_j |v_i - v_j|^2 >= 1 - D^2 / 2 with D the largest chord between two vertices
// (sum_{i<j} l_i l_j <= 1/2), hence |p - q| = 1 - |q| <= 1 - sqrt(1 - D^2 / 2) <= D^2 / 2.  With e2 = max_i |v_i - v_0|^2, D <= 2 sqrt(e2):
// pad = 2 e2 + 1e-9 per axis (the 1e-9 absorbs the rounding of the comparison) -- the pad the Mesh -> Grid candidate pass puts around
// a cell.  Two polygons that share a point then have boxes that share it.  (The bulge of the longest SIDE over its chord, d^2 / 8, bounds
// the sides only; it would lose a polar cap's inner cell.)
// One thread per (destination, source) pair clips: the subject polygon in LDS, [vertex][component][lane], cb = the two meshes' largest
// vertex counts added -- a convex m-gon cut by a convex n-gon has at most m + n vertices --, the destination polygon in registers.
// No floating-point contraction in this translation unit (see k_store_conserve.hip).
#pragma clang fp contract(off)
#include <math.h>

#include <algorithm>

#include "geom.h"
#include "mpg_internal.h"
#include "conserve_clip.h"

#define CM_STACK 96   // 7 siblings pushed per level, <= MPG_BVH_MAXLEV levels (tree_walk.h: 77 entries at most)

// the padded coordinate hull of cell c (see the head of this file); false: fewer than three vertices
static_assert(CM_STACK >= WalkCap<BvhTree>::FILTER, "the stack holds the walk's proven bound (tree_walk.h): its guard is never taken");
__device__ __forceinline__ bool cell_box(int64_t c, int maxEdges, const int32_t *__restrict__ voc, const double *__restrict__ vx,
                                         const double *__restrict__ vy, const double *__restrict__ vz, double *lo, double *hi) {
  lo[0] = lo[1] = lo[2] = 2.0;
  hi[0] = hi[1] = hi[2] = -2.0;
  dv3 first = dv3{0, 0, 0};
  double e2 = 0.0;
  int n = 0;
  for (int j = 0; j < maxEdges && n < CONS_MAXV; ++j) {
    const int32_t v = voc[c * maxEdges + j];
    if (v <= 0) continue;
    const dv3 x = dv3{vx[v - 1], vy[v - 1], vz[v - 1]};
    if (n == 0) first = x;
    lo[0] = fmin(lo[0], x.x); hi[0] = fmax(hi[0], x.x);
    lo[1] = fmin(lo[1], x.y); hi[1] = fmax(hi[1], x.y);
    lo[2] = fmin(lo[2], x.z); hi[2] = fmax(hi[2], x.z);
    const dv3 d = x - first;
    e2 = fmax(e2, dot3(d, d));
    ++n;
  }
  if (n < 3) {
    lo[0] = lo[1] = lo[2] = 2.0;
    hi[0] = hi[1] = hi[2] = -2.0;
    return false;
  }
  const double pad = 2.0 * e2 + 1e-9;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] -= pad;
    hi[k] += pad;
  }
  return true;
}

// orientation of every cell, once per Store and mesh: 0 the listed order is counter-clockwise seen from outside, 1 it is clockwise (the
// clip reverses it), 2 no polygon (fewer than three vertices or a fan area of exactly 0): never part of a pair
__global__ __launch_bounds__(256) void k_cell_orient(int64_t nC, int maxEdges, const int32_t *__restrict__ voc, const double *__restrict__ vx,
                                                     const double *__restrict__ vy, const double *__restrict__ vz, uint8_t *__restrict__ orient) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= nC) return;
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
  orient[c] = (n < 3 || area == 0.0) ? 2 : (area < 0.0 ? 1 : 0);
}

__global__ __launch_bounds__(256) void k_cbvh_cellbox(int64_t n, const int32_t *__restrict__ sid, int maxEdges, const int32_t *__restrict__ voc,
                                                      const double *__restrict__ vx, const double *__restrict__ vy,
                                                      const double *__restrict__ vz, double *__restrict__ cellbox) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  double lo[3], hi[3];
  cell_box(sid[i], maxEdges, voc, vx, vy, vz, lo, hi);
  double *o = cellbox + 6 * i;
  o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = hi[0]; o[4] = hi[1]; o[5] = hi[2];
}

static int build_cell_bvh(mpg_mesh_s *m, hipStream_t s) {
  CellBvh &b = m->cbvh;
  if (b.built) return MPG_SUCCESS;
  int rc;
  const int64_t n = m->nCells;
  if ((rc = b.cellbox.alloc(6 * (size_t)n))) return rc;
  rc = mpg_bvh_build(
      b, n, "mpg_regrid_store_conserve_mesh",
      [&](unsigned long long *key, int32_t *id) { return mpg_k_morton(n, m->cell.x.p, m->cell.y.p, m->cell.z.p, key, id, 0, s); },
      [&]() {
        k_cbvh_cellbox<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(n, b.sorted_id.p, m->maxEdges, m->voc.p, m->vert.x.p, m->vert.y.p, m->vert.z.p,
                                                                   b.cellbox.p);
        static_assert(MPG_BVH_LEAF == MPG_BVH_FAN, "a leaf's box is the hull of its cells' boxes as an upper node's is of its children's");
        return mpg_k_bvh_up(n, b.nnodes[0], b.cellbox.p, b.box.p, s);
      },
      s, true);
  if (rc) b.free();
  return rc;
}

// One thread per destination cell: depth-first over the nodes whose box meets the cell's (its own loop, as k_mesh_bilinear's: the node to visit
// next in a register, only siblings on the stack); every source cell of every leaf reached whose own box meets it is a candidate.
// FILL = false counts them (cnt[d]; the scan's extra element cnt[nD] = 0), FILL = true writes them at poff[d] .. in the same order.
template <bool FILL>
__global__ __launch_bounds__(256) void k_cm_candidates(int64_t nD, int maxEdges, const int32_t *__restrict__ voc, const double *__restrict__ vx,
                                                       const double *__restrict__ vy, const double *__restrict__ vz,
                                                       const uint8_t *__restrict__ orient_d, const uint8_t *__restrict__ orient_s, CellBvhView b,
                                                       int32_t *__restrict__ cnt, const int32_t *__restrict__ poff, int32_t *__restrict__ pair_d,
                                                       int32_t *__restrict__ pair_s, int32_t *__restrict__ overflow) {
  const int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (d > nD) return;
  if (d == nD) {
    if (!FILL) cnt[d] = 0;
    return;
  }
  double lo[3], hi[3];
  int found = 0;
  const bool poly = orient_d[d] != 2 && cell_box(d, maxEdges, voc, vx, vy, vz, lo, hi);
  if (poly && b.n > 0) {
    const int32_t o = FILL ? poff[d] : 0, oe = FILL ? poff[d + 1] : 0;
    auto meets = [&](const double *bx) -> bool {
      return !(bx[0] > hi[0] || bx[3] < lo[0] || bx[1] > hi[1] || bx[4] < lo[1] || bx[2] > hi[2] || bx[5] < lo[2]);
    };
    int stack[CM_STACK];
    int sp = 0;
    const int top = b.nlev - 1;
    int cur = meets(b.box + 6 * b.off[top]) ? (top << 27) : -1;
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
          if (!meets(b.cellbox + 6 * i)) continue;
          const int32_t sc = b.sid[i];
          if (orient_s[sc] == 2) continue;
          if (FILL) {
            if (o + found < oe) {   // (the count pass walked the same tree: always true)
              pair_d[o + found] = (int32_t)d;
              pair_s[o + found] = sc;
            }
          }
          ++found;
        }
        continue;
      }
      const int64_t c0 = node * MPG_BVH_FAN, c1 = min(b.nnodes[lev - 1], c0 + MPG_BVH_FAN);
      for (int64_t c = c0; c < c1; ++c) {
        if (!meets(b.box + 6 * (b.off[lev - 1] + c))) continue;
        const int enc = ((lev - 1) << 27) | (int)c;
        if (cur < 0) cur = enc;
        else if (sp < CM_STACK) stack[sp++] = enc;
        else atomicOr(overflow, 1);   // cannot happen (see CM_STACK); reported, never silently dropped
      }
    }
  }
  if (!FILL) cnt[d] = found;
}

// One thread per pair: I(d, s) -> pair_val.  Both polygons are fetched as k_conserve_clip_pairs fetches its one: all vertex numbers, then
// all coordinates, then use.  The destination polygon is put in order through the lane's own LDS column (slots 0 .. nd - 1, which the
// subject polygon overwrites afterwards) and read back into registers with constant indices; its sides are taken by shifting that array.
__global__ __launch_bounds__(CLIP_NT) void k_cm_clip_pairs(int64_t npairs, const int32_t *__restrict__ pair_d, const int32_t *__restrict__ pair_s,
                                                           int me_s, const int32_t *__restrict__ voc_s, const double *__restrict__ sx,
                                                           const double *__restrict__ sy, const double *__restrict__ sz,
                                                           const uint8_t *__restrict__ orient_s, int me_d, const int32_t *__restrict__ voc_d,
                                                           const double *__restrict__ dx, const double *__restrict__ dy,
                                                           const double *__restrict__ dz, const uint8_t *__restrict__ orient_d, int cb,
                                                           double *__restrict__ pair_val, int32_t *__restrict__ truncated) {
  extern __shared__ double cm_clip_lds[];   // [cb][3][CLIP_NT]
  const int64_t t = blockIdx.x * (int64_t)CLIP_NT + threadIdx.x;
  if (t >= npairs) return;
  const LdsPoly L{cm_clip_lds + threadIdx.x, cb};
  const int64_t d = pair_d[t], c = pair_s[t];
  int32_t vid_s[CONS_MAXV], vid_d[CONS_MAXV];
#pragma unroll
  for (int k = 0; k < CONS_MAXV; ++k) {
    vid_s[k] = k < me_s ? voc_s[c * me_s + k] : 0;
    vid_d[k] = k < me_d ? voc_d[d * me_d + k] : 0;
  }
  const bool rev_s = orient_s[c] == 1, rev_d = orient_d[d] == 1;
  int ns_tot = 0, nd_tot = 0, safe_s = 0, safe_d = 0;
#pragma unroll
  for (int k = 0; k < CONS_MAXV; ++k) {
    if (vid_s[k] > 0) {
      ++ns_tot;
      if (safe_s == 0) safe_s = vid_s[k];
    }
    if (vid_d[k] > 0) {
      ++nd_tot;
      if (safe_d == 0) safe_d = vid_d[k];
    }
  }
  double ar = 0.0;
  int trunc = 0;
  if (safe_s > 0 && safe_d > 0 && ns_tot <= cb && nd_tot <= cb) {   // (cb >= both counts by construction: the LDS slots stay in bounds whatever the input)
    dv3 vs[CONS_MAXV], vd[CONS_MAXV];   // padding entries re-load the cell's first vertex
#pragma unroll
    for (int k = 0; k < CONS_MAXV; ++k) {
      const int64_t a = (vid_s[k] > 0 ? vid_s[k] : safe_s) - 1, b = (vid_d[k] > 0 ? vid_d[k] : safe_d) - 1;
      vs[k] = dv3{sx[a], sy[a], sz[a]};
      vd[k] = dv3{dx[b], dy[b], dz[b]};
    }
    int nd = 0;
#pragma unroll
    for (int k = 0; k < CONS_MAXV; ++k)
      if (vid_d[k] > 0) {
        L.set(0, rev_d ? nd_tot - 1 - nd : nd, vd[k]);
        ++nd;
      }
    dv3 q[CONS_MAXV];
#pragma unroll
    for (int k = 0; k < CONS_MAXV; ++k) q[k] = k < nd ? L.get(0, k) : dv3{0, 0, 0};
    int n = 0;
#pragma unroll
    for (int k = 0; k < CONS_MAXV; ++k)
      if (vid_s[k] > 0) {
        L.set(0, rev_s ? ns_tot - 1 - n : n, vs[k]);
        ++n;
      }
    // side e runs from q[0] to q[1] after e shifts of the register array by one vertex (constant indices only: an array indexed by e
    // would live in scratch memory); the closing side ends at the first vertex
    const dv3 qfirst = q[0];
    for (int e = 0; e < nd && n >= 3; ++e) {
      const dv3 qa = q[0], qb = e + 1 == nd ? qfirst : q[1];
#pragma unroll
      for (int k = 0; k + 1 < CONS_MAXV; ++k) q[k] = q[k + 1];
      const dv3 side = qb - qa;
      if (dot3(side, side) < 1e-24) continue;     // collapsed side: bounds nothing
      n = clip_halfspace_lds(n, L, cross3(qa, side), cb, &trunc);
    }
    if (n >= 3) {
      double sa = 0.0;
      const dv3 v0 = L.get(0, 0);
      for (int k = 1; k + 1 < n; ++k) sa += sph_tri_area(v0, L.get(0, k), L.get(0, k + 1));
      ar = sa > 0.0 ? sa : 0.0;
    }
  }
  pair_val[t] = ar;
  if (trunc) atomicOr(truncated, 1);   // (a flag for the error path, not a stored byte)
}

int mpg_k_store_conserve_mesh(mpg_mesh_s *src, mpg_mesh_s *dst, int norm_type, mpg_handle_s *h, hipStream_t s) {
  int rc;
  if (src->maxEdges > CONS_MAXV || dst->maxEdges > CONS_MAXV) {
    mpg_set_error("mpg_regrid_store_conserve_mesh: maxEdges %d > %d", std::max(src->maxEdges, dst->maxEdges), CONS_MAXV);
    return MPG_ERR_UNSUPPORTED;
  }
  const int64_t nS = src->nCells, nD = dst->nCells;   // (window meshes are refused by the entry point: every cell is resident)
  h->kind = MPG_KIND_CSR;
  h->nnz_per_row = 0;
  h->n_src = nS;
  h->n_dst = nD;
  h->nx_dst = (int)nD;
  h->ny_dst = 1;
  h->store_path = 0;
  if ((rc = h->rowptr.alloc((size_t)nD + 1)) || (rc = h->dst_frac.alloc((size_t)std::max<int64_t>(nD, 1)))) return rc;
  if (nD == 0 || nS == 0) {   // nothing to intersect: the empty matrix
    MPG_HIP(hipMemsetAsync(h->rowptr.p, 0, sizeof(int32_t) * (size_t)(nD + 1), s));
    if (nD > 0) MPG_HIP(hipMemsetAsync(h->dst_frac.p, 0, sizeof(double) * (size_t)nD, s));
    MPG_HIP(hipStreamSynchronize(s));
    if ((rc = h->col.alloc(1)) || (rc = h->val.alloc(1))) return rc;
    h->nnz = 0;
    return MPG_SUCCESS;
  }
  if ((rc = mpg_k_mesh_max_valence(src, s)) || (rc = mpg_k_mesh_max_valence(dst, s))) return rc;
  const bool had = src->cbvh.built;
  if ((rc = build_cell_bvh(src, s))) return rc;
  const CellBvh &b = src->cbvh;
  CellBvhView v;
  mpg_bvh_view(b, v);
  v.cellbox = b.cellbox.p;
  const double *sx = src->vert.x.p, *sy = src->vert.y.p, *sz = src->vert.z.p, *dx = dst->vert.x.p, *dy = dst->vert.y.p, *dz = dst->vert.z.p;
  // (1) orientation of both meshes' cells
  TmpBuf<uint8_t> orient_s, orient_d;
  if ((rc = orient_s.alloc((size_t)nS, s))) return rc;
  k_cell_orient<<<(unsigned)((nS + 255) / 256), 256, 0, s>>>(nS, src->maxEdges, src->voc.p, sx, sy, sz, orient_s.p);
  const uint8_t *od = orient_s.p;
  if (dst != src) {
    if ((rc = orient_d.alloc((size_t)nD, s))) return rc;
    k_cell_orient<<<(unsigned)((nD + 255) / 256), 256, 0, s>>>(nD, dst->maxEdges, dst->voc.p, dx, dy, dz, orient_d.p);
    od = orient_d.p;
  }
  MPG_HIP(hipGetLastError());
  // (2) candidates: count, scan, fill -- the pair list grouped by destination cell
  TmpBuf<int32_t> cnt, poff, ovf, pair_d, pair_s, truncated;
  TmpBuf<double> pair_val;
  if ((rc = cnt.alloc((size_t)nD + 1, s)) || (rc = poff.alloc((size_t)nD + 1, s)) || (rc = ovf.alloc(1, s)) || (rc = truncated.alloc(1, s))) return rc;
  MPG_HIP(hipMemsetAsync(ovf.p, 0, sizeof(int32_t), s));
  MPG_HIP(hipMemsetAsync(truncated.p, 0, sizeof(int32_t), s));
  const unsigned nbd = (unsigned)((nD + 256) / 256);
  k_cm_candidates<false><<<nbd, 256, 0, s>>>(nD, dst->maxEdges, dst->voc.p, dx, dy, dz, od, orient_s.p, v, cnt.p, nullptr, nullptr, nullptr, ovf.p);
  MPG_HIP(hipGetLastError());
  if ((rc = mpg_scan_excl_i32(cnt.p, poff.p, nD + 1, s))) return rc;
  // the pair count twice -- the int32 scan's last entry and a 64-bit sum (the scan could wrap more than once) -- in ONE round trip
  int32_t npairs = 0, h_ovf = 0;
  long long total = 0;
  {
    TmpBuf<long long> tot;
    if ((rc = tot.alloc(1, s))) return rc;
    if ((rc = mpg_sum_i32_i64(cnt.p, nD, tot.p, s))) return rc;
    MPG_HIP(hipMemcpyAsync(&npairs, poff.p + nD, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MPG_HIP(hipMemcpyAsync(&total, tot.p, sizeof(total), hipMemcpyDeviceToHost, s));
    MPG_HIP(hipMemcpyAsync(&h_ovf, ovf.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MPG_HIP(hipStreamSynchronize(s));
    if (h_ovf) {
      mpg_set_error("mpg_regrid_store_conserve_mesh: the traversal stack of the candidate search overflowed");
      return MPG_ERR_OVERFLOW;
    }
    if (npairs < 0 || total != (long long)npairs) {
      mpg_set_error("mpg_regrid_store_conserve_mesh: %lld candidate pairs exceed 2^31", total);
      return MPG_ERR_OVERFLOW;
    }
  }
  if ((rc = pair_d.alloc((size_t)npairs + 1, s)) || (rc = pair_s.alloc((size_t)npairs + 1, s)) || (rc = pair_val.alloc((size_t)npairs + 1, s))) return rc;
  k_cm_candidates<true><<<nbd, 256, 0, s>>>(nD, dst->maxEdges, dst->voc.p, dx, dy, dz, od, orient_s.p, v, nullptr, poff.p, pair_d.p, pair_s.p, ovf.p);
  MPG_HIP(hipGetLastError());
  // (3) clip: one thread per pair.  Slots: a convex m-gon cut by a convex n-gon has at most m + n vertices
  const int nvs = std::max(3, std::min(src->max_valence, src->maxEdges)), nvd = std::max(3, std::min(dst->max_valence, dst->maxEdges));
  const int cb = nvs + nvd;   // <= 2 * CONS_MAXV = 24: 36 KB
  const size_t clip_lds_bytes = sizeof(double) * cb * 3 * CLIP_NT;
  if (clip_lds_bytes > 48 * 1024)
    MPG_HIP(hipFuncSetAttribute((const void *)k_cm_clip_pairs, hipFuncAttributeMaxDynamicSharedMemorySize, (int)clip_lds_bytes));
  if (npairs > 0)
    k_cm_clip_pairs<<<(unsigned)(((int64_t)npairs + CLIP_NT - 1) / CLIP_NT), CLIP_NT, clip_lds_bytes, s>>>(
        npairs, pair_d.p, pair_s.p, src->maxEdges, src->voc.p, sx, sy, sz, orient_s.p, dst->maxEdges, dst->voc.p, dx, dy, dz, od, cb, pair_val.p,
        truncated.p);
  MPG_HIP(hipGetLastError());
  // (4) rows keyed by destination cell, columns = source cell ids ascending
  if ((rc = mpg_k_conserve_rows(dst, poff.p, pair_s.p, pair_val.p, truncated.p, cb, norm_type, "mpg_regrid_store_conserve_mesh", h, s))) return rc;
  // mpg_handle_store_stats: [1] pairs clipped, [2] destination cells that left the common path (there is one path: 0), [3] microseconds of
  // GPU time this Store spent building the source mesh's cell tree (0: the mesh had it already), [6] polygon slots of the clip
  h->store_stats[1] = npairs;
  h->store_stats[2] = 0;
  h->store_stats[3] = had ? 0 : (int64_t)(b.build_ms * 1e3f);
  h->store_stats[6] = cb;
  return MPG_SUCCESS;
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_store_conserve_mesh() { return (const void *)k_cell_orient; }
