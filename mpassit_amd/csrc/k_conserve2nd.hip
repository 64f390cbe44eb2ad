// Second-order conservative regridding (mpg_handle_conserve2nd): a finished first-order conservative CSR handle turned into the CSR handle
// of a linear reconstruction inside every source cell (include/mpassit_amd.h states the rule, conserve2nd.h is its arithmetic).  The
// stored (destination, source) pairs are the candidate list: no search.  A Store-time family:
//
//   cell pass      k_c2_cells      one lane per cell of either side: the listed fan's sign (orientation byte) and |area|; for a source cell
//                                  also G_i, the unit vector of the counter-clockwise polygon's fan moment (the stored centre as fallback).
//   stencil pass   k_c2_stencil    one lane per source cell: N1(i) of patch.h minus i minus the masked cells, M, det, the test -> a count;
//                                  after mpg_scan_excl_i32 the same walk writes the ascending ids and the two b planes: a small CSR built
//                                  by count, scan, fill as k_patch.hip's.  The entry count is the call's one host round trip of its own.
//   piece pass     k_c2_piece      the hot one: one lane per stored entry q, its row found by a search of rowptr.  The source polygon sits
//                                  in LDS, [slot][component][lane] with CLIP_NT = 64 lanes (LdsPoly, clip_halfspace_lds of conserve_clip.h);
//                                  the destination cell's sides are re-read from memory side by side -- the lanes of a wavefront are
//                                  neighbouring entries of one or two rows, so these loads hit the same lines -- which keeps the LDS at
//                                  cb = (source + destination vertex counts) slots, at most 24 x 3 x 8 x 64 = 36 KB a workgroup: four
//                                  workgroups of one wavefront per CU by LDS (160 KB), the Mesh -> Mesh Store's figure.  -> A_q, m_q.
//   row pass       k_c2_rowsum     one lane per destination row: sum of A_q in stored order (MPG_NORM_FRACAREA's divisor).
//   centroid pass  k_c2_centroid   one lane per source over its segment of the handle's transposed index (ascending destination ids); the
//                                  entry is found in the destination row by a search of its ascending columns -> A_i, M_i.
//   entry pass     k_c2_entry      one lane per entry: delta_q in the frame of G_i, and w_q.
//   pattern        mpg_k_compose_pattern (k_compose.hip's symbolic job) with the stencil CSR as the inner operand: "compose_block_rows"
//                                  covers this call as well.
//   value pass     k_c2_values     one lane per entry (j, e) of the result: the row's entries in stored order, within each the stencil row
//                                  of its source, acc = acc + w_q * t.  No atomics: the same bytes from run to run.
// Integer atomics count the statistics and raise the truncation flag; none decides a stored byte.  All temporaries are TmpBuf.
#pragma clang fp contract(off)
#include <algorithm>

#include "geom.h"
#include "mpg_internal.h"
#include "conserve_clip.h"
#include "patch.h"
#include "conserve2nd.h"

// the cells of one side: a mesh's (voc [n][me] 1-based and 0-padded, the vertices' unit vectors) or a grid's (the CORNER points
// [(ny + 1)][(nx + 1)], cell id = j * nx + i)
struct C2Cells {
  const int32_t *voc;   // nullptr: a grid
  int me;               // listed slots per cell (4 on a grid)
  int64_t nV;
  const double *x, *y, *z;
  int nx;
  int64_t n;
  // listed slot k of cell c -> false: a pad
  __device__ __forceinline__ bool vertex(int64_t c, int k, double *p) const {
    int64_t v;
    if (voc) {
      v = (int64_t)voc[c * me + k] - 1;
      if (v < 0 || v >= nV) return false;
    } else {
      const int64_t i = c % nx, j = c / nx;
      v = (j + (k >> 1)) * (int64_t)(nx + 1) + i + ((k == 1 || k == 2) ? 1 : 0);
    }
    p[0] = x[v]; p[1] = y[v]; p[2] = z[v];
    return true;
  }
};

// the polygon of cell c, vertex by vertex, counter-clockwise when rev says that the listed order is clockwise -> f(p) per vertex
template <class F>
__device__ __forceinline__ void c2_walk(const C2Cells &P, int64_t c, bool rev, F f) {
  for (int s = 0; s < P.me; ++s) {
    double p[3];
    if (P.vertex(c, rev ? P.me - 1 - s : s, p)) f(p);
  }
}

struct C2Fan {   // the fan from the first vertex handed in
  double p0[3], prev[3], area, m[3];
  int n;
  __device__ __forceinline__ void init() {
    area = 0.0;
    m[0] = m[1] = m[2] = 0.0;
    n = 0;
  }
  __device__ __forceinline__ void add(const double *p) {
    if (n == 0) {
      p0[0] = p[0]; p0[1] = p[1]; p0[2] = p[2];
    } else if (n >= 2) {
      const double a = c2_tri_area(p0, prev, p);
      area = area + a;
      c2_moment_add(a, p0, prev, p, m);
    }
    prev[0] = p[0]; prev[1] = p[1]; prev[2] = p[2];
    ++n;
  }
};

static inline unsigned c2_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

// orient: 0 the listed order is counter-clockwise, 1 clockwise, 2 no polygon (fewer than three vertices or a fan area of 0); area = |fan|;
// G (source side only, [3][n]): the unit vector of the counter-clockwise polygon's moment, else the stored centre (cx, cy, cz)
__global__ __launch_bounds__(256) void k_c2_cells(C2Cells P, const double *__restrict__ cx, const double *__restrict__ cy,
                                                  const double *__restrict__ cz, uint8_t *__restrict__ orient, double *__restrict__ area,
                                                  double *__restrict__ G) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= P.n) return;
  C2Fan f;
  f.init();
  c2_walk(P, c, false, [&](const double *p) { f.add(p); });
  const bool none = f.n < 3 || f.area == 0.0, rev = f.area < 0.0;
  orient[c] = none ? 2 : rev ? 1 : 0;
  area[c] = none ? 0.0 : fabs(f.area);
  if (!G) return;
  if (rev) {
    f.init();
    c2_walk(P, c, true, [&](const double *p) { f.add(p); });
  }
  double g[3] = {cx[c], cy[c], cz[c]};
  if (f.n >= 3) (void)c2_unit(f.m, g);
  G[c] = g[0];
  G[P.n + c] = g[1];
  G[2 * P.n + c] = g[2];
}

// stats: [0] sources with a passing stencil, [1] sources without one
__device__ __forceinline__ int c2_wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

// FILL false: cnt[i] = the stencil's entries (cnt[n] = 0 for the scan).  true: ids ascending and the b planes from sptr[i] on
template <bool FILL>
__global__ __launch_bounds__(256) void k_c2_stencil(PtSrc src, int64_t n, const double *__restrict__ G, const uint8_t *__restrict__ mask,
                                                    int32_t *__restrict__ cnt, const int32_t *__restrict__ sptr, int32_t *__restrict__ scol,
                                                    double *__restrict__ sbx, double *__restrict__ sby, unsigned long long *__restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int pass = 0, fail = 0;
  if (i < n) {
    int32_t ids[PT_MAX_PNTS];
    const int n1 = src.ring1((int32_t)i, ids);
    const bool usable = n1 <= PT_MAX_PNTS && !(mask && mask[i]);
    const double Gi[3] = {G[i], G[n + i], G[2 * n + i]};
    double e1[3], e2[3];
    pt_frame(Gi, e1, e2);
    C2Sten st;
    c2_sten_init(st);
    auto member = [&](int32_t k) { return k != (int32_t)i && k >= 0 && (int64_t)k < n && !(mask && mask[k]); };
    if (usable)
      for (int a = 0; a < n1; ++a) {
        const int32_t k = ids[a];
        if (!member(k)) continue;
        const double Gk[3] = {G[k], G[n + k], G[2 * n + k]};
        double dx, dy;
        c2_sten_d(Gi, Gk, e1, e2, dx, dy);
        c2_sten_add(st, dx, dy);
      }
    const bool ok = usable && c2_sten_pass(st);
    pass = ok;
    fail = !ok;
    if (!FILL) {
      cnt[i] = ok ? st.n + 1 : 1;
    } else {
      int64_t w = sptr[i];
      const int64_t end = sptr[i + 1];
      if (!ok) {
        if (w < end) {
          scol[w] = (int32_t)i;
          sbx[w] = 0.0;
          sby[w] = 0.0;
        }
      } else {
        int64_t own = -1;
        double sx = 0.0, sy = 0.0;
        for (int a = 0; a < n1; ++a) {
          const int32_t k = ids[a];
          if (!member(k)) continue;
          if (own < 0 && k > (int32_t)i) own = w++;
          const double Gk[3] = {G[k], G[n + k], G[2 * n + k]};
          double dx, dy, bx, by;
          c2_sten_d(Gi, Gk, e1, e2, dx, dy);
          c2_sten_b(st, dx, dy, bx, by);
          sx = sx + bx;
          sy = sy + by;
          if (w < end) {   // (the count pass walked the same ring: always true)
            scol[w] = k;
            sbx[w] = bx;
            sby[w] = by;
          }
          ++w;
        }
        if (own < 0) own = w++;
        if (own < end) {
          scol[own] = (int32_t)i;
          sbx[own] = -sx;
          sby[own] = -sy;
        }
      }
    }
  } else if (!FILL && i == n) {
    cnt[i] = 0;
  }
  if (!FILL) {
    pass = c2_wave_sum(pass);
    fail = c2_wave_sum(fail);
    if ((threadIdx.x & 63) == 0) {   // (integer sums: the order does not matter)
      if (pass) atomicAdd(&stats[0], (unsigned long long)pass);
      if (fail) atomicAdd(&stats[1], (unsigned long long)fail);
    }
  }
}

// the first row whose end lies behind entry q
__device__ __forceinline__ int64_t c2_row_of(const int32_t *__restrict__ rowptr, int64_t nrows, int64_t q) {
  int64_t lo = 0, hi = nrows;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)rowptr[mid + 1] <= q) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// One lane per stored entry: A_q and m_q [3][nnz] of source cell col[q] inside the destination cell of q's row
__global__ __launch_bounds__(CLIP_NT) void k_c2_piece(int64_t nnz, int64_t nrows, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                      C2Cells S, const uint8_t *__restrict__ orient_s, C2Cells D,
                                                      const uint8_t *__restrict__ orient_d, int cb, double *__restrict__ Aq,
                                                      double *__restrict__ mq, int32_t *__restrict__ truncated) {
  extern __shared__ double c2_clip_lds[];   // [cb][3][CLIP_NT]
  const int64_t q = blockIdx.x * (int64_t)CLIP_NT + threadIdx.x;
  if (q >= nnz) return;
  const LdsPoly L{c2_clip_lds + threadIdx.x, cb};
  const int64_t j = c2_row_of(rowptr, nrows, q), i = col[q];
  double area = 0.0, m[3] = {0.0, 0.0, 0.0};
  int trunc = 0;
  if (j < nrows && i >= 0 && i < S.n && orient_s[i] != 2 && orient_d[j] != 2) {
    int n = 0;
    c2_walk(S, i, orient_s[i] == 1, [&](const double *p) {
      if (n < cb) L.set(0, n++, dv3{p[0], p[1], p[2]});
      else trunc = 1;
    });
    // the destination cell's sides in counter-clockwise order, the closing side last
    dv3 first = dv3{0, 0, 0}, prev = first;
    int nd = 0;
    auto side = [&](dv3 a, dv3 b) {
      if (n < 3) return;
      const dv3 ab = b - a;
      if (dot3(ab, ab) < 1e-24) return;   // collapsed side: bounds nothing
      n = clip_halfspace_lds(n, L, cross3(a, ab), cb, &trunc);
    };
    c2_walk(D, j, orient_d[j] == 1, [&](const double *p) {
      const dv3 x = dv3{p[0], p[1], p[2]};
      if (nd == 0) first = x;
      else side(prev, x);
      prev = x;
      ++nd;
    });
    if (nd >= 3) side(prev, first);
    else n = 0;
    if (n >= 3) {
      const dv3 v0 = L.get(0, 0);
      const double p0[3] = {v0.x, v0.y, v0.z};
      dv3 a = L.get(0, 1);
      for (int t = 1; t + 1 < n; ++t) {
        const dv3 b = L.get(0, t + 1);
        const double pa[3] = {a.x, a.y, a.z}, pb[3] = {b.x, b.y, b.z};
        const double at = c2_tri_area(p0, pa, pb);
        area = area + at;
        c2_moment_add(at, p0, pa, pb, m);
        a = b;
      }
      area = area > 0.0 ? area : 0.0;
    }
  }
  Aq[q] = area;
  mq[q] = m[0];
  mq[nnz + q] = m[1];
  mq[2 * nnz + q] = m[2];
  if (trunc) atomicOr(truncated, 1);   // (a flag for the error path, not a stored byte)
}

__global__ __launch_bounds__(256) void k_c2_rowsum(int64_t nrows, const int32_t *__restrict__ rowptr, const double *__restrict__ Aq,
                                                   double *__restrict__ rsum) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= nrows) return;
  double s = 0.0;
  for (int64_t q = rowptr[j]; q < rowptr[j + 1]; ++q) s = s + Aq[q];
  rsum[j] = s;
}

// A_i and M_i [3][n_src] over the pieces of source i in ascending destination id
__global__ __launch_bounds__(256) void k_c2_centroid(int64_t n_src, const int32_t *__restrict__ tr_ptr, const int32_t *__restrict__ tr_row,
                                                     int64_t nrows, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                     int64_t nnz, const double *__restrict__ Aq, const double *__restrict__ mq,
                                                     double *__restrict__ Ai, double *__restrict__ Mi) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_src) return;
  double A = 0.0, M[3] = {0.0, 0.0, 0.0};
  for (int64_t t = tr_ptr[i]; t < tr_ptr[i + 1]; ++t) {
    const int64_t j = tr_row[t];
    if (j < 0 || j >= nrows) continue;
    const int64_t b = rowptr[j], e = rowptr[j + 1];
    int64_t lo = b, hi = e;   // the first entry of the row whose column is not below i
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (col[mid] < (int32_t)i) lo = mid + 1;
      else hi = mid;
    }
    if (!(lo < e && col[lo] == (int32_t)i))   // (a row whose columns do not ascend, as a from-weights handle's may: the first match in stored order)
      for (lo = b; lo < e && col[lo] != (int32_t)i; ++lo) {}
    if (lo >= e) continue;
    A = A + Aq[lo];
    M[0] = M[0] + mq[lo];
    M[1] = M[1] + mq[nnz + lo];
    M[2] = M[2] + mq[2 * nnz + lo];
  }
  Ai[i] = A;
  Mi[i] = M[0];
  Mi[n_src + i] = M[1];
  Mi[2 * n_src + i] = M[2];
}

// delta_q = (ex, ey) and w_q of every stored entry; div: area(d) per row (MPG_NORM_DSTAREA) or the row sums (MPG_NORM_FRACAREA)
__global__ __launch_bounds__(256) void k_c2_entry(int64_t nnz, int64_t nrows, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                  int64_t n_src, const double *__restrict__ G, const double *__restrict__ Aq,
                                                  const double *__restrict__ mq, const double *__restrict__ Ai, const double *__restrict__ Mi,
                                                  const double *__restrict__ div, double *__restrict__ ex, double *__restrict__ ey,
                                                  double *__restrict__ w) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= nnz) return;
  const int64_t j = c2_row_of(rowptr, nrows, q), i = col[q];
  double dx = 0.0, dy = 0.0, wq = 0.0;
  if (j < nrows && i >= 0 && i < n_src) {
    const double Gi[3] = {G[i], G[n_src + i], G[2 * n_src + i]};
    double e1[3], e2[3];
    pt_frame(Gi, e1, e2);
    const double m[3] = {mq[q], mq[nnz + q], mq[2 * nnz + q]}, M[3] = {Mi[i], Mi[n_src + i], Mi[2 * n_src + i]};
    c2_offset(m, Aq[q], M, Ai[i], e1, e2, dx, dy);
    const double d = div[j];
    wq = d > 0.0 ? Aq[q] / d : 0.0;
  }
  ex[q] = dx;
  ey[q] = dy;
  w[q] = wq;
}

// One lane per entry (j, e) of the result
__global__ __launch_bounds__(256) void k_c2_values(int64_t nnz_c, int64_t nrows, const int32_t *__restrict__ crowptr, const int32_t *__restrict__ ccol,
                                                   const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t n_src,
                                                   const int32_t *__restrict__ sptr, const int32_t *__restrict__ scol,
                                                   const double *__restrict__ sbx, const double *__restrict__ sby, const double *__restrict__ ex,
                                                   const double *__restrict__ ey, const double *__restrict__ w, double *__restrict__ val) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= nnz_c) return;
  const int64_t j = c2_row_of(crowptr, nrows, c);
  double acc = 0.0;
  if (j < nrows) {
    const int32_t e = ccol[c];
    for (int64_t p = rowptr[j]; p < rowptr[j + 1]; ++p) {
      const int32_t i = col[p];
      if (i < 0 || (int64_t)i >= n_src) continue;
      for (int64_t k = sptr[i]; k < sptr[i + 1]; ++k) {
        if (scol[k] != e) continue;
        const double t = c2_t(ex[p], ey[p], sbx[k], sby[k], e == i);
        const double term = w[p] * t;
        acc = acc + term;
        break;   // (a stencil holds a column at most once)
      }
    }
  }
  val[c] = acc;
}

static void c2_cells(C2Cells &P, const mpg_mesh_s *m, const mpg_grid_s *g) {
  if (m) {
    P.voc = m->voc.p; P.me = m->maxEdges; P.nV = m->nVertices; P.x = m->vert.x.p; P.y = m->vert.y.p; P.z = m->vert.z.p; P.nx = 0; P.n = m->nCells;
  } else {
    const PointSet &c = g->pts[MPG_STAGGERLOC_CORNER];
    P.voc = nullptr; P.me = 4; P.nV = c.n; P.x = c.x.p; P.y = c.y.p; P.z = c.z.p; P.nx = g->nx; P.n = (int64_t)g->nx * g->ny;
  }
}

// in: a finished first-order conservative CSR handle; exactly one of (smesh, sgrid) and of (dmesh, dgrid): the cells it was stored between;
// ps: the source's rings (patch.h) and stored centres.  out: shape and method set by the caller, arrays empty.  Arguments checked by the
// API entry point; blocking.
int mpg_k_conserve2nd(mpg_handle_s *in, mpg_mesh_s *smesh, mpg_grid_s *sgrid, mpg_mesh_s *dmesh, mpg_grid_s *dgrid, const PtSrc &ps, int norm_type,
                      const uint8_t *src_mask, mpg_handle_s *out, hipStream_t s) {
  const char *who = "mpg_handle_conserve2nd";
  int rc;
  const int64_t nS = in->n_src, nD = in->n_dst, nnz = in->nnz;
  C2Cells S, D;
  c2_cells(S, smesh, sgrid);
  c2_cells(D, dmesh, dgrid);
  out->kind = MPG_KIND_CSR;
  out->nnz_per_row = 0;
  int nvs = 4, nvd = 4;
  if (smesh) {
    if ((rc = mpg_k_mesh_max_valence(smesh, s))) return rc;
    nvs = std::max(3, std::min(smesh->max_valence, smesh->maxEdges));
  }
  if (dmesh) {
    if ((rc = mpg_k_mesh_max_valence(dmesh, s))) return rc;
    nvd = std::max(3, std::min(dmesh->max_valence, dmesh->maxEdges));
  }
  const int cb = nvs + nvd;   // a convex m-gon cut by a convex n-gon has at most m + n vertices; <= 2 * CONS_MAXV = 24 slots
  if ((rc = mpg_k_transpose_build(in, s))) return rc;
  TmpBuf<uint8_t> orient_s, orient_d;
  TmpBuf<double> area_s, area_d, G, Aq, mq, rsum, Ai, Mi, ex, ey, w, sbx, sby;
  TmpBuf<int32_t> cnt, sptr, scol, truncated;
  TmpBuf<unsigned long long> stats;
  TmpBuf<long long> total;
  if ((rc = orient_s.alloc((size_t)nS + 1, s)) || (rc = orient_d.alloc((size_t)nD + 1, s)) || (rc = area_s.alloc((size_t)nS + 1, s)) ||
      (rc = area_d.alloc((size_t)nD + 1, s)) || (rc = G.alloc(3 * (size_t)nS + 1, s)) || (rc = Aq.alloc((size_t)nnz + 1, s)) ||
      (rc = mq.alloc(3 * (size_t)nnz + 1, s)) || (rc = rsum.alloc((size_t)nD + 1, s)) || (rc = Ai.alloc((size_t)nS + 1, s)) ||
      (rc = Mi.alloc(3 * (size_t)nS + 1, s)) || (rc = ex.alloc((size_t)nnz + 1, s)) || (rc = ey.alloc((size_t)nnz + 1, s)) ||
      (rc = w.alloc((size_t)nnz + 1, s)) || (rc = cnt.alloc((size_t)nS + 1, s)) || (rc = sptr.alloc((size_t)nS + 1, s)) ||
      (rc = truncated.alloc(1, s)) || (rc = stats.alloc(2, s)) || (rc = total.alloc(1, s)))
    return rc;
  MPG_HIP(hipMemsetAsync(stats.p, 0, sizeof(unsigned long long) * 2, s));
  MPG_HIP(hipMemsetAsync(truncated.p, 0, sizeof(int32_t), s));
  // (1) cells of both sides, (2) the stencils: count, the entry count's round trip, scan, fill
  if (nS > 0) k_c2_cells<<<c2_grid(nS), 256, 0, s>>>(S, ps.x, ps.y, ps.z, orient_s.p, area_s.p, G.p);
  if (nD > 0) k_c2_cells<<<c2_grid(nD), 256, 0, s>>>(D, nullptr, nullptr, nullptr, orient_d.p, area_d.p, nullptr);
  k_c2_stencil<false><<<c2_grid(nS + 1), 256, 0, s>>>(ps, nS, G.p, src_mask, cnt.p, nullptr, nullptr, nullptr, nullptr, stats.p);
  MPG_HIP(hipGetLastError());
  if ((rc = mpg_sum_i32_i64(cnt.p, nS + 1, total.p, s))) return rc;
  long long nsten = 0;
  unsigned long long st[2] = {0, 0};
  MPG_HIP(hipMemcpyAsync(&nsten, total.p, sizeof(long long), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipMemcpyAsync(st, stats.p, sizeof(st), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipStreamSynchronize(s));
  if (nsten > 0x7ffffffeLL) {
    mpg_set_error("%s: the stencils would have %lld entries, more than 2^31 - 2 (int32 offsets): convert the parts of the source separately", who,
                  nsten);
    return MPG_ERR_OVERFLOW;
  }
  if ((rc = mpg_scan_excl_i32(cnt.p, sptr.p, nS + 1, s))) return rc;
  if ((rc = scol.alloc((size_t)nsten + 1, s)) || (rc = sbx.alloc((size_t)nsten + 1, s)) || (rc = sby.alloc((size_t)nsten + 1, s))) return rc;
  if (nS > 0) k_c2_stencil<true><<<c2_grid(nS), 256, 0, s>>>(ps, nS, G.p, src_mask, nullptr, sptr.p, scol.p, sbx.p, sby.p, stats.p);
  MPG_HIP(hipGetLastError());
  // (3) pieces, row sums, centroids, offsets and weights
  if (nnz > 0) {
    const size_t lds = sizeof(double) * cb * 3 * CLIP_NT;
    if (lds > 48 * 1024) MPG_HIP(hipFuncSetAttribute((const void *)k_c2_piece, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    k_c2_piece<<<(unsigned)((nnz + CLIP_NT - 1) / CLIP_NT), CLIP_NT, lds, s>>>(nnz, nD, in->rowptr.p, in->col.p, S, orient_s.p, D, orient_d.p, cb,
                                                                              Aq.p, mq.p, truncated.p);
    MPG_HIP(hipGetLastError());
  }
  if (nD > 0) k_c2_rowsum<<<c2_grid(nD), 256, 0, s>>>(nD, in->rowptr.p, Aq.p, rsum.p);
  if (nS > 0) k_c2_centroid<<<c2_grid(nS), 256, 0, s>>>(nS, in->tr_ptr.p, in->tr_row.p, nD, in->rowptr.p, in->col.p, nnz, Aq.p, mq.p, Ai.p, Mi.p);
  if (nnz > 0)
    k_c2_entry<<<c2_grid(nnz), 256, 0, s>>>(nnz, nD, in->rowptr.p, in->col.p, nS, G.p, Aq.p, mq.p, Ai.p, Mi.p,
                                            norm_type == MPG_NORM_FRACAREA ? rsum.p : area_d.p, ex.p, ey.p, w.p);
  MPG_HIP(hipGetLastError());
  // (4) the pattern of (in . stencils) and the values
  rc = mpg_k_compose_pattern(in, sptr.p, scol.p, nS, out, s, [&]() -> int {
    if (out->nnz > 0)
      k_c2_values<<<c2_grid(out->nnz), 256, 0, s>>>(out->nnz, nD, out->rowptr.p, out->col.p, in->rowptr.p, in->col.p, nS, sptr.p, scol.p, sbx.p,
                                                    sby.p, ex.p, ey.p, w.p, out->val.p);
    MPG_HIP(hipGetLastError());
    return MPG_SUCCESS;
  });
  if (rc == MPG_ERR_OVERFLOW)
    mpg_set_error("%s: the second-order handle would have more than 2^31 - 2 entries (rowptr is int32): convert the parts of the destination "
                  "separately", who);
  if (rc) return rc;
  if (in->dst_frac.p && nD > 0) {
    if ((rc = out->dst_frac.alloc((size_t)nD))) return rc;
    MPG_HIP(hipMemcpyAsync(out->dst_frac.p, in->dst_frac.p, sizeof(double) * (size_t)nD, hipMemcpyDeviceToDevice, s));
  }
  int32_t h_trunc = 0;
  MPG_HIP(hipMemcpyAsync(&h_trunc, truncated.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipStreamSynchronize(s));   // (also: the temporaries may go)
  if (h_trunc) {
    mpg_set_error("%s: a clipped polygon outgrew its %d slots (a non-convex cell): the first-order handle's cells must be convex", who, cb);
    return MPG_ERR_OVERFLOW;
  }
  out->store_stats[1] = nnz;
  out->store_stats[2] = (int64_t)st[0];
  out->store_stats[3] = (int64_t)st[1];
  out->store_stats[4] = nsten;
  out->store_stats[6] = out->max_row;
  return MPG_SUCCESS;
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_conserve2nd() { return (const void *)&k_c2_cells; }
