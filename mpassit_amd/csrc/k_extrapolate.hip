// Extrapolation (mpg_handle_extrapolate): the unmapped rows of a route handle filled from the K nearest source points, as a NEW handle of
// the same shape (include/mpassit_amd.h states the contract).  A Store-time family of three passes:
//
//   pass 1  k_ex_flag      1 where a row is unmapped (fixed: slot 0's index < 0; CSR: an empty row); mpg_scan_excl_i32 numbers them and
//           k_ex_compact   lists them in ascending row order, so that neighbouring list entries are neighbouring points.  The count is read back.
//   pass 2  k_ex_knn<Src, KCAP>   one thread per listed point: knn_search (knn.h) through the source's tree -- the mesh's site BVH built whole
//                          (ExMeshSrc: a leaf = 8 sorted sites) or a stagger's point pyramid (ExGridSrc: a leaf = a 4 x 4 block of points) --
//                          with the pinned distance arithmetic (dist2_nofma, boxdist2_nofma).  Writes ids[KCAP][nu], d2[KCAP][nu] (SoA) and
//                          the row's entry count: 1 for nearest-source-to-destination and under the coincidence rule, n_src when the
//                          source set is smaller than N.  KCAP in {1, 2, 4, 8}; the list stays in VGPRs, the only scratch is the walk's stack.
//   pass 3  fixed output   idx / w copied, then k_ex_fill_fixed<KCAP> overwrites the listed rows: entries in slots 0 .. k - 1, every
//                          remaining slot repeats entry 0's id with weight +0.0
//           CSR output     k_ex_rowlen -> the 64-bit entry count (read back, checked) -> mpg_scan_excl_i32 -> k_ex_fill_csr<KCAP>: mapped rows
//                          copied (a fixed row: its slots in slot order, a nearest handle's weight 1.0), new rows written in ascending
//                          (d2, id) order, which is the Regrid's summation order; the longest row is recorded (an integer maximum)
// The weights are knn_weights (knn.h): one text for device and host.  No floating-point atomics: the same bytes from run to run.
//
// mpg_handle_extrapolate_masked runs the same passes with two changes.  k_ex_flag_skip leaves the rows of dst_skip out of the list.  With a
// source mask, K = min(N, unmasked sources) (k_ex_unmasked, summed), one `alive` byte per tree node is built bottom-up (k_ex_alive_leaf,
// then k_ex_alive_up per level: knn_mask.h says why) and k_ex_knn_masked<Src, KCAP> walks the AliveTree: it never enters a subtree without
// an unmasked source, and its leaf bodies test mask[id] before they compute a distance.  Without a mask the unmasked kernels run as they are.
// The two searched sets -- ExMeshSrc, ExGridSrc: the tree plus its leaf bodies leaf / leaf_masked / leaf_alive -- live in knn_src.h, which
// k_store_dtos.hip shares; leaf_masked opens every item with `if (mask[c]) continue;`, ahead of dist2_nofma.
#include "geom.h"
#include "knn.h"
#include "knn_mask.h"
#include "knn_src.h"
#include "mpg_internal.h"

#define EX_MAX_SLOTS 4   // slots per row of a fixed handle (3, 4 or 1)

struct ExIn {
  const int32_t *rowptr;   // CSR row pointers; nullptr: fixed slots
  const int32_t *col;      // CSR columns, or idx [nz][n] (-1 = none)
  const double *val;       // CSR values, or w [nz][n]; nullptr: every value 1.0 (nearest)
  int nz;                  // slots of a fixed handle
  int64_t n;               // rows
};

static ExIn ex_in(const mpg_handle_s *h) {
  ExIn o;
  if (h->kind == MPG_KIND_CSR) {
    o.rowptr = h->rowptr.p; o.col = h->col.p; o.val = h->val.p; o.nz = 0;
  } else {
    o.rowptr = nullptr; o.col = h->idx.p; o.val = h->w.p; o.nz = h->nnz_per_row;
  }
  o.n = h->n_dst;
  return o;
}

static inline unsigned ex_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

// flag[i] for i < n, and flag[n] = 0 so that the scan of n + 1 flags ends in the count
__global__ __launch_bounds__(256) void k_ex_flag(ExIn in, int32_t *__restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > in.n) return;
  int f = 0;
  if (i < in.n) f = in.rowptr ? in.rowptr[i + 1] == in.rowptr[i] : in.col[i] < 0;
  flag[i] = f;
}

// ... the same with the rows of `skip` left out (mpg_handle_extrapolate_masked's dst_skip): they stay unmapped
__global__ __launch_bounds__(256) void k_ex_flag_skip(ExIn in, const uint8_t *__restrict__ skip, int32_t *__restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > in.n) return;
  int f = 0;
  if (i < in.n && !skip[i]) f = in.rowptr ? in.rowptr[i + 1] == in.rowptr[i] : in.col[i] < 0;
  flag[i] = f;
}

// u[c] = 1 for an unmasked source (summed: the candidates' count)
__global__ __launch_bounds__(256) void k_ex_unmasked(int64_t n, const uint8_t *__restrict__ mask, int32_t *__restrict__ u) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c < n) u[c] = mask[c] == 0;
}

// the alive bytes of knn_mask.h, one kernel per level: the leaves from the mask, every upper level from the one below
template <class Src>
__global__ __launch_bounds__(256) void k_ex_alive_leaf(Src src, int64_t leaves, const uint8_t *__restrict__ mask, uint8_t *__restrict__ alive) {
  const int64_t node = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (node < leaves) alive[src.tree().v.off[0] + node] = src.leaf_alive((int)node, mask);
}
template <class Src>
__global__ __launch_bounds__(256) void k_ex_alive_up(Src src, int lev, int64_t nodes, uint8_t *alive) {
  const int64_t node = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (node < nodes) alive[src.tree().v.off[lev] + node] = alive_parent(src.tree(), lev, (int)node, alive);
}

__global__ __launch_bounds__(256) void k_ex_compact(int64_t n, const int32_t *__restrict__ flag, const int32_t *__restrict__ pos,
                                                    int32_t *__restrict__ list) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && flag[i]) list[pos[i]] = (int32_t)i;
}

template <class Src, int KCAP>
__global__ __launch_bounds__(256) void k_ex_knn(int64_t nu, const int32_t *__restrict__ list, const double *__restrict__ px,
                                                const double *__restrict__ py, const double *__restrict__ pz, Src src, int idavg, int kmax,
                                                int32_t *__restrict__ ids, double *__restrict__ d2, int32_t *__restrict__ cnt) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= nu) return;
  const int64_t p = list[u];
  const double X = px[p], Y = py[p], Z = pz[p];
  KBest<KCAP> best;
  knn_search(
      src.tree(), [&](const double *bx) { return boxdist2_nofma(X, Y, Z, bx); }, [&](int node, auto f) { src.leaf(node, X, Y, Z, f); }, best);
#pragma unroll
  for (int k = 0; k < KCAP; ++k) {
    ids[(int64_t)k * nu + u] = best.id[k];
    d2[(int64_t)k * nu + u] = best.d2[k];
  }
  cnt[u] = (!idavg || best.d2[0] == 0.0) ? min(best.n, 1) : min(best.n, kmax);   // (KCAP >= N: the list may hold more than the row takes)
}

// the same search over the unmasked sources alone, through the alive bytes (the caller launches it only when a source is unmasked; a
// dead root would be no search at all: knn_search_masked)
template <class Src, int KCAP>
__global__ __launch_bounds__(256) void k_ex_knn_masked(int64_t nu, const int32_t *__restrict__ list, const double *__restrict__ px,
                                                       const double *__restrict__ py, const double *__restrict__ pz, Src src,
                                                       const uint8_t *__restrict__ mask, const uint8_t *__restrict__ alive, int idavg, int kmax,
                                                       int32_t *__restrict__ ids, double *__restrict__ d2, int32_t *__restrict__ cnt) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= nu) return;
  const int64_t p = list[u];
  const double X = px[p], Y = py[p], Z = pz[p];
  KBest<KCAP> best;
  knn_search_masked(
      src.tree(), alive, [&](const double *bx) { return boxdist2_nofma(X, Y, Z, bx); },
      [&](int node, auto f) { src.leaf_masked(node, X, Y, Z, mask, f); }, best);
#pragma unroll
  for (int k = 0; k < KCAP; ++k) {
    ids[(int64_t)k * nu + u] = best.id[k];
    d2[(int64_t)k * nu + u] = best.d2[k];
  }
  cnt[u] = (!idavg || best.d2[0] == 0.0) ? min(best.n, 1) : min(best.n, kmax);
}

// the entries of listed row u: ids, weights, count
template <int KCAP>
__device__ __forceinline__ int ex_row(int64_t u, int64_t nu, const int32_t *__restrict__ ids, const double *__restrict__ d2,
                                      const int32_t *__restrict__ cnt, int idavg, double e, int32_t (&id)[KCAP], double (&w)[KCAP]) {
  double d[KCAP];
#pragma unroll
  for (int k = 0; k < KCAP; ++k) {
    id[k] = ids[(int64_t)k * nu + u];
    d[k] = d2[(int64_t)k * nu + u];
    w[k] = 0.0;
  }
  return knn_weights(d, cnt[u], idavg != 0, e, w);
}

// out_idx [nz][n], out_w [nz][n] or nullptr (a nearest handle stays without weights: every new row is one entry of weight 1)
template <int KCAP>
__global__ __launch_bounds__(256) void k_ex_fill_fixed(int64_t nu, const int32_t *__restrict__ list, const int32_t *__restrict__ ids,
                                                       const double *__restrict__ d2, const int32_t *__restrict__ cnt, int idavg, double e,
                                                       int nz, int64_t n, int32_t *__restrict__ out_idx, double *__restrict__ out_w) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= nu) return;
  int32_t id[KCAP];
  double w[KCAP];
  const int k = ex_row<KCAP>(u, nu, ids, d2, cnt, idavg, e, id, w);
  if (k == 0) return;   // no source points at all: the row stays unmapped
  const int64_t p = list[u];
#pragma unroll
  for (int s = 0; s < EX_MAX_SLOTS; ++s) {
    if (s < nz) {
      const bool own = s < KCAP && s < k;
      out_idx[(int64_t)s * n + p] = own ? id[s < KCAP ? s : 0] : id[0];
      if (out_w) out_w[(int64_t)s * n + p] = own ? w[s < KCAP ? s : 0] : 0.0;
    }
  }
}

// len[i] for i < n (a mapped fixed row: its slots that hold an index), len[n] = 0
__global__ __launch_bounds__(256) void k_ex_rowlen(ExIn in, const int32_t *__restrict__ flag, const int32_t *__restrict__ pos, int64_t nu,
                                                   const int32_t *__restrict__ cnt, int32_t *__restrict__ len) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > in.n) return;
  int v = 0;
  if (i < in.n) {
    if (flag[i]) v = nu > 0 ? cnt[pos[i]] : 0;   // (nu == 0 with a flag: there is no source point to fill from)
    else if (in.rowptr) v = in.rowptr[i + 1] - in.rowptr[i];
    else
      for (int s = 0; s < in.nz; ++s) v += in.col[(int64_t)s * in.n + i] >= 0;
  }
  len[i] = v;
}

template <int KCAP>
__global__ __launch_bounds__(256) void k_ex_fill_csr(ExIn in, const int32_t *__restrict__ flag, const int32_t *__restrict__ pos, int64_t nu,
                                                     const int32_t *__restrict__ ids, const double *__restrict__ d2,
                                                     const int32_t *__restrict__ cnt, int idavg, double e, const int32_t *__restrict__ rowptr,
                                                     int32_t *__restrict__ col, double *__restrict__ val, int32_t *__restrict__ longest) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int32_t len = 0;
  if (i < in.n) {
    int64_t at = rowptr[i];
    len = rowptr[i + 1] - (int32_t)at;
    if (flag[i]) {
      if (nu > 0) {
        int32_t id[KCAP];
        double w[KCAP];
        const int k = ex_row<KCAP>(pos[i], nu, ids, d2, cnt, idavg, e, id, w);
#pragma unroll
        for (int q = 0; q < KCAP; ++q)
          if (q < k) {
            col[at + q] = id[q];
            val[at + q] = w[q];
          }
      }
    } else if (in.rowptr) {
      const int64_t b = in.rowptr[i];
      for (int q = 0; q < len; ++q) {
        col[at + q] = in.col[b + q];
        val[at + q] = in.val[b + q];
      }
    } else {
      for (int s = 0; s < in.nz; ++s) {
        const int32_t c = in.col[(int64_t)s * in.n + i];
        if (c < 0) continue;
        col[at] = c;
        val[at] = in.val ? in.val[(int64_t)s * in.n + i] : 1.0;
        ++at;
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) len = max(len, __shfl_down(len, o));
  if ((threadIdx.x & 63) == 0 && len > 0) atomicMax(longest, len);   // (an integer maximum: the order does not matter)
}

template <class Src>
static void ex_launch_knn(int kcap, int64_t nu, const int32_t *list, const PointSet &dst, const Src &src, int idavg, int kmax, int32_t *ids,
                          double *d2, int32_t *cnt, hipStream_t s) {
  const unsigned nb = ex_grid(nu);
  if (kcap == 1) k_ex_knn<Src, 1><<<nb, 256, 0, s>>>(nu, list, dst.x.p, dst.y.p, dst.z.p, src, idavg, kmax, ids, d2, cnt);
  else if (kcap == 2) k_ex_knn<Src, 2><<<nb, 256, 0, s>>>(nu, list, dst.x.p, dst.y.p, dst.z.p, src, idavg, kmax, ids, d2, cnt);
  else if (kcap == 4) k_ex_knn<Src, 4><<<nb, 256, 0, s>>>(nu, list, dst.x.p, dst.y.p, dst.z.p, src, idavg, kmax, ids, d2, cnt);
  else k_ex_knn<Src, 8><<<nb, 256, 0, s>>>(nu, list, dst.x.p, dst.y.p, dst.z.p, src, idavg, kmax, ids, d2, cnt);
}

template <class Src>
static void ex_launch_knn_masked(int kcap, int64_t nu, const int32_t *list, const PointSet &dst, const Src &src, const uint8_t *mask,
                                 const uint8_t *alive, int idavg, int kmax, int32_t *ids, double *d2, int32_t *cnt, hipStream_t s) {
  const unsigned nb = ex_grid(nu);
  if (kcap == 1) k_ex_knn_masked<Src, 1><<<nb, 256, 0, s>>>(nu, list, dst.x.p, dst.y.p, dst.z.p, src, mask, alive, idavg, kmax, ids, d2, cnt);
  else if (kcap == 2) k_ex_knn_masked<Src, 2><<<nb, 256, 0, s>>>(nu, list, dst.x.p, dst.y.p, dst.z.p, src, mask, alive, idavg, kmax, ids, d2, cnt);
  else if (kcap == 4) k_ex_knn_masked<Src, 4><<<nb, 256, 0, s>>>(nu, list, dst.x.p, dst.y.p, dst.z.p, src, mask, alive, idavg, kmax, ids, d2, cnt);
  else k_ex_knn_masked<Src, 8><<<nb, 256, 0, s>>>(nu, list, dst.x.p, dst.y.p, dst.z.p, src, mask, alive, idavg, kmax, ids, d2, cnt);
}

// the alive bytes of the source's tree under `mask`, bottom-up: one launch per level (nlev and the level sizes are the host's own copy)
template <class Src>
static int ex_alive_build(const Src &src, int nlev, const int64_t *level_nodes, const uint8_t *mask, uint8_t *alive, hipStream_t s) {
  k_ex_alive_leaf<Src><<<ex_grid(level_nodes[0]), 256, 0, s>>>(src, level_nodes[0], mask, alive);
  for (int lev = 1; lev < nlev; ++lev) k_ex_alive_up<Src><<<ex_grid(level_nodes[lev]), 256, 0, s>>>(src, lev, level_nodes[lev], alive);
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

// in: the handle to fill.  Exactly one of src_mesh (its cells) / src_grid (its `src_stagger` points, which exist) is set; dst: the
// destination points, in.n_dst of them.  out: shape and method set by the caller, arrays empty.  Blocking.
// src_mask [n_src] / dst_skip [n_dst]: device bytes or nullptr (mpg_handle_extrapolate_masked); who: the entry point the messages name.
int mpg_k_extrapolate(mpg_handle_s *in, mpg_mesh_s *src_mesh, mpg_grid_s *src_grid, int src_stagger, const PointSet &dst, int method, int npnts,
                      double e, mpg_handle_s *out, hipStream_t s, const uint8_t *src_mask, const uint8_t *dst_skip, const char *who) {
  int rc;
  const int64_t n = in->n_dst, n_src = in->n_src;
  const int idavg = method == MPG_EXTRAPMETHOD_NEAREST_IDAVG;
  const int N = idavg ? npnts : 1;
  const int kcap = N <= 1 ? 1 : N <= 2 ? 2 : N <= 4 ? 4 : 8;
  const ExIn I = ex_in(in);
  const bool fixed_out = in->kind == MPG_KIND_FIXED && N <= in->nnz_per_row;
  if (in->kind == MPG_KIND_FIXED && in->nnz_per_row > EX_MAX_SLOTS) {
    mpg_set_error("%s: a fixed handle of %d slots per row is not served (%d at most)", who, in->nnz_per_row, EX_MAX_SLOTS);
    return MPG_ERR_UNSUPPORTED;
  }
  // the search structure first: a tree that cannot be built refuses the call before anything else is allocated
  ExMeshSrc ms;
  ExGridSrc gs;
  if (n_src > 0 && src_mesh) {
    if ((rc = mpg_k_build_bvh(src_mesh, s, true))) return rc;
    mpg_bvh_view(src_mesh->bvh, ms.b);
    ms.b.sx = src_mesh->bvh.sorted.x.p; ms.b.sy = src_mesh->bvh.sorted.y.p; ms.b.sz = src_mesh->bvh.sorted.z.p;
  } else if (n_src > 0) {
    Pyramid &pyr = src_grid->pyr[src_stagger];
    const PointSet &sp = src_grid->pts[src_stagger];
    if (!pyr.built && (rc = mpg_k_build_pyramid(sp, src_grid->snx[src_stagger], src_grid->sny[src_stagger], pyr, s))) return rc;
    if ((rc = mpg_walk_check<PyrTree>((int64_t)pyr.nx[0] * pyr.ny[0], who))) return rc;
    gs.pyr = mpg_pyr_view(pyr);
    gs.snx = src_grid->snx[src_stagger]; gs.sny = src_grid->sny[src_stagger];
    gs.sx = sp.x.p; gs.sy = sp.y.p; gs.sz = sp.z.p;
  }
  // the candidates: every source, or the unmasked ones (counted, read back with the rows below)
  TmpBuf<long long> nlive;
  if (src_mask && n_src > 0) {
    TmpBuf<int32_t> u;
    if ((rc = u.alloc((size_t)n_src, s)) || (rc = nlive.alloc(1, s))) return rc;
    k_ex_unmasked<<<ex_grid(n_src), 256, 0, s>>>(n_src, src_mask, u.p);
    MPG_HIP(hipGetLastError());
    if ((rc = mpg_sum_i32_i64(u.p, n_src, nlive.p, s))) return rc;
  }
  // pass 1
  TmpBuf<int32_t> flag, pos, list, ids, cnt;
  TmpBuf<double> d2;
  TmpBuf<uint8_t> alive;
  if ((rc = flag.alloc((size_t)n + 1, s)) || (rc = pos.alloc((size_t)n + 1, s))) return rc;
  if (dst_skip) k_ex_flag_skip<<<ex_grid(n + 1), 256, 0, s>>>(I, dst_skip, flag.p);
  else k_ex_flag<<<ex_grid(n + 1), 256, 0, s>>>(I, flag.p);
  MPG_HIP(hipGetLastError());
  if ((rc = mpg_scan_excl_i32(flag.p, pos.p, n + 1, s))) return rc;
  int32_t nu32 = 0;
  long long live = n_src;
  MPG_HIP(hipMemcpyAsync(&nu32, pos.p + n, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (nlive.p) MPG_HIP(hipMemcpyAsync(&live, nlive.p, sizeof(long long), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipStreamSynchronize(s));
  const int K = (int)(live < N ? live : N);
  const int64_t nu = K > 0 ? nu32 : 0;   // without a candidate nothing can be filled, and no tree is walked: its root would be dead
  // pass 2
  if (nu > 0) {
    if ((rc = list.alloc((size_t)nu, s)) || (rc = ids.alloc((size_t)kcap * nu, s)) || (rc = d2.alloc((size_t)kcap * nu, s)) ||
        (rc = cnt.alloc((size_t)nu, s)))
      return rc;
    k_ex_compact<<<ex_grid(n), 256, 0, s>>>(n, flag.p, pos.p, list.p);
    if (src_mask) {
      // the alive bytes of this call's mask, then the walk that never enters a dead subtree
      int64_t level_nodes[MPG_PYR_MAXLEV > MPG_BVH_MAXLEV ? MPG_PYR_MAXLEV : MPG_BVH_MAXLEV];
      int nlev;
      int64_t total;
      if (src_mesh) {
        nlev = ms.b.nlev;
        for (int l = 0; l < nlev; ++l) level_nodes[l] = ms.b.nnodes[l];
        total = ms.b.off[nlev];
      } else {
        nlev = gs.pyr.nlev;
        for (int l = 0; l < nlev; ++l) level_nodes[l] = (int64_t)gs.pyr.nx[l] * gs.pyr.ny[l];
        total = gs.pyr.off[nlev];
      }
      if ((rc = alive.alloc((size_t)total, s))) return rc;
      if ((rc = src_mesh ? ex_alive_build(ms, nlev, level_nodes, src_mask, alive.p, s) : ex_alive_build(gs, nlev, level_nodes, src_mask, alive.p, s)))
        return rc;
      if (src_mesh) ex_launch_knn_masked(kcap, nu, list.p, dst, ms, src_mask, alive.p, idavg, K, ids.p, d2.p, cnt.p, s);
      else ex_launch_knn_masked(kcap, nu, list.p, dst, gs, src_mask, alive.p, idavg, K, ids.p, d2.p, cnt.p, s);
    } else if (src_mesh) ex_launch_knn(kcap, nu, list.p, dst, ms, idavg, K, ids.p, d2.p, cnt.p, s);
    else ex_launch_knn(kcap, nu, list.p, dst, gs, idavg, K, ids.p, d2.p, cnt.p, s);
    MPG_HIP(hipGetLastError());
  }
  out->store_stats[1] = nu;
  out->store_stats[2] = K;
  if (src_mask || dst_skip) out->store_stats[3] = live;   // (the masked call's statistic: its entry point sets it when both are nullptr)
  // pass 3
  if (fixed_out) {
    const int nz = in->nnz_per_row;
    out->kind = MPG_KIND_FIXED;
    out->nnz_per_row = nz;
    out->nnz = in->nnz;
    if ((rc = out->idx.alloc((size_t)nz * (size_t)n))) return rc;
    if (in->w.p && (rc = out->w.alloc((size_t)nz * (size_t)n))) return rc;
    if (n > 0) {
      MPG_HIP(hipMemcpyAsync(out->idx.p, in->idx.p, sizeof(int32_t) * (size_t)nz * (size_t)n, hipMemcpyDeviceToDevice, s));
      if (in->w.p) MPG_HIP(hipMemcpyAsync(out->w.p, in->w.p, sizeof(double) * (size_t)nz * (size_t)n, hipMemcpyDeviceToDevice, s));
    }
    if (nu > 0) {
      const unsigned nb = ex_grid(nu);
      if (kcap == 1) k_ex_fill_fixed<1><<<nb, 256, 0, s>>>(nu, list.p, ids.p, d2.p, cnt.p, idavg, e, nz, n, out->idx.p, out->w.p);
      else if (kcap == 2) k_ex_fill_fixed<2><<<nb, 256, 0, s>>>(nu, list.p, ids.p, d2.p, cnt.p, idavg, e, nz, n, out->idx.p, out->w.p);
      else k_ex_fill_fixed<4><<<nb, 256, 0, s>>>(nu, list.p, ids.p, d2.p, cnt.p, idavg, e, nz, n, out->idx.p, out->w.p);   // (N <= nz <= 4)
      MPG_HIP(hipGetLastError());
    }
    MPG_HIP(hipStreamSynchronize(s));   // the temporaries may go
    return MPG_SUCCESS;
  }
  out->kind = MPG_KIND_CSR;
  out->nnz_per_row = 0;
  if ((rc = out->rowptr.alloc((size_t)n + 1))) return rc;
  TmpBuf<int32_t> len, longest;
  TmpBuf<long long> total;
  if ((rc = len.alloc((size_t)n + 1, s)) || (rc = longest.alloc(1, s)) || (rc = total.alloc(1, s))) return rc;
  MPG_HIP(hipMemsetAsync(longest.p, 0, sizeof(int32_t), s));
  k_ex_rowlen<<<ex_grid(n + 1), 256, 0, s>>>(I, flag.p, pos.p, nu, cnt.p, len.p);
  MPG_HIP(hipGetLastError());
  if ((rc = mpg_sum_i32_i64(len.p, n + 1, total.p, s))) return rc;
  long long nnz = 0;
  MPG_HIP(hipMemcpyAsync(&nnz, total.p, sizeof(long long), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipStreamSynchronize(s));
  if (!knn_nnz_fits(nnz)) {
    mpg_set_error("%s: the CSR output would have %lld entries, more than 2^31 - 2 (rowptr is int32): lower num_src_pnts, or "
                  "extrapolate the parts of the destination separately", who, nnz);
    return MPG_ERR_OVERFLOW;
  }
  if ((rc = mpg_scan_excl_i32(len.p, out->rowptr.p, n + 1, s))) return rc;
  if ((rc = out->col.alloc((size_t)nnz + 1)) || (rc = out->val.alloc((size_t)nnz + 1))) return rc;
  out->nnz = nnz;
  if (n > 0) {
    const unsigned nb = ex_grid(n);
    if (kcap == 1) k_ex_fill_csr<1><<<nb, 256, 0, s>>>(I, flag.p, pos.p, nu, ids.p, d2.p, cnt.p, idavg, e, out->rowptr.p, out->col.p, out->val.p, longest.p);
    else if (kcap == 2) k_ex_fill_csr<2><<<nb, 256, 0, s>>>(I, flag.p, pos.p, nu, ids.p, d2.p, cnt.p, idavg, e, out->rowptr.p, out->col.p, out->val.p, longest.p);
    else if (kcap == 4) k_ex_fill_csr<4><<<nb, 256, 0, s>>>(I, flag.p, pos.p, nu, ids.p, d2.p, cnt.p, idavg, e, out->rowptr.p, out->col.p, out->val.p, longest.p);
    else k_ex_fill_csr<8><<<nb, 256, 0, s>>>(I, flag.p, pos.p, nu, ids.p, d2.p, cnt.p, idavg, e, out->rowptr.p, out->col.p, out->val.p, longest.p);
    MPG_HIP(hipGetLastError());
  }
  int32_t max_row = 0;
  MPG_HIP(hipMemcpyAsync(&max_row, longest.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipStreamSynchronize(s));
  out->max_row = max_row;
  return MPG_SUCCESS;
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_extrapolate() { return (const void *)&k_ex_knn<ExMeshSrc, 1>; }
