// Nearest destination to source (mpg_regrid_store_nearest_dtos): every source point goes to the ONE destination point nearest to it, and
// row d of the CSR handle lists the sources that chose d (include/mpassit_amd.h states the contract).  The one Store that scatters; three
// passes, none of which lets an arrival order decide a stored byte:
//
//   pass 1  k_dtos_search<Dst>   one lane per source: dtos_nearest (dtos.h = knn_search with KBest<1>) through the DESTINATION's tree -- the
//           [_masked]            mesh's site BVH built whole (ExMeshSrc) or a stagger's point pyramid (ExGridSrc), knn_src.h -- writes
//                                nearest[s], -1 for a masked source.  With a destination mask the `alive` bytes of knn_mask.h are built
//                                per call (k_dtos_alive_*), and with every destination masked nearest is all -1 without a walk.
//           The order of the visit.  The sources are the queries, so a wave walks few subtrees when its 64 lanes are neighbours.  A
//           grid's ids are: lanes s .. s + 63 are a strip of one row (or of two), id order is taken as it is.  A mesh's cell, vertex and
//           edge numbers promise nothing -- MPAS meshes are numbered by their generator's own order -- so lane u takes the source
//           order[u] of a Morton sort of the source points (mpg_k_morton + the radix sort, as the site BVH's build does), and still
//           writes nearest[s] by id: the order changes which lanes share a wave, never a result.
//   pass 2  k_dtos_count         cnt[d] += the sources that chose d: integer atomics, aggregated per run of equal neighbours in a wave
//                                (fine onto coarse sends hundreds of neighbouring lanes to one counter: a wave of one run costs ONE
//                                atomic).  An integer sum is the same in any order.  mpg_sum_i32_i64(cnt) is read back and checked
//                                against the mapped sources' count (the scan of the flags), mpg_scan_excl_i32(cnt) = rowptr.
//           k_dtos_keys          key[pos[s]] = dst << 32 | s for the mapped sources, compacted in ascending s; the stable device-wide
//                                radix sort of the keys carries s along: the sorted values ARE col, row d's entries in ascending source
//                                id.  k_dtos_rowstat: the longest row (an integer maximum) and the non-empty rows (an integer count).
//   pass 3  k_dtos_values        one lane per entry: dtos_value (dtos.h) of the length of the entry's row (the sorted key's high word).
#include "geom.h"
#include "dtos.h"
#include "knn_src.h"
#include "mpg_internal.h"

static inline unsigned dt_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

template <class Dst>
__global__ __launch_bounds__(256) void k_dtos_alive_leaf(Dst dst, int64_t leaves, const uint8_t *__restrict__ mask, uint8_t *__restrict__ alive) {
  const int64_t node = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (node < leaves) alive[dst.tree().v.off[0] + node] = dst.leaf_alive((int)node, mask);
}
template <class Dst>
__global__ __launch_bounds__(256) void k_dtos_alive_up(Dst dst, int lev, int64_t nodes, uint8_t *alive) {
  const int64_t node = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (node < nodes) alive[dst.tree().v.off[lev] + node] = alive_parent(dst.tree(), lev, (int)node, alive);
}

// order: the visiting order of the sources (nullptr: by id); src_mask: nullptr = none
template <class Dst>
__global__ __launch_bounds__(256) void k_dtos_search(int64_t n, const int32_t *__restrict__ order, const double *__restrict__ px,
                                                     const double *__restrict__ py, const double *__restrict__ pz,
                                                     const uint8_t *__restrict__ src_mask, Dst dst, int32_t *__restrict__ nearest) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= n) return;
  const int64_t p = order ? (int64_t)order[u] : u;
  if (src_mask && src_mask[p]) {
    nearest[p] = -1;
    return;
  }
  const double X = px[p], Y = py[p], Z = pz[p];
  nearest[p] = dtos_nearest(
      dst.tree(), [&](const double *bx) { return boxdist2_nofma(X, Y, Z, bx); }, [&](int node, auto f) { dst.leaf(node, X, Y, Z, f); });
}

// ... over the unmasked destinations alone, through the alive bytes
template <class Dst>
__global__ __launch_bounds__(256) void k_dtos_search_masked(int64_t n, const int32_t *__restrict__ order, const double *__restrict__ px,
                                                            const double *__restrict__ py, const double *__restrict__ pz,
                                                            const uint8_t *__restrict__ src_mask, Dst dst, const uint8_t *__restrict__ dst_mask,
                                                            const uint8_t *__restrict__ alive, int32_t *__restrict__ nearest) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= n) return;
  const int64_t p = order ? (int64_t)order[u] : u;
  if (src_mask && src_mask[p]) {
    nearest[p] = -1;
    return;
  }
  const double X = px[p], Y = py[p], Z = pz[p];
  nearest[p] = dtos_nearest_masked(
      dst.tree(), alive, [&](const double *bx) { return boxdist2_nofma(X, Y, Z, bx); },
      [&](int node, auto f) { dst.leaf_masked(node, X, Y, Z, dst_mask, f); });
}

// u[d] = 1 for an unmasked destination (summed: the candidates' count)
__global__ __launch_bounds__(256) void k_dtos_unmasked(int64_t n, const uint8_t *__restrict__ mask, int32_t *__restrict__ u) {
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (d < n) u[d] = mask[d] == 0;
}

__global__ __launch_bounds__(256) void k_dtos_none(int64_t n, int32_t *__restrict__ nearest) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s < n) nearest[s] = -1;
}

// flag[s] = the source is mapped (flag[n] = 0: the scan of n + 1 flags ends in the count); cnt[d] += the sources of d.  Every lane of a
// wave stays in the kernel to its end: the shuffle and the ballot read all 64.  A run of equal neighbours adds its length once, by its
// first lane; the next run's first lane is the next set bit of `heads`.
__global__ __launch_bounds__(256) void k_dtos_count(int64_t n, int64_t n_dst, const int32_t *__restrict__ nearest, int32_t *__restrict__ flag,
                                                    int32_t *__restrict__ cnt) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int32_t d = s < n ? nearest[s] : -1;
  if (d >= n_dst) d = -1;   // (cannot happen: ids come from the destination's own tree; a counter outside cnt is never touched)
  if (s <= n) flag[s] = d >= 0;
  const int32_t prev = __shfl_up(d, 1);
  const bool head = lane == 0 || prev != d;
  const unsigned long long heads = __ballot(head);
  if (head && d >= 0) {
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    const int run = above ? __ffsll(above) : 64 - lane;
    atomicAdd(&cnt[d], run);   // (an integer count: the order of the adds does not matter)
  }
}

__global__ __launch_bounds__(256) void k_dtos_keys(int64_t n, const int32_t *__restrict__ nearest, const int32_t *__restrict__ flag,
                                                   const int32_t *__restrict__ pos, unsigned long long *__restrict__ key,
                                                   int32_t *__restrict__ val) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= n || !flag[s]) return;
  const int64_t at = pos[s];
  key[at] = ((unsigned long long)(uint32_t)nearest[s] << 32) | (unsigned long long)(uint32_t)s;
  val[at] = (int32_t)s;
}

// stat[0] = the longest row (maximum), stat[1] = the non-empty rows (count): integers, any order
__global__ __launch_bounds__(256) void k_dtos_rowstat(int64_t n_dst, const int32_t *__restrict__ cnt, int32_t *__restrict__ stat) {
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int32_t len = d < n_dst ? cnt[d] : 0;
  int32_t some = len > 0;
  for (int o = 32; o > 0; o >>= 1) {
    len = max(len, __shfl_down(len, o));
    some += __shfl_down(some, o);
  }
  if ((threadIdx.x & 63) == 0 && some > 0) {
    atomicMax(&stat[0], len);
    atomicAdd(&stat[1], some);
  }
}

__global__ __launch_bounds__(256) void k_dtos_values(int64_t nnz, int norm, const unsigned long long *__restrict__ key,
                                                     const int32_t *__restrict__ cnt, double *__restrict__ val) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q < nnz) val[q] = dtos_value(norm, cnt[(int64_t)(key[q] >> 32)]);
}

template <class Dst>
static int dt_alive_build(const Dst &dst, int nlev, const int64_t *level_nodes, const uint8_t *mask, uint8_t *alive, hipStream_t s) {
  k_dtos_alive_leaf<Dst><<<dt_grid(level_nodes[0]), 256, 0, s>>>(dst, level_nodes[0], mask, alive);
  for (int lev = 1; lev < nlev; ++lev) k_dtos_alive_up<Dst><<<dt_grid(level_nodes[lev]), 256, 0, s>>>(dst, lev, level_nodes[lev], alive);
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

template <class Dst>
static int dt_search(const Dst &dst, int nlev, const int64_t *level_nodes, int64_t total_nodes, const PointSet &src, int64_t n,
                     const int32_t *order, const uint8_t *src_mask, const uint8_t *dst_mask, int32_t *nearest, hipStream_t s) {
  int rc;
  if (!dst_mask) {
    k_dtos_search<Dst><<<dt_grid(n), 256, 0, s>>>(n, order, src.x.p, src.y.p, src.z.p, src_mask, dst, nearest);
    MPG_HIP(hipGetLastError());
    return MPG_SUCCESS;
  }
  TmpBuf<uint8_t> alive;
  if ((rc = alive.alloc((size_t)total_nodes, s))) return rc;
  if ((rc = dt_alive_build(dst, nlev, level_nodes, dst_mask, alive.p, s))) return rc;
  k_dtos_search_masked<Dst><<<dt_grid(n), 256, 0, s>>>(n, order, src.x.p, src.y.p, src.z.p, src_mask, dst, dst_mask, alive.p, nearest);
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;   // (alive goes back to the stream's pool: its next user on this stream is ordered behind the search)
}

int mpg_k_store_dtos(const PointSet &src, int64_t n_src, bool src_morton, mpg_mesh_s *dst_mesh, mpg_grid_s *dst_grid, int dst_stagger, int norm,
                     const uint8_t *src_mask, const uint8_t *dst_mask, mpg_handle_s *h, hipStream_t s) {
  const char *who = "mpg_regrid_store_nearest_dtos";
  int rc;
  const int64_t n_dst = h->n_dst;
  // the searched set's tree first: one that cannot be built refuses the call before anything else is allocated
  ExMeshSrc md;
  ExGridSrc gd;
  int64_t level_nodes[MPG_PYR_MAXLEV > MPG_BVH_MAXLEV ? MPG_PYR_MAXLEV : MPG_BVH_MAXLEV];
  int nlev = 0;
  int64_t total_nodes = 0;
  if (n_src > 0 && n_dst > 0 && dst_mesh) {
    if ((rc = mpg_k_build_bvh(dst_mesh, s, true))) return rc;
    mpg_bvh_view(dst_mesh->bvh, md.b);
    md.b.sx = dst_mesh->bvh.sorted.x.p; md.b.sy = dst_mesh->bvh.sorted.y.p; md.b.sz = dst_mesh->bvh.sorted.z.p;
    nlev = md.b.nlev;
    for (int l = 0; l < nlev; ++l) level_nodes[l] = md.b.nnodes[l];
    total_nodes = md.b.off[nlev];
  } else if (n_src > 0 && n_dst > 0) {
    Pyramid &pyr = dst_grid->pyr[dst_stagger];
    const PointSet &dp = dst_grid->pts[dst_stagger];
    if (!pyr.built && (rc = mpg_k_build_pyramid(dp, dst_grid->snx[dst_stagger], dst_grid->sny[dst_stagger], pyr, s))) return rc;
    if ((rc = mpg_walk_check<PyrTree>((int64_t)pyr.nx[0] * pyr.ny[0], who))) return rc;
    gd.pyr = mpg_pyr_view(pyr);
    gd.snx = dst_grid->snx[dst_stagger]; gd.sny = dst_grid->sny[dst_stagger];
    gd.sx = dp.x.p; gd.sy = dp.y.p; gd.sz = dp.z.p;
    nlev = gd.pyr.nlev;
    for (int l = 0; l < nlev; ++l) level_nodes[l] = (int64_t)gd.pyr.nx[l] * gd.pyr.ny[l];
    total_nodes = gd.pyr.off[nlev];
  }
  h->kind = MPG_KIND_CSR;
  h->nnz_per_row = 0;
  h->has_src_nearest = true;
  if ((rc = h->src_nearest.alloc((size_t)n_src)) || (rc = h->rowptr.alloc((size_t)n_dst + 1))) return rc;
  TmpBuf<int32_t> flag, pos, cnt, stat, order, sval;
  TmpBuf<long long> sums;   // [0] the unmasked destinations, [1] the sum of cnt
  TmpBuf<unsigned long long> key, skey;
  if ((rc = sums.alloc(2, s))) return rc;
  long long live = n_dst;
  // pass 1
  if (n_src > 0) {
    bool search = n_dst > 0;
    if (search && dst_mask) {
      // every destination masked: no candidate, and no tree is walked (its root would be dead)
      TmpBuf<int32_t> u;
      if ((rc = u.alloc((size_t)n_dst, s))) return rc;
      k_dtos_unmasked<<<dt_grid(n_dst), 256, 0, s>>>(n_dst, dst_mask, u.p);
      MPG_HIP(hipGetLastError());
      if ((rc = mpg_sum_i32_i64(u.p, n_dst, sums.p, s))) return rc;
      MPG_HIP(hipMemcpyAsync(&live, sums.p, sizeof(long long), hipMemcpyDeviceToHost, s));
      MPG_HIP(hipStreamSynchronize(s));
      search = live > 0;
    }
    if (search) {
      if (src_morton) {
        if ((rc = key.alloc((size_t)n_src, s)) || (rc = skey.alloc((size_t)n_src, s)) || (rc = sval.alloc((size_t)n_src, s)) ||
            (rc = order.alloc((size_t)n_src, s)))
          return rc;
        if ((rc = mpg_k_morton(n_src, src.x.p, src.y.p, src.z.p, key.p, sval.p, 0, s))) return rc;
        if ((rc = mpg_sort_pairs_u64_i32(key.p, skey.p, sval.p, order.p, n_src, s))) return rc;
      }
      if ((rc = dst_mesh ? dt_search(md, nlev, level_nodes, total_nodes, src, n_src, order.p, src_mask, dst_mask, h->src_nearest.p, s)
                         : dt_search(gd, nlev, level_nodes, total_nodes, src, n_src, order.p, src_mask, dst_mask, h->src_nearest.p, s)))
        return rc;
    } else {
      k_dtos_none<<<dt_grid(n_src), 256, 0, s>>>(n_src, h->src_nearest.p);
      MPG_HIP(hipGetLastError());
    }
  }
  // pass 2
  if ((rc = flag.alloc((size_t)n_src + 1, s)) || (rc = pos.alloc((size_t)n_src + 1, s)) || (rc = cnt.alloc((size_t)n_dst + 1, s)) ||
      (rc = stat.alloc(2, s)))
    return rc;
  MPG_HIP(hipMemsetAsync(cnt.p, 0, sizeof(int32_t) * ((size_t)n_dst + 1), s));
  MPG_HIP(hipMemsetAsync(stat.p, 0, sizeof(int32_t) * 2, s));
  k_dtos_count<<<dt_grid(n_src + 1), 256, 0, s>>>(n_src, n_dst, h->src_nearest.p, flag.p, cnt.p);
  MPG_HIP(hipGetLastError());
  if ((rc = mpg_scan_excl_i32(flag.p, pos.p, n_src + 1, s))) return rc;
  if ((rc = mpg_sum_i32_i64(cnt.p, n_dst + 1, sums.p + 1, s))) return rc;
  if ((rc = mpg_scan_excl_i32(cnt.p, h->rowptr.p, n_dst + 1, s))) return rc;
  if (n_dst > 0) k_dtos_rowstat<<<dt_grid(n_dst), 256, 0, s>>>(n_dst, cnt.p, stat.p);
  MPG_HIP(hipGetLastError());
  int32_t mapped = 0, st[2] = {0, 0};
  long long total = 0;
  MPG_HIP(hipMemcpyAsync(&mapped, pos.p + n_src, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipMemcpyAsync(&total, sums.p + 1, sizeof(long long), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipMemcpyAsync(st, stat.p, sizeof(st), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipStreamSynchronize(s));
  if (total != (long long)mapped || !knn_nnz_fits(total)) {
    mpg_set_error("%s: the rows count %lld entries, the mapped sources are %d (an internal error: report it with the two point sets)", who, total,
                  (int)mapped);
    return MPG_ERR_OVERFLOW;
  }
  const int64_t nnz = mapped;
  if ((rc = h->col.alloc((size_t)nnz + 1)) || (rc = h->val.alloc((size_t)nnz + 1))) return rc;
  h->nnz = nnz;
  h->max_row = st[0];
  h->store_stats[1] = nnz;
  h->store_stats[2] = st[1];
  h->store_stats[3] = st[0];
  if (nnz > 0) {
    if ((rc = key.alloc((size_t)nnz, s)) || (rc = skey.alloc((size_t)nnz, s)) || (rc = sval.alloc((size_t)nnz, s))) return rc;
    k_dtos_keys<<<dt_grid(n_src), 256, 0, s>>>(n_src, h->src_nearest.p, flag.p, pos.p, key.p, sval.p);
    MPG_HIP(hipGetLastError());
    if ((rc = mpg_sort_pairs_u64_i32(key.p, skey.p, sval.p, h->col.p, nnz, s))) return rc;
    // pass 3
    k_dtos_values<<<dt_grid(nnz), 256, 0, s>>>(nnz, norm, skey.p, cnt.p, h->val.p);
    MPG_HIP(hipGetLastError());
  }
  MPG_HIP(hipStreamSynchronize(s));   // the temporaries may go
  return MPG_SUCCESS;
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_store_dtos() { return (const void *)&k_dtos_search<ExMeshSrc>; }
