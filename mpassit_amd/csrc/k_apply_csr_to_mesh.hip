// Regrid of a CSR handle onto a destination that is a plain list of points -- the cells of a mesh -- written in either memory order of a
// mesh field: [lev][cell] or MPAS file order [cell][lev] (mpg_regrid_csr_to_mesh_dev).  The source is a stack of grid planes, possibly
// pitched; any CSR handle is served (conservative Grid -> Mesh, conservative Mesh -> Grid, from-weights).
//
// The entries of the block's 64 rows are staged through LDS as one run (apply_mesh.h CsrRun) and every wave walks it for its own levels,
// lanes along rows, wave w on levels w, w + 4, ...: index and weight traffic is paid once per workgroup, not once per level.  A wave
// carries CM_LB levels at a time (CM_LB independent fma chains and gathers in flight per lane); a run longer than one chunk is staged
// again for every batch of 4 * CM_LB levels.  A row's value is k_apply_generic_t<..., NNZ = 0, ...>'s expression -- acc =
// fma(val[q], src, acc) from 0.0 in stored order, whatever chunk an entry arrives in -- then fma(acc, scale, offset) rounded once to the
// destination type: the same bits.
//   [lev][cell]  every level's 64 results go straight out, one run per level
//   [cell][lev]  the LDS tile and am_drain_tile, as in k_apply_to_mesh, its level chunks above the tile cap included
// No atomics, no allocation, no synchronisation with the host: the call is capturable in a hipGraph from the first call.
#include "apply_mesh.h"

#define CM_LB 4                       // levels a wave carries at a time
#define CM_RP (AM_CELLS + 4)          // row pointers of the block, padded so that the tile behind them stays 8-byte aligned

template <typename TS, typename TD, bool LEVF>
__global__ __launch_bounds__(256) void k_apply_csr_to_mesh(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                           const double *__restrict__ val, const TS *__restrict__ src, TD *__restrict__ dst,
                                                           int64_t P, int64_t ld, int nlev, unsigned ntile, int kc, int S, double scale,
                                                           double offset) {
  extern __shared__ double sval[];                     // sval[AM_CHUNK] | scol[AM_CHUNK] | srp[CM_RP] | tile[64][S] in the destination type
  int32_t *scol = (int32_t *)(sval + AM_CHUNK);
  int32_t *srp = scol + AM_CHUNK;
  TD *tile = (TD *)(srp + CM_RP);
  const unsigned lin = xcd_remap(blockIdx.x, gridDim.x);
  const unsigned tl = lin % ntile;
  const int f = (int)(lin / ntile);
  const int64_t p0 = (int64_t)tl * AM_CELLS;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const CsrRun run = am_csr_run(rowptr, col, val, P, p0, t, srp, scol, sval);
  const int rb = srp[lane], re = srp[lane + 1];
  const bool in = p0 + lane < P;
  const TS *sf = src + (int64_t)f * nlev * ld;
  TD *df = dst + (int64_t)f * nlev * P;
  const int ncell = (int)min((int64_t)AM_CELLS, P - p0);
  for (int k0 = 0; k0 < nlev; k0 += kc) {
    const int kn = min(kc, nlev - k0);
    for (int kb = 0; kb < kn; kb += 4 * CM_LB) {
      double acc[CM_LB];
      const TS *pl[CM_LB];
#pragma unroll
      for (int j = 0; j < CM_LB; ++j) {
        const int k = kb + wave + 4 * j;
        acc[j] = 0.0;
        pl[j] = sf + (int64_t)(k0 + (k < kn ? k : 0)) * ld;   // a level slot past the chunk gathers level k0 and stores nothing
      }
      for (int ch = 0; ch < run.nchunk; ++ch) {
        const int qa = run.enter(ch);
        const int b = max(rb, qa), e = min(re - qa, AM_CHUNK) + qa;
        for (int q = b; q < e; ++q) {
          const int32_t c = scol[q - qa];
          const double w = sval[q - qa];
#pragma unroll
          for (int j = 0; j < CM_LB; ++j) acc[j] = fma(w, (double)pl[j][c], acc[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < CM_LB; ++j) {
        const int k = kb + wave + 4 * j;
        if (k < kn) {
          const TD r = (TD)fma(acc[j], scale, offset);
          if (LEVF) tile[lane * S + k] = r;
          else if (in) stream_store_lane(r, df + (int64_t)(k0 + k) * P + p0 + lane, (unsigned)lane * (unsigned)sizeof(TD));
        }
      }
    }
    if (LEVF) {
      am_drain_tile(tile, S, df, p0, k0, ncell, kn, nlev, t, lane);
      if (k0 + kc < nlev) __syncthreads();   // the next chunk overwrites the tile
    }
  }
}

template <typename TS, typename TD>
static int launch_layout(mpg_handle_s *h, const void *src, int64_t ld, int nlev, int nfields, void *dst, bool levf, double scale, double offset,
                         hipStream_t s) {
  const int64_t P = h->n_dst;
  uint64_t ntile;
  int rc = am_grid("mpg_regrid_csr_to_mesh", P, nfields, &ntile);
  if (rc) return rc;
  const TilePlan tp = am_tile_plan(nlev, sizeof(TD), levf, (size_t)AM_CHUNK * (sizeof(double) + sizeof(int32_t)) + CM_RP * sizeof(int32_t), 1);
  auto fn = levf ? k_apply_csr_to_mesh<TS, TD, true> : k_apply_csr_to_mesh<TS, TD, false>;
  if ((rc = am_allow_lds((const void *)fn, tp.lds))) return rc;
  fn<<<(unsigned)(ntile * (uint64_t)nfields), 256, tp.lds, s>>>(h->rowptr.p, h->col.p, h->val.p, (const TS *)src, (TD *)dst, P, ld, nlev, (unsigned)ntile,
                                                                tp.kc, tp.S, scale, offset);
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

// ld: the source's level stride in elements (>= n_src; checked by the API entry point, like the handle's kind)
int mpg_k_apply_csr_to_mesh(mpg_handle_s *h, const void *src, int src_type, int64_t ld, int nlev, int nfields, void *dst, int dst_type, int layout,
                            double scale, double offset, hipStream_t s) {
  if (h->n_dst == 0 || nlev == 0 || nfields == 0) return MPG_SUCCESS;
  const bool levf = layout == MPG_LAYOUT_LEV_FAST && nlev > 1;   // (a single level is the same memory in both layouts)
  return mpg_dispatch_types(src_type, dst_type, [&](auto ts, auto td) {
    return launch_layout<decltype(ts), decltype(td)>(h, src, ld, nlev, nfields, dst, levf, scale, offset, s);
  });
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_apply_csr_to_mesh() { return (const void *)&k_apply_csr_to_mesh<float, float, true>; }
