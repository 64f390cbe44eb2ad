// Regrid onto a destination that is a plain list of points -- the cells or vertices of a mesh -- written in either memory order of a
// mesh field: [lev][cell] or MPAS file order [cell][lev] (mpg_regrid_to_mesh_dev).  The source is a stack of grid planes, possibly
// pitched.  Serves every fixed-nnz handle: 4 weights (Grid -> Mesh bilinear, Grid -> Grid), 3 (Mesh -> Grid bilinear), 1 (nearest).
//
// The points' indices and weights are staged through LDS once (apply_mesh.h am_stage_fixed) and then held in registers.  Lanes run along
// points, so neighbouring mesh cells gather neighbouring grid points (A / B and D / C of a quad are adjacent pairs in two adjacent grid
// rows); wave w takes levels w, w + 4, ...  Arithmetic and epilogue are those of the typed Regrid (geom.h wsum_fixed, then
// fma(x, scale, offset) rounded once to the destination type): the same bits.
//   [lev][cell]  every level's 64 results go straight out, one run per level
//   [cell][lev]  results are staged in the LDS tile and leave through am_drain_tile, in level chunks when the tile outgrows its cap
//                (apply_mesh.h am_tile_plan)
// No atomics, no allocation, no synchronisation with the host: the call is capturable in a hipGraph from the first call.
#include "apply_mesh.h"

template <typename TS, typename TD, int NNZ, bool LEVF>
__global__ __launch_bounds__(256) void k_apply_to_mesh(const int32_t *__restrict__ idx, const double *__restrict__ w, const TS *__restrict__ src,
                                                       TD *__restrict__ dst, int64_t P, int64_t ld, int nlev, unsigned ntile, int kc, int S,
                                                       double scale, double offset) {
  extern __shared__ double sw[];                       // sw[NNZ][64] | sidx[NNZ][64] | tile[64][S] in the destination type
  int32_t *sidx = (int32_t *)(sw + NNZ * AM_CELLS);
  TD *tile = (TD *)(sidx + NNZ * AM_CELLS);
  const unsigned lin = xcd_remap(blockIdx.x, gridDim.x);
  const unsigned tl = lin % ntile;
  const int f = (int)(lin / ntile);
  const int64_t p0 = (int64_t)tl * AM_CELLS;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  am_stage_fixed<NNZ>(idx, w, P, p0, t, sidx, sw);
  int32_t c[NNZ];
  double ww[NNZ];
#pragma unroll
  for (int q = 0; q < NNZ; ++q) {
    c[q] = sidx[q * AM_CELLS + lane];
    ww[q] = NNZ > 1 ? sw[q * AM_CELLS + lane] : 1.0;
  }
  const bool mapped = c[0] >= 0;
#pragma unroll
  for (int q = 0; q < NNZ; ++q) c[q] = mapped ? c[q] : 0;   // an unmapped point reads source 0 and its result is masked (wsum_fixed)
  const bool in = p0 + lane < P;
  const TS *sf = src + (int64_t)f * nlev * ld;
  TD *df = dst + (int64_t)f * nlev * P;
  const int ncell = (int)min((int64_t)AM_CELLS, P - p0);
  for (int k0 = 0; k0 < nlev; k0 += kc) {
    const int kn = min(kc, nlev - k0);
    const TS *sk = sf + (int64_t)(k0 + wave) * ld;
    auto gather = [&](const TS *plane, double *v) {
#pragma unroll
      for (int q = 0; q < NNZ; ++q) v[q] = (double)plane[c[q]];
    };
    auto put = [&](int k, const double *v) {
      const TD r = (TD)fma(wsum_fixed<NNZ>(ww, v, mapped), scale, offset);
      if (LEVF) tile[lane * S + k] = r;
      else if (in) stream_store_lane(r, df + (int64_t)(k0 + k) * P + p0 + lane, (unsigned)lane * (unsigned)sizeof(TD));
    };
    // two of the wave's levels per step: 2 x NNZ independent gathers in flight
    int k = wave;
    for (; k + 4 < kn; k += 8) {
      double v0[NNZ], v1[NNZ];
      gather(sk, v0);
      gather(sk + 4 * ld, v1);
      put(k, v0);
      put(k + 4, v1);
      sk += 8 * ld;
    }
    if (k < kn) {
      double v0[NNZ];
      gather(sk, v0);
      put(k, v0);
    }
    if (LEVF) {
      am_drain_tile(tile, S, df, p0, k0, ncell, kn, nlev, t, lane);
      if (k0 + kc < nlev) __syncthreads();   // the next chunk overwrites the tile
    }
  }
}

template <typename TS, typename TD, int NNZ>
static int launch_layout(mpg_handle_s *h, const void *src, int64_t ld, int nlev, int nfields, void *dst, bool levf, double scale, double offset,
                         hipStream_t s) {
  const int64_t P = h->n_dst;
  uint64_t ntile;
  int rc = am_grid("mpg_regrid_to_mesh", P, nfields, &ntile);
  if (rc) return rc;
  const TilePlan tp = am_tile_plan(nlev, sizeof(TD), levf, (size_t)NNZ * AM_CELLS * (sizeof(double) + sizeof(int32_t)), 1);
  auto fn = levf ? k_apply_to_mesh<TS, TD, NNZ, true> : k_apply_to_mesh<TS, TD, NNZ, false>;
  if ((rc = am_allow_lds((const void *)fn, tp.lds))) return rc;
  fn<<<(unsigned)(ntile * (uint64_t)nfields), 256, tp.lds, s>>>(h->idx.p, h->w.p, (const TS *)src, (TD *)dst, P, ld, nlev, (unsigned)ntile, tp.kc, tp.S,
                                                                scale, offset);
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

template <typename TS, typename TD>
static int launch_nnz(mpg_handle_s *h, const void *src, int64_t ld, int nlev, int nfields, void *dst, bool levf, double scale, double offset,
                      hipStream_t s) {
  if (h->nnz_per_row == 4) return launch_layout<TS, TD, 4>(h, src, ld, nlev, nfields, dst, levf, scale, offset, s);
  if (h->nnz_per_row == 3) return launch_layout<TS, TD, 3>(h, src, ld, nlev, nfields, dst, levf, scale, offset, s);
  return launch_layout<TS, TD, 1>(h, src, ld, nlev, nfields, dst, levf, scale, offset, s);
}

// ld: the source's level stride in elements (>= n_src; checked by the API entry point, like the handle's kind)
int mpg_k_apply_to_mesh(mpg_handle_s *h, const void *src, int src_type, int64_t ld, int nlev, int nfields, void *dst, int dst_type, int layout,
                        double scale, double offset, hipStream_t s) {
  if (h->n_dst == 0 || nlev == 0 || nfields == 0) return MPG_SUCCESS;
  // nothing mapped: nlev * nfields planes of n_dst points, whichever the layout
  if (h->n_src == 0) return am_no_sources("mpg_regrid_to_mesh", dst, dst_type, h->n_dst, (int64_t)nlev * nfields, h->n_dst, offset, s);
  const bool levf = layout == MPG_LAYOUT_LEV_FAST && nlev > 1;   // (a single level is the same memory in both layouts)
  return mpg_dispatch_types(src_type, dst_type, [&](auto ts, auto td) {
    return launch_nnz<decltype(ts), decltype(td)>(h, src, ld, nlev, nfields, dst, levf, scale, offset, s);
  });
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_apply_to_mesh() { return (const void *)&k_apply_to_mesh<float, float, 4, true>; }
