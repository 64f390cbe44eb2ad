// Regrid of a CSR handle onto a destination that is a plain list of points -- the cells of a mesh -- written in either memory order of a
// mesh field: [lev][cell] or MPAS file order [cell][lev] (mpg_regrid_csr_to_mesh_dev).  The CSR sibling of k_apply_to_mesh.hip: the source
// is a stack of grid planes, possibly pitched; any CSR handle is served (conservative Grid -> Mesh, conservative Mesh -> Grid, from-weights).
//
// One workgroup owns 64 consecutive rows and all levels.  The entries of those rows are ONE contiguous run [rowptr[c0], rowptr[c0 + 64])
// of col / val: the workgroup loads the run coalesced into LDS -- once when it fits CM_CHUNK entries, else chunk by chunk -- and every
// wave walks it for its own levels, lanes along rows, wave w on levels w, w + 4, ...: index and weight traffic is paid once per
// workgroup, not once per level.  A wave carries CM_LB levels at a time (CM_LB independent fma chains and gathers in flight per lane);
// a run longer than one chunk is staged again for every batch of 4 * CM_LB levels (from L2), so that a row's accumulators never
// leave registers.  A row's value is k_apply_generic_t<..., NNZ = 0, ...>'s expression -- acc = fma(val[q], src, acc) from 0.0 in stored
// order, whatever chunk an entry arrives in -- then fma(acc, scale, offset) rounded once to the destination type: the same bits.
//   [lev][cell]  every level's 64 results go straight out, one run per level
//   [cell][lev]  the LDS tile + stream_store_lane path of k_apply_to_mesh, its level chunks above 64 KB of tile included
// No atomics, no allocation, no synchronisation with the host: the call is capturable in a hipGraph from the first call.
#include <algorithm>

#include "geom.h"
#include "mpg_internal.h"

#define CM_CELLS 64
#define CM_CHUNK 1024                 // entries of the run resident in LDS: 12 KB (64 rows of a mesh as fine as its grid hold 200-600)
#define CM_LB 4                       // levels a wave carries at a time
#define CM_RP (CM_CELLS + 4)          // row pointers of the block, padded so that the tile behind them stays 8-byte aligned
#define CM_TILE_BYTES (64 * 1024)

template <typename TS, typename TD, bool LEVF>
__global__ __launch_bounds__(256) void k_apply_csr_to_mesh(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                           const double *__restrict__ val, const TS *__restrict__ src, TD *__restrict__ dst,
                                                           int64_t P, int64_t ld, int nlev, unsigned ntile, int kc, int S, double scale,
                                                           double offset) {
  extern __shared__ double sval[];                     // sval[CM_CHUNK] | scol[CM_CHUNK] | srp[CM_RP] | tile[64][S] in the destination type
  int32_t *scol = (int32_t *)(sval + CM_CHUNK);
  int32_t *srp = scol + CM_CHUNK;
  TD *tile = (TD *)(srp + CM_RP);
  const unsigned lin = xcd_remap(blockIdx.x, gridDim.x);
  const unsigned tl = lin % ntile;
  const int f = (int)(lin / ntile);
  const int64_t p0 = (int64_t)tl * CM_CELLS;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t <= CM_CELLS) srp[t] = rowptr[min(p0 + t, P)];   // rows past the end are empty
  __syncthreads();
  const int r0 = srp[0], r1 = srp[CM_CELLS];
  const int rb = srp[lane], re = srp[lane + 1];
  const int nchunk = (int)(((int64_t)r1 - r0 + CM_CHUNK - 1) / CM_CHUNK);
  auto stage = [&](int qa) {
    const int n = min(CM_CHUNK, r1 - qa);
    for (int i = t; i < n; i += 256) {
      scol[i] = col[qa + i];
      sval[i] = val[qa + i];
    }
  };
  if (nchunk == 1) {
    stage(r0);
    __syncthreads();
  }
  const bool in = p0 + lane < P;
  const TS *sf = src + (int64_t)f * nlev * ld;
  TD *df = dst + (int64_t)f * nlev * P;
  const int ncell = (int)min((int64_t)CM_CELLS, P - p0);
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
      for (int ch = 0; ch < nchunk; ++ch) {
        const int qa = r0 + ch * CM_CHUNK;   // (ch * CM_CHUNK < r1 - r0)
        if (nchunk > 1) {
          __syncthreads();   // the chunk before has been walked by every wave
          stage(qa);
          __syncthreads();
        }
        const int b = max(rb, qa), e = min(re - qa, CM_CHUNK) + qa;
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
      __syncthreads();
      // the chunk's results in destination order: element e = cell (e / kn), level k0 + (e % kn); with kn == nlev one contiguous run
      const int total = ncell * kn;
      const int dc = 256 / kn, dk = 256 % kn;
      int cc = t / kn, kk = t % kn;
      TD *out = df + p0 * nlev + k0;
      const bool run = kn == nlev;   // workgroup-uniform
      for (int e = t; e < total; e += 256) {
        TD *a = out + (int64_t)cc * nlev + kk;
        const TD r = tile[cc * S + kk];
        if (run) stream_store_lane(r, a, (unsigned)lane * (unsigned)sizeof(TD));
        else *a = r;
        cc += dc;
        kk += dk;
        if (kk >= kn) {
          kk -= kn;
          ++cc;
        }
      }
      if (k0 + kc < nlev) __syncthreads();   // the next chunk overwrites the tile
    }
  }
}

template <typename TS, typename TD>
static int launch_layout(mpg_handle_s *h, const void *src, int64_t ld, int nlev, int nfields, void *dst, bool levf, double scale, double offset,
                         hipStream_t s) {
  const int64_t P = h->n_dst;
  const uint64_t ntile = (uint64_t)((P + CM_CELLS - 1) / CM_CELLS);
  if (ntile * (uint64_t)nfields > 0x7fffffffull) {
    mpg_set_error("mpg_regrid_csr_to_mesh: %lld points x %d fields exceed one launch", (long long)P, nfields);
    return MPG_ERR_OVERFLOW;
  }
  int kc = nlev, S = 0;
  size_t lds = (size_t)CM_CHUNK * (sizeof(double) + sizeof(int32_t)) + CM_RP * sizeof(int32_t);
  if (levf) {
    // all levels in one tile when they fit, else chunks of a multiple of 32 levels; row stride odd (k_apply_to_mesh.hip)
    if ((size_t)CM_CELLS * (size_t)(nlev | 1) * sizeof(TD) > CM_TILE_BYTES) kc = (int)(CM_TILE_BYTES / (CM_CELLS * sizeof(TD)) - 1) / 32 * 32;
    S = kc | 1;
    lds += (size_t)CM_CELLS * (size_t)S * sizeof(TD);
  }
  auto fn = levf ? k_apply_csr_to_mesh<TS, TD, true> : k_apply_csr_to_mesh<TS, TD, false>;
  if (lds > 48 * 1024) MPG_HIP(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  fn<<<(unsigned)(ntile * (uint64_t)nfields), 256, lds, s>>>(h->rowptr.p, h->col.p, h->val.p, (const TS *)src, (TD *)dst, P, ld, nlev, (unsigned)ntile, kc,
                                                             S, scale, offset);
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

// ld: the source's level stride in elements (>= n_src; checked by the API entry point, like the handle's kind)
int mpg_k_apply_csr_to_mesh(mpg_handle_s *h, const void *src, int src_type, int64_t ld, int nlev, int nfields, void *dst, int dst_type, int layout,
                            double scale, double offset, hipStream_t s) {
  if (h->n_dst == 0 || nlev == 0 || nfields == 0) return MPG_SUCCESS;
  const int sf32 = src_type & MPG_TYPE_F32, df32 = dst_type & MPG_TYPE_F32;
  const bool levf = layout == MPG_LAYOUT_LEV_FAST && nlev > 1;   // (a single level is the same memory in both layouts)
  if (sf32 && df32) return launch_layout<float, float>(h, src, ld, nlev, nfields, dst, levf, scale, offset, s);
  if (sf32) return launch_layout<float, double>(h, src, ld, nlev, nfields, dst, levf, scale, offset, s);
  if (df32) return launch_layout<double, float>(h, src, ld, nlev, nfields, dst, levf, scale, offset, s);
  return launch_layout<double, double>(h, src, ld, nlev, nfields, dst, levf, scale, offset, s);
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_apply_csr_to_mesh() { return (const void *)&k_apply_csr_to_mesh<float, float, true>; }
