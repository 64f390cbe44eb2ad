// What the four mesh-order Regrid kernels (k_apply_to_mesh / k_apply_csr_to_mesh / k_apply_rows / k_apply_csr_rows.hip) and the wind
// kernels on two fixed handles (k_wind_pair.hip) and on two CSR handles (k_wind_csr.hip) share: the staging of a block's indices and weights or of its CSR run through LDS, the
// (point, level) cursor along a block's [cell][lev] run, the drain of the [cell][lev] result tile, and on the host the tile plan, the
// launch grid, the path of a handle without sources and the (src_type, dst_type) dispatch.  One workgroup of 256 threads owns AM_CELLS
// consecutive destination points and all levels in every one of the six; the LDS arrays are declared by the kernels (dynamic or static)
// and handed in as pointers; the main loops stay there.  k_wind_vector.hip is the seventh: it stages its run through CsrRunN, which stands
// beside CsrRun and changes nothing the six compile.
#pragma once
#include <algorithm>

#include "geom.h"
#include "mpg_internal.h"

#define AM_CELLS 64                  // destination points (rows) of a workgroup
#define AM_CHUNK 1024                // entries of a block's CSR run resident in LDS: 12 KB (64 rows of a mesh as fine as its grid hold 200-600)
#define AM_TILE_BYTES (64 * 1024)    // cap of the [cell][lev] result tile

// ---- device ---------------------------------------------------------------------------------------------------------------------------
// Fixed-nnz handle: idx / w of the block's points into sidx[NNZ][64] / sw[NNZ][64], -1 for a point past P (sw is not written for NNZ 1)
template <int NNZ>
__device__ __forceinline__ void am_stage_fixed(const int32_t *__restrict__ idx, const double *__restrict__ w, int64_t P, int64_t p0, int t,
                                               int32_t *sidx, double *sw) {
  if (t < NNZ * AM_CELLS) {
    const int pt = t & 63, q = t >> 6;
    const bool in = p0 + pt < P;
    const int64_t p = in ? p0 + pt : 0;
    sidx[q * AM_CELLS + pt] = in ? idx[q * P + p] : -1;
    if (NNZ > 1) sw[q * AM_CELLS + pt] = w[q * P + p];
  }
  __syncthreads();
}

// CSR handle: the entries of the block's 64 rows are ONE contiguous run [r0, r1) of col / val.  It is loaded coalesced into scol / sval:
// once, by am_csr_run, when it fits AM_CHUNK entries (nchunk == 1), else chunk by chunk by enter() -- again for every batch of results
// the kernel carries in registers (from L2), so that a row's accumulator never leaves them.  nchunk is workgroup-uniform and so are
// the barriers of enter(): every thread of the workgroup has to call it for every chunk, in the same order.
struct CsrRun {
  const int32_t *col;
  const double *val;
  int32_t *scol;
  double *sval;
  int t, r0, r1, nchunk;
  __device__ __forceinline__ void stage(int qa) const {
    const int n = min(AM_CHUNK, r1 - qa);
    for (int i = t; i < n; i += 256) {
      scol[i] = col[qa + i];
      sval[i] = val[qa + i];
    }
  }
  // chunk ch (ch * AM_CHUNK < r1 - r0) is resident on return; its first entry qa: entry q of the run is scol / sval[q - qa]
  __device__ __forceinline__ int enter(int ch) const {
    const int qa = r0 + ch * AM_CHUNK;
    if (nchunk > 1) {
      __syncthreads();   // the chunk before has been walked by every wave
      stage(qa);
      __syncthreads();
    }
    return qa;
  }
};
// srp[0 .. 64]: the block's row pointers (row i of the block is [srp[i], srp[i + 1])), valid on return
__device__ __forceinline__ CsrRun am_csr_run(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const double *__restrict__ val,
                                             int64_t P, int64_t p0, int t, int32_t *srp, int32_t *scol, double *sval) {
  if (t <= AM_CELLS) srp[t] = rowptr[min(p0 + t, P)];   // rows past the end are empty
  __syncthreads();
  CsrRun r{col, val, scol, sval, t, srp[0], srp[AM_CELLS], 0};
  r.nchunk = (int)(((int64_t)r.r1 - r.r0 + AM_CHUNK - 1) / AM_CHUNK);
  if (r.nchunk == 1) {
    r.stage(r.r0);
    __syncthreads();
  }
  return r;
}

// The same run with NV value planes per entry, vstride elements apart in memory (k_wind_vector.hip: the 2 x 2 block of an entry), CH
// entries resident at a time: sval[NV][CH].  What CsrRun says about nchunk and the barriers of enter() holds here.
template <int NV, int CH>
struct CsrRunN {
  const int32_t *col;
  const double *val;
  int64_t vstride;
  int32_t *scol;
  double *sval;
  int t, r0, r1, nchunk;
  __device__ __forceinline__ void stage(int qa) const {
    const int n = min(CH, r1 - qa);
    for (int i = t; i < n; i += 256) {
      scol[i] = col[qa + i];
#pragma unroll
      for (int k = 0; k < NV; ++k) sval[k * CH + i] = val[k * vstride + qa + i];
    }
  }
  // chunk ch (ch * CH < r1 - r0) is resident on return; its first entry qa: plane k of entry q of the run is sval[k * CH + q - qa]
  __device__ __forceinline__ int enter(int ch) const {
    const int qa = r0 + ch * CH;
    if (nchunk > 1) {
      __syncthreads();   // the chunk before has been walked by every wave
      stage(qa);
      __syncthreads();
    }
    return qa;
  }
};
template <int NV, int CH>
__device__ __forceinline__ CsrRunN<NV, CH> am_csr_run_n(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                        const double *__restrict__ val, int64_t vstride, int64_t P, int64_t p0, int t,
                                                        int32_t *srp, int32_t *scol, double *sval) {
  if (t <= AM_CELLS) srp[t] = rowptr[min(p0 + t, P)];   // rows past the end are empty
  __syncthreads();
  CsrRunN<NV, CH> r{col, val, vstride, scol, sval, t, srp[0], srp[AM_CELLS], 0};
  r.nchunk = (int)(((int64_t)r.r1 - r.r0 + CH - 1) / CH);
  if (r.nchunk == 1) {
    r.stage(r.r0);
    __syncthreads();
  }
  return r;
}

// (point cc, level kk) of element e = cc * n + kk of a run of rows of n levels, for thread t's elements t, t + 256, ...: advanced by 256
// elements at a time without a division per element
struct RunCursor {
  int cc, kk, dc, dk, n;
  __device__ __forceinline__ RunCursor(int t, int n_) : cc(t / n_), kk(t % n_), dc(256 / n_), dk(256 % n_), n(n_) {}
  __device__ __forceinline__ void next() {
    cc += dc;
    kk += dk;
    if (kk >= n) {
      kk -= n;
      ++cc;
    }
  }
};

// The result tile [cell][S] of ncell points x kn levels leaves in destination order once every wave has written it: element e = cell
// (e / kn), level e % kn goes to out[cell * nlev + level] (out: the block's first point at the chunk's first level).  With kn == nlev
// that is one contiguous run and whole lines go non-temporal (geom.h stream_store_lane); a level chunk leaves as ncell pieces of a row.
template <typename TD>
__device__ __forceinline__ void am_drain_tile(const TD *tile, int S, TD *df, int64_t p0, int k0, int ncell, int kn, int nlev, int t, int lane) {
  __syncthreads();
  const int total = ncell * kn;
  RunCursor cur(t, kn);
  TD *out = df + p0 * nlev + k0;
  const bool run = kn == nlev;   // workgroup-uniform
  for (int e = t; e < total; e += 256) {
    TD *a = out + (int64_t)cur.cc * nlev + cur.kk;
    const TD r = tile[cur.cc * S + cur.kk];
    if (run) stream_store_lane(r, a, (unsigned)lane * (unsigned)sizeof(TD));
    else *a = r;
    cur.next();
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// The ntiles (1 or 2) [cell][lev] tiles of one shape of a 64-point block behind `head` bytes of dynamic LDS; together they stay within
// AM_TILE_BYTES: all levels in one tile when they fit the cap -- AM_TILE_BYTES for one tile, half of it for each of two (k_wind_pair.hip:
// a wind's two components; all levels up to 63 float64 / 127 float32, else chunks of 32 / 96) -- else chunks of kc levels, a multiple of
// 32 (a 128-byte line of a float32 row, two of a float64 row); row stride S odd, so that the column writes of a wave hit distinct banks.
// lds counts every tile.  No tile for [lev][cell] results (levf false).
struct TilePlan {
  int kc, S;
  size_t lds;
};
static inline TilePlan am_tile_plan(int nlev, size_t esz, bool levf, size_t head, int ntiles) {
  TilePlan p{nlev, 0, head};
  if (levf) {
    const size_t cap = AM_TILE_BYTES / ntiles;
    if ((size_t)AM_CELLS * (size_t)(nlev | 1) * esz > cap) p.kc = (int)(cap / (AM_CELLS * esz) - 1) / 32 * 32;
    p.S = p.kc | 1;
    p.lds += ntiles * (size_t)AM_CELLS * (size_t)p.S * esz;
  }
  return p;
}
static inline int am_allow_lds(const void *fn, size_t lds) {
  if (lds > 48 * 1024) MPG_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return MPG_SUCCESS;
}

// blocks of 64 points; one workgroup per (block, field) has to fit one launch
static inline int am_grid(const char *call, int64_t P, int nfields, uint64_t *ntile) {
  *ntile = (uint64_t)((P + AM_CELLS - 1) / AM_CELLS);
  if (*ntile * (uint64_t)nfields > 0x7fffffffull) {
    mpg_set_error("%s: %lld points x %d fields exceed one launch", call, (long long)P, nfields);
    return MPG_ERR_OVERFLOW;
  }
  return MPG_SUCCESS;
}

// a handle without sources maps nothing: the destination is the epilogue of 0.0 (as mpg_regrid_typed_dev); planes as mpg_zero_planes
static inline int am_no_sources(const char *call, void *dst, int dst_type, int64_t P, int64_t nplanes, int64_t ld, double offset, hipStream_t s) {
  if (offset != 0.0) {
    mpg_set_error("%s: handle without sources and a non-zero offset is not supported", call);
    return MPG_ERR_UNSUPPORTED;
  }
  return mpg_zero_planes(dst, (dst_type & MPG_TYPE_F32) ? 4 : 8, P, nplanes, ld, s);
}

// f(TS(), TD()) with the element types of (src_type, dst_type): float for MPG_TYPE_F32, else double
template <typename F>
static inline int mpg_dispatch_types(int src_type, int dst_type, F &&f) {
  const bool sf32 = src_type & MPG_TYPE_F32, df32 = dst_type & MPG_TYPE_F32;
  if (sf32 && df32) return f(float(), float());
  if (sf32) return f(float(), double());
  if (df32) return f(double(), float());
  return f(double(), double());
}
