// Regrid from rows to rows: the source is [n_src][nlev] and the result [n_dst][nlev] -- MPAS file order on both sides, the memory order
// of a Mesh -> Mesh job that reads a field from one MPAS file and writes it to another (mpg_regrid_rows_dev).  Serves every fixed-nnz
// handle without pole caps: 3 weights (Mesh -> Mesh / Mesh -> Grid bilinear), 4 (Grid -> Mesh, Grid -> Grid), 1 (nearest).
//
// The block's results are ONE contiguous run of 64 * nlev elements, and the kernel is laid out along that run: element e of the run is
// point e / nlev, level e % nlev (apply_mesh.h RunCursor), and thread t takes elements t, t + 256, ... -- a wavefront always holds 64
// consecutive elements of the run, whatever nlev is, so
//   stores  every wavefront store is 64 consecutive elements: whole 128-byte lines non-temporal, the run's two end lines write-back
//           (geom.h stream_store_lane); no LDS tile, no level chunks, no lane idles on an odd nlev
//   loads   the lanes of a wavefront that share a point read consecutive levels of the same source rows: with nlev = 55 a wavefront
//           covers parts of two points and each of its NNZ gathers is two coalesced pieces of two rows (220 / 440 bytes a whole row)
// The points' indices and weights are staged once through LDS (am_stage_fixed) and read from there per element (the point changes along
// a wavefront).  Four elements per thread are in flight at a time: 4 x NNZ independent row reads.  Row bases are 64-bit (n_src * nlev
// exceeds int32 at the 3 M-cell sizes).  Arithmetic and epilogue are those of the typed Regrid (geom.h wsum_fixed, then
// fma(x, scale, offset) rounded once to the destination type): element [p][k] has the bits of element [k][p] of
// mpg_regrid_typed_dev(MPG_LAYOUT_LEV_FAST).
// No atomics, no allocation, no synchronisation with the host: the call is capturable in a hipGraph from the first call.
#include "apply_mesh.h"

#define RW_UNROLL 4

template <typename TS, typename TD, int NNZ>
__global__ __launch_bounds__(256) void k_apply_rows(const int32_t *__restrict__ idx, const double *__restrict__ w, const TS *__restrict__ src,
                                                    TD *__restrict__ dst, int64_t P, int64_t n_src, int nlev, unsigned ntile, double scale,
                                                    double offset) {
  __shared__ double sw[NNZ * AM_CELLS];
  __shared__ int32_t sidx[NNZ * AM_CELLS];
  const unsigned lin = xcd_remap(blockIdx.x, gridDim.x);
  const unsigned tl = lin % ntile;
  const int f = (int)(lin / ntile);
  const int64_t p0 = (int64_t)tl * AM_CELLS;
  const int t = threadIdx.x, lane = t & 63;
  am_stage_fixed<NNZ>(idx, w, P, p0, t, sidx, sw);
  const TS *sf = src + (int64_t)f * n_src * nlev;
  TD *out = dst + ((int64_t)f * P + p0) * nlev;
  const int ncell = (int)min((int64_t)AM_CELLS, P - p0);
  const int total = ncell * nlev;
  RunCursor cur(t, nlev);
  for (int e0 = t; e0 < total; e0 += RW_UNROLL * 256) {
    double v[RW_UNROLL][NNZ], ww[RW_UNROLL][NNZ];
    bool mapped[RW_UNROLL];
#pragma unroll
    for (int u = 0; u < RW_UNROLL; ++u) {
      const bool ok = e0 + u * 256 < total;
      const int c = ok ? cur.cc : 0;   // a lane past the run's end reads point 0's row (a valid one) and stores nothing
      mapped[u] = sidx[c] >= 0;
#pragma unroll
      for (int q = 0; q < NNZ; ++q) {
        const int32_t s = mapped[u] ? sidx[q * AM_CELLS + c] : 0;   // an unmapped point reads source 0 and its result is masked (wsum_fixed)
        ww[u][q] = NNZ > 1 ? sw[q * AM_CELLS + c] : 1.0;
        v[u][q] = (double)sf[(int64_t)s * nlev + cur.kk];
      }
      cur.next();
    }
#pragma unroll
    for (int u = 0; u < RW_UNROLL; ++u) {
      const int e = e0 + u * 256;
      const TD r = (TD)fma(wsum_fixed<NNZ>(ww[u], v[u], mapped[u]), scale, offset);
      if (e < total) stream_store_lane(r, out + e, (unsigned)lane * (unsigned)sizeof(TD));
    }
  }
}

template <typename TS, typename TD, int NNZ>
static int launch_rows(mpg_handle_s *h, const void *src, int nlev, int nfields, void *dst, double scale, double offset, hipStream_t s) {
  const int64_t P = h->n_dst;
  uint64_t ntile;
  int rc = am_grid("mpg_regrid_rows", P, nfields, &ntile);
  if (rc) return rc;
  k_apply_rows<TS, TD, NNZ><<<(unsigned)(ntile * (uint64_t)nfields), 256, 0, s>>>(h->idx.p, h->w.p, (const TS *)src, (TD *)dst, P, h->n_src, nlev,
                                                                                 (unsigned)ntile, scale, offset);
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

template <typename TS, typename TD>
static int launch_nnz(mpg_handle_s *h, const void *src, int nlev, int nfields, void *dst, double scale, double offset, hipStream_t s) {
  if (h->nnz_per_row == 4) return launch_rows<TS, TD, 4>(h, src, nlev, nfields, dst, scale, offset, s);
  if (h->nnz_per_row == 3) return launch_rows<TS, TD, 3>(h, src, nlev, nfields, dst, scale, offset, s);
  return launch_rows<TS, TD, 1>(h, src, nlev, nfields, dst, scale, offset, s);
}

// (the handle's kind, its slot count and the level count are checked by the API entry point)
int mpg_k_apply_rows(mpg_handle_s *h, const void *src, int src_type, int nlev, int nfields, void *dst, int dst_type, double scale, double offset,
                     hipStream_t s) {
  if (h->n_dst == 0 || nfields == 0) return MPG_SUCCESS;
  // nothing mapped: nfields planes of n_dst rows
  if (h->n_src == 0) return am_no_sources("mpg_regrid_rows", dst, dst_type, h->n_dst * (int64_t)nlev, nfields, h->n_dst * (int64_t)nlev, offset, s);
  return mpg_dispatch_types(src_type, dst_type, [&](auto ts, auto td) {
    return launch_nnz<decltype(ts), decltype(td)>(h, src, nlev, nfields, dst, scale, offset, s);
  });
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_apply_rows() { return (const void *)&k_apply_rows<float, float, 3>; }
