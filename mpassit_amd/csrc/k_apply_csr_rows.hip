// CSR Regrid from rows to rows: the source is [n_src][nlev] and the result [n_dst][nlev] -- MPAS file order on both sides, the memory order
// of a conservative Mesh -> Mesh job that reads a field from one MPAS file and writes it to another (mpg_regrid_csr_rows_dev).  Any CSR
// handle without pole caps is served (conservative Mesh -> Mesh, Grid -> Mesh, Mesh -> Grid, from-weights).
//
// The block's results are ONE contiguous run of 64 * nlev elements and the kernel is laid out along that run, as k_apply_rows is
// (apply_mesh.h RunCursor): every wavefront store is 64 consecutive elements (geom.h stream_store_lane), and the lanes of a point read
// consecutive levels of the same source row.  The entries of the 64 rows are staged through LDS as one run (apply_mesh.h CsrRun), a run
// longer than one chunk again for every batch of CR_UNROLL * 256 elements.  An element's accumulator stays in a register across the
// chunks; CR_UNROLL elements per thread are in flight, each walking its own row's part of the chunk.  No LDS result tile, no level
// chunks.  Row bases are 64-bit.
// A row's value is k_apply_generic_t<..., NNZ = 0, ...>'s expression -- acc = fma(val[q], src[col[q] * nlev + k], acc) from 0.0 in stored
// order, whatever chunk an entry arrives in -- then fma(acc, scale, offset) rounded once to the destination type: element [p][k] has the
// bits of element [k][p] of mpg_regrid_typed_dev(MPG_LAYOUT_LEV_FAST).  An empty row gives (dst type)(0.0 * scale + offset).
// No atomics, no allocation, no synchronisation with the host: the call is capturable in a hipGraph from the first call.
#include "apply_mesh.h"

#define CR_UNROLL 4

template <typename TS, typename TD>
__global__ __launch_bounds__(256) void k_apply_csr_rows(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                        const double *__restrict__ val, const TS *__restrict__ src, TD *__restrict__ dst,
                                                        int64_t P, int64_t n_src, int nlev, unsigned ntile, double scale, double offset) {
  __shared__ double sval[AM_CHUNK];
  __shared__ int32_t scol[AM_CHUNK];
  __shared__ int32_t srp[AM_CELLS + 1];
  const unsigned lin = xcd_remap(blockIdx.x, gridDim.x);
  const unsigned tl = lin % ntile;
  const int f = (int)(lin / ntile);
  const int64_t p0 = (int64_t)tl * AM_CELLS;
  const int t = threadIdx.x, lane = t & 63;
  const CsrRun run = am_csr_run(rowptr, col, val, P, p0, t, srp, scol, sval);
  const TS *sf = src + (int64_t)f * n_src * nlev;
  TD *out = dst + ((int64_t)f * P + p0) * nlev;
  const int ncell = (int)min((int64_t)AM_CELLS, P - p0);
  const int total = ncell * nlev;
  RunCursor cur(t, nlev);
  for (int e0 = 0; e0 < total; e0 += CR_UNROLL * 256) {   // (workgroup-uniform: every thread meets the barriers below)
    double acc[CR_UNROLL];
    int rb[CR_UNROLL], re[CR_UNROLL];
    const TS *ps[CR_UNROLL];
#pragma unroll
    for (int u = 0; u < CR_UNROLL; ++u) {
      const bool ok = e0 + t + u * 256 < total;   // an element past the run's end walks an empty row and stores nothing
      acc[u] = 0.0;
      rb[u] = ok ? srp[cur.cc] : 0;
      re[u] = ok ? srp[cur.cc + 1] : 0;
      ps[u] = sf + (ok ? cur.kk : 0);
      cur.next();
    }
    for (int ch = 0; ch < run.nchunk; ++ch) {
      const int qa = run.enter(ch);
      // this chunk's part of every element's row, as positions in the staged chunk: [b, b + n)
      int b[CR_UNROLL], n[CR_UNROLL], nmax = 0;
#pragma unroll
      for (int u = 0; u < CR_UNROLL; ++u) {
        b[u] = max(rb[u], qa) - qa;
        n[u] = min(re[u] - qa, AM_CHUNK) - b[u];
        nmax = max(nmax, n[u]);
      }
      for (int i = 0; i < nmax; ++i) {
#pragma unroll
        for (int u = 0; u < CR_UNROLL; ++u)
          if (i < n[u]) acc[u] = fma(sval[b[u] + i], (double)ps[u][(int64_t)scol[b[u] + i] * nlev], acc[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < CR_UNROLL; ++u) {
      const int e = e0 + t + u * 256;
      const TD r = (TD)fma(acc[u], scale, offset);
      if (e < total) stream_store_lane(r, out + e, (unsigned)lane * (unsigned)sizeof(TD));
    }
  }
}

template <typename TS, typename TD>
static int launch_csr_rows(mpg_handle_s *h, const void *src, int nlev, int nfields, void *dst, double scale, double offset, hipStream_t s) {
  const int64_t P = h->n_dst;
  uint64_t ntile;
  int rc = am_grid("mpg_regrid_csr_rows", P, nfields, &ntile);
  if (rc) return rc;
  k_apply_csr_rows<TS, TD><<<(unsigned)(ntile * (uint64_t)nfields), 256, 0, s>>>(h->rowptr.p, h->col.p, h->val.p, (const TS *)src, (TD *)dst, P,
                                                                                h->n_src, nlev, (unsigned)ntile, scale, offset);
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

// (the handle's kind and the level count are checked by the API entry point)
int mpg_k_apply_csr_rows(mpg_handle_s *h, const void *src, int src_type, int nlev, int nfields, void *dst, int dst_type, double scale, double offset,
                         hipStream_t s) {
  if (h->n_dst == 0 || nfields == 0) return MPG_SUCCESS;
  return mpg_dispatch_types(src_type, dst_type, [&](auto ts, auto td) {
    return launch_csr_rows<decltype(ts), decltype(td)>(h, src, nlev, nfields, dst, scale, offset, s);
  });
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_apply_csr_rows() { return (const void *)&k_apply_csr_rows<float, float>; }
