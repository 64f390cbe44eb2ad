// A wind's two components through two CSR handles onto one set of mesh points (mpg_wind_csr_to_mesh_dev, mpg_wind_csr_to_edges_dev): what
// k_wind_pair.hip does for two fixed handles, for the handles whose rows have any length -- the periodic Grid -> Mesh Store of a global
// lat-lon or Gaussian analysis, the conservative Stores, from-weights.  The two Regrids of k_apply_csr_to_mesh.hip and the arithmetic
// between their float64 results and the store, in ONE pass, without the two float64 intermediates a host would write and read again.
// Per (point, level):
//   acc_u = fma(val_u[q], (double)U[col_u[q]], acc_u)     from 0.0, the row's entries in stored order, whatever LDS chunk an entry arrives in
//   a  = fma(acc_u, 1.0, 0.0)                              float64, the bits of mpg_regrid_csr_to_mesh_dev(rh_u, dst F64, scale 1, offset 0)
//   b  = fma(acc_v, 1.0, 0.0)                              the same with rh_v, V
//   (o0, o1) = combine(a, b, c, s)                         the four policies of wind_policies.h (the table: k_wind_pair.hip), no contraction
//   store (TD)o0 [, (TD)o1]                                one rounding to the destination type
// A point whose row is empty in either handle gets +0.0 in every result (0 c - 0 s can be -0.0: hence a mask and not the arithmetic).
//
// The kernel is k_apply_csr_to_mesh's with two accumulators per level: a 256-thread workgroup owns AM_CELLS consecutive points in xcd_remap
// block order; the entries of its 64 rows are staged through LDS as one run per handle (apply_mesh.h CsrRun) -- ONE run when the two
// handles are the same, and then every staged (col, val) feeds both accumulators; with two handles each run is walked for its own
// component.  Lanes run along rows, wave w takes levels w, w + 4, ..., WC_LB levels at a time (2 x WC_LB independent fma chains per lane on
// one handle); a run longer than one chunk is staged again for every batch of 4 * WC_LB levels.  A row's sum is sequential, so no bit
// depends on WC_LB or on the chunking.  The point's c / s are held in registers.
// As compiled for gfx950 (profiles/r21_wind_csr.md) the one-handle loop stays at 64 to 78 VGPRs and waits for each of its 2 x WC_LB
// gathers before it issues the next: an entry costs eight load latencies where k_apply_csr_to_mesh pays one.  Rows of 4 entries hide
// that; a cap row of nx entries, walked by one lane, does not.  Known, measured, and left for a pull request of its own.
//   [lev][point]  every level's 64 results per component go straight out (stream_store_lane)
//   [point][lev]  results are staged in NOUT LDS tiles, which leave one after the other through am_drain_tile, in level chunks when
//                 they outgrow the tile cap (apply_mesh.h am_tile_plan, which is told how many runs are resident in front of the tiles)
// No atomics, no allocation, no synchronisation with the host: the call is capturable in a hipGraph from the first call.
#pragma clang fp contract(off)
#include "apply_mesh.h"
#include "wind_policies.h"

#define WC_LB 4                       // levels a wave carries at a time
#define WC_RP (AM_CELLS + 4)          // row pointers of a run, padded so that what lies behind them stays 8-byte aligned
// bytes of LDS in front of the tiles with nruns (1 or 2) runs resident
#define WC_HEAD(nruns) ((size_t)(nruns) * (AM_CHUNK * (sizeof(double) + sizeof(int32_t)) + WC_RP * sizeof(int32_t)))

struct WindCsr {
  const int32_t *rp_u, *rp_v;     // [P + 1] row pointers; the same pointers (all three) for one handle given twice
  const int32_t *col_u, *col_v;   // [nnz]
  const double *val_u, *val_v;    // [nnz]
  const double *c, *s;            // [P] (read by the policies with ANGLES only)
  const void *u, *v;              // [nlev] planes ldu / ldv elements apart
  void *r0, *r1;                  // nlev * P each, [lev][point] or [point][lev]; r1 only touched by the policies with NOUT 2
  int64_t P, ldu, ldv;
  int nlev, kc, S;
};

template <typename TS, typename TD, bool LEVF, typename C>
__global__ __launch_bounds__(256) void k_wind_csr(WindCsr a) {
  extern __shared__ double sval[];                     // sval[R][AM_CHUNK] | scol[R][AM_CHUNK] | srp[R][WC_RP] | tile0[64][S] [| tile1[64][S]]; R runs
  const bool same = a.rp_u == a.rp_v && a.col_u == a.col_v && a.val_u == a.val_v;   // workgroup-uniform: so are the barriers below
  const int R = same ? 1 : 2;
  int32_t *scol = (int32_t *)(sval + R * AM_CHUNK);
  int32_t *srp = scol + R * AM_CHUNK;
  TD *tile0 = (TD *)(srp + R * WC_RP);
  TD *tile1 = tile0 + AM_CELLS * a.S;                  // (NOUT 2 only: the plan holds one tile otherwise)
  const unsigned tl = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t P = a.P, p0 = (int64_t)tl * AM_CELLS;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nlev = a.nlev, S = a.S, kc = a.kc;
  const CsrRun ru = am_csr_run(a.rp_u, a.col_u, a.val_u, P, p0, t, srp, scol, sval);
  const CsrRun rv = same ? ru : am_csr_run(a.rp_v, a.col_v, a.val_v, P, p0, t, srp + WC_RP, scol + AM_CHUNK, sval + AM_CHUNK);
  const int ub = srp[lane], ue = srp[lane + 1];
  const int vb = same ? ub : srp[WC_RP + lane], ve = same ? ue : srp[WC_RP + lane + 1];
  const bool both = ub < ue && vb < ve;                // a row empty in either handle: +0.0 in every result
  const bool in = p0 + lane < P;
  double c = 1.0, s = 0.0;
  if (C::ANGLES && in) {
    c = a.c[p0 + lane];
    s = a.s[p0 + lane];
  }
  const TS *su = (const TS *)a.u, *sv = (const TS *)a.v;
  TD *d0 = (TD *)a.r0, *d1 = (TD *)a.r1;
  const int64_t ldu = a.ldu, ldv = a.ldv;
  const int ncell = (int)min((int64_t)AM_CELLS, P - p0);
  for (int k0 = 0; k0 < nlev; k0 += kc) {
    const int kn = min(kc, nlev - k0);
    for (int kb = 0; kb < kn; kb += 4 * WC_LB) {
      double au[WC_LB], av[WC_LB];
      const TS *pu[WC_LB], *pv[WC_LB];
#pragma unroll
      for (int j = 0; j < WC_LB; ++j) {
        const int k = kb + wave + 4 * j;
        const int64_t lev = k0 + (k < kn ? k : 0);      // a level slot past the chunk gathers level k0 and stores nothing
        au[j] = 0.0;
        av[j] = 0.0;
        pu[j] = su + lev * ldu;
        pv[j] = sv + lev * ldv;
      }
      if (same) {
        for (int ch = 0; ch < ru.nchunk; ++ch) {
          const int qa = ru.enter(ch);
          const int b = max(ub, qa), e = min(ue - qa, AM_CHUNK) + qa;
          for (int q = b; q < e; ++q) {
            const int32_t cc = scol[q - qa];
            const double w = sval[q - qa];
#pragma unroll
            for (int j = 0; j < WC_LB; ++j) {
              au[j] = fma(w, (double)pu[j][cc], au[j]);
              av[j] = fma(w, (double)pv[j][cc], av[j]);
            }
          }
        }
      } else {
        for (int ch = 0; ch < ru.nchunk; ++ch) {
          const int qa = ru.enter(ch);
          const int b = max(ub, qa), e = min(ue - qa, AM_CHUNK) + qa;
          for (int q = b; q < e; ++q) {
            const int32_t cc = ru.scol[q - qa];
            const double w = ru.sval[q - qa];
#pragma unroll
            for (int j = 0; j < WC_LB; ++j) au[j] = fma(w, (double)pu[j][cc], au[j]);
          }
        }
        for (int ch = 0; ch < rv.nchunk; ++ch) {
          const int qa = rv.enter(ch);
          const int b = max(vb, qa), e = min(ve - qa, AM_CHUNK) + qa;
          for (int q = b; q < e; ++q) {
            const int32_t cc = rv.scol[q - qa];
            const double w = rv.sval[q - qa];
#pragma unroll
            for (int j = 0; j < WC_LB; ++j) av[j] = fma(w, (double)pv[j][cc], av[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < WC_LB; ++j) {
        const int k = kb + wave + 4 * j;
        if (k < kn) {
          // fma(x, 1.0, 0.0): the epilogue of mpg_regrid_csr_to_mesh_dev at scale 1, offset 0 (a -0.0 sum becomes +0.0 there too)
          const double ra = fma(au[j], 1.0, 0.0), rb = fma(av[j], 1.0, 0.0);
          double o0, o1;
          C::combine(ra, rb, c, s, o0, o1);
          const TD q0 = both ? (TD)o0 : (TD)0.0, q1 = both ? (TD)o1 : (TD)0.0;
          if (LEVF) {
            tile0[lane * S + k] = q0;
            if (C::NOUT == 2) tile1[lane * S + k] = q1;
          } else if (in) {
            const int64_t off = (int64_t)(k0 + k) * P + p0 + lane;
            stream_store_lane(q0, d0 + off, (unsigned)lane * (unsigned)sizeof(TD));
            if (C::NOUT == 2) stream_store_lane(q1, d1 + off, (unsigned)lane * (unsigned)sizeof(TD));
          }
        }
      }
    }
    if (LEVF) {
      am_drain_tile(tile0, S, d0, p0, k0, ncell, kn, nlev, t, lane);
      if (C::NOUT == 2) am_drain_tile(tile1, S, d1, p0, k0, ncell, kn, nlev, t, lane);
      if (k0 + kc < nlev) __syncthreads();   // the next chunk overwrites the tiles
    }
  }
}

template <typename TS, typename TD, typename C>
static int launch(const WindCsr &a, bool levf, unsigned ntile, size_t lds, hipStream_t s) {
  auto fn = levf ? k_wind_csr<TS, TD, true, C> : k_wind_csr<TS, TD, false, C>;
  int rc = am_allow_lds((const void *)fn, lds);
  if (rc) return rc;
  fn<<<ntile, 256, lds, s>>>(a);
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

// The API entry point has checked the handles (CSR, no pole terms, one n_dst), the strides (ldu >= hu->n_src, ldv >= hv->n_src), the enums
// and the arrays.  edges false: (r0, r1) = (ue, ve), c / s both set or both NULL (no rotation); edges true: (r0, r1) = (un, ut), c / s
// set, r1 == nullptr: the normal component only.
int mpg_k_wind_csr(bool edges, mpg_handle_s *hu, mpg_handle_s *hv, const double *c, const double *s_, const void *u, const void *v, int src_type,
                   int64_t ldu, int64_t ldv, int nlev, void *r0, void *r1, int dst_type, int layout, hipStream_t s) {
  const int64_t P = hu->n_dst;
  if (P == 0 || nlev == 0) return MPG_SUCCESS;
  const size_t esz = (dst_type & MPG_TYPE_F32) ? 4 : 8;
  const int nout = edges && r1 == nullptr ? 1 : 2;
  if (hu->nnz == 0 || hv->nnz == 0) {   // one handle has no entries: every row is empty in it, so every result is +0.0
    int rc = mpg_zero_planes(r0, esz, P, nlev, P, s);
    return rc || nout == 1 ? rc : mpg_zero_planes(r1, esz, P, nlev, P, s);
  }
  uint64_t ntile;
  int rc = am_grid(edges ? "mpg_wind_csr_to_edges" : "mpg_wind_csr_to_mesh", P, 1, &ntile);
  if (rc) return rc;
  const bool same = hu->rowptr.p == hv->rowptr.p && hu->col.p == hv->col.p && hu->val.p == hv->val.p;   // (the kernel's own test)
  const bool levf = layout == MPG_LAYOUT_LEV_FAST && nlev > 1;   // (a single level is the same memory in both layouts)
  const TilePlan tp = am_tile_plan(nlev, esz, levf, WC_HEAD(same ? 1 : 2), nout);
  const WindCsr a{hu->rowptr.p, hv->rowptr.p, hu->col.p, hv->col.p, hu->val.p, hv->val.p, c, s_, u, v, r0, r1, P, ldu, ldv, nlev, tp.kc, tp.S};
  return mpg_dispatch_types(src_type, dst_type, [&](auto ts, auto td) {
    typedef decltype(ts) TS;
    typedef decltype(td) TD;
    if (edges)
      return nout == 2 ? launch<TS, TD, EdgesBoth>(a, levf, (unsigned)ntile, tp.lds, s) : launch<TS, TD, EdgesNormal>(a, levf, (unsigned)ntile, tp.lds, s);
    return c ? launch<TS, TD, CellsRotated>(a, levf, (unsigned)ntile, tp.lds, s) : launch<TS, TD, CellsPlain>(a, levf, (unsigned)ntile, tp.lds, s);
  });
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_wind_csr() { return (const void *)&k_wind_csr<float, float, true, CellsRotated>; }
