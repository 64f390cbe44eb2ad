// A wind's two components onto one set of mesh points (mpg_wind_to_mesh_dev, mpg_wind_to_edges_dev): U on one stagger and V on another
// -- grid-relative on a Lambert grid -- through two handles onto the SAME points, combined there with two per-point numbers (c, s) and
// cast, in ONE pass: the two Regrids of k_apply_to_mesh.hip and the arithmetic between their float64 results and the store, without the
// two float64 intermediates a host would write and read again.  Per (point, level):
//   a  = fma(wsum_fixed<NNZ>(w_u, U[idx_u]), 1.0, 0.0)    float64, the bits of mpg_regrid_to_mesh_dev(rh_u, dst F64, scale 1, offset 0)
//   b  = fma(wsum_fixed<NNZ>(w_v, V[idx_v]), 1.0, 0.0)
//   (o0, o1) = combine(a, b, c, s)                        the policy C below; every product and sum rounded (no contraction, as k_rotate)
//   store (TD)o0 [, (TD)o1]                               one rounding to the destination type
// A point unmapped in either handle gets +0.0 in every result.  The four policies:
//   CellsRotated  mesh cells / vertices, earth-relative winds: c, s = cos / sin(alpha)   ue = a c - b s ; ve = a s + b c
//                 (the inverse of interp.F90:737-748: u_g = u_e ca + v_e sa, v_g = v_e ca - u_e sa)
//   CellsPlain    ... of a grid that does not rotate: no angles are read                 ue = a ; ve = b
//   EdgesNormal   mesh edges, the edge-normal wind `u` MPAS carries.  The rotation to earth-relative winds (alpha) and the projection
//                 onto the edge normal (theta = angleEdge) compose into one rotation by phi = theta - alpha: c, s = cos / sin(phi)
//                                                                                         un = a c + b s ; ONE result
//   EdgesBoth     ... and the tangential component                                       un = a c + b s ; ut = b c - a s
//
// The kernel is k_apply_to_mesh's with two of everything: a 256-thread workgroup owns AM_CELLS consecutive points in xcd_remap block
// order; indices and weights of both handles are staged through LDS once (apply_mesh.h am_stage_fixed; ONE set when the two handles are
// the same) and then held in registers with the point's c / s; lanes run along points, wave w takes levels w, w + 4, ...; two levels
// are gathered per step (4 x NNZ independent loads in flight).
//   [lev][point]  every level's 64 results per component go straight out (stream_store_lane)
//   [point][lev]  results are staged in NOUT LDS tiles, which leave one after the other through am_drain_tile, in level chunks when
//                 they outgrow the tile cap (apply_mesh.h am_tile_plan)
// No atomics, no allocation, no synchronisation with the host: the call is capturable in a hipGraph from the first call.
#pragma clang fp contract(off)
#include "apply_mesh.h"
#include "wind_policies.h"   // CellsRotated, CellsPlain, EdgesNormal, EdgesBoth: shared with k_wind_csr.hip

struct WindPair {
  const int32_t *idx_u, *idx_v;   // [NNZ][P] each, -1 = unmapped; the same pointers for one handle given twice
  const double *w_u, *w_v;        // [NNZ][P] (not read for NNZ 1)
  const double *c, *s;            // [P] (read by the policies with ANGLES only)
  const void *u, *v;              // [nlev] planes ldu / ldv elements apart
  void *r0, *r1;                  // nlev * P each, [lev][point] or [point][lev]; r1 only touched by the policies with NOUT 2
  int64_t P, ldu, ldv;
  int nlev, kc, S;
};

template <typename TS, typename TD, int NNZ, bool LEVF, typename C>
__global__ __launch_bounds__(256) void k_wind_pair(WindPair a) {
  extern __shared__ double sw[];                       // sw[2][NNZ][64] | sidx[2][NNZ][64] | tile0[64][S] [| tile1[64][S]] in the destination type
  int32_t *sidx = (int32_t *)(sw + 2 * NNZ * AM_CELLS);
  TD *tile0 = (TD *)(sidx + 2 * NNZ * AM_CELLS);
  TD *tile1 = tile0 + AM_CELLS * a.S;                  // (NOUT 2 only: the plan holds one tile otherwise)
  const unsigned tl = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t P = a.P, p0 = (int64_t)tl * AM_CELLS;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nlev = a.nlev, S = a.S;
  const bool same = a.idx_u == a.idx_v;                // workgroup-uniform: so are the barriers of the second staging
  am_stage_fixed<NNZ>(a.idx_u, a.w_u, P, p0, t, sidx, sw);
  if (!same) am_stage_fixed<NNZ>(a.idx_v, a.w_v, P, p0, t, sidx + NNZ * AM_CELLS, sw + NNZ * AM_CELLS);
  const int o = same ? 0 : NNZ * AM_CELLS;
  int32_t cu[NNZ], cv[NNZ];
  double wu[NNZ], wv[NNZ];
#pragma unroll
  for (int q = 0; q < NNZ; ++q) {
    cu[q] = sidx[q * AM_CELLS + lane];
    cv[q] = sidx[o + q * AM_CELLS + lane];
    wu[q] = NNZ > 1 ? sw[q * AM_CELLS + lane] : 1.0;
    wv[q] = NNZ > 1 ? sw[o + q * AM_CELLS + lane] : 1.0;
  }
  const bool mu = cu[0] >= 0, mv = cv[0] >= 0, both = mu && mv;
#pragma unroll
  for (int q = 0; q < NNZ; ++q) {   // an unmapped point reads source 0 and its result is masked
    cu[q] = mu ? cu[q] : 0;
    cv[q] = mv ? cv[q] : 0;
  }
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
  for (int k0 = 0; k0 < nlev; k0 += a.kc) {
    const int kn = min(a.kc, nlev - k0);
    const TS *uk = su + (int64_t)(k0 + wave) * ldu, *vk = sv + (int64_t)(k0 + wave) * ldv;
    auto gather = [&](const TS *pu, const TS *pv, double *xu, double *xv) {
#pragma unroll
      for (int q = 0; q < NNZ; ++q) xu[q] = (double)pu[cu[q]];
#pragma unroll
      for (int q = 0; q < NNZ; ++q) xv[q] = (double)pv[cv[q]];
    };
    auto put = [&](int k, const double *xu, const double *xv) {
      // fma(x, 1.0, 0.0): the epilogue of mpg_regrid_to_mesh_dev at scale 1, offset 0 (a -0.0 sum becomes +0.0 there too)
      const double ra = fma(wsum_fixed<NNZ>(wu, xu, mu), 1.0, 0.0), rb = fma(wsum_fixed<NNZ>(wv, xv, mv), 1.0, 0.0);
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
    };
    // two of the wave's levels per step: 4 x NNZ independent gathers in flight
    int k = wave;
    for (; k + 4 < kn; k += 8) {
      double u0[NNZ], v0[NNZ], u1[NNZ], v1[NNZ];
      gather(uk, vk, u0, v0);
      gather(uk + 4 * ldu, vk + 4 * ldv, u1, v1);
      put(k, u0, v0);
      put(k + 4, u1, v1);
      uk += 8 * ldu;
      vk += 8 * ldv;
    }
    if (k < kn) {
      double u0[NNZ], v0[NNZ];
      gather(uk, vk, u0, v0);
      put(k, u0, v0);
    }
    if (LEVF) {
      am_drain_tile(tile0, S, d0, p0, k0, ncell, kn, nlev, t, lane);
      if (C::NOUT == 2) am_drain_tile(tile1, S, d1, p0, k0, ncell, kn, nlev, t, lane);
      if (k0 + a.kc < nlev) __syncthreads();   // the next chunk overwrites the tiles
    }
  }
}

template <typename TS, typename TD, typename C>
static int launch(const WindPair &a, int nnz, bool levf, unsigned ntile, size_t lds, hipStream_t s) {
  auto fn = nnz == 4 ? (levf ? k_wind_pair<TS, TD, 4, true, C> : k_wind_pair<TS, TD, 4, false, C>)
                     : (levf ? k_wind_pair<TS, TD, 1, true, C> : k_wind_pair<TS, TD, 1, false, C>);
  int rc = am_allow_lds((const void *)fn, lds);
  if (rc) return rc;
  fn<<<ntile, 256, lds, s>>>(a);
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

// The API entry point has checked the handles (fixed, no pole caps, both 4 slots or both 1, one n_dst), the strides (ldu >= hu->n_src,
// ldv >= hv->n_src), the enums and the arrays.  edges false: (r0, r1) = (ue, ve), c / s both set or both NULL (no rotation); edges true:
// (r0, r1) = (un, ut), c / s set, r1 == nullptr: the normal component only.
int mpg_k_wind_pair(bool edges, mpg_handle_s *hu, mpg_handle_s *hv, const double *c, const double *s_, const void *u, const void *v, int src_type,
                    int64_t ldu, int64_t ldv, int nlev, void *r0, void *r1, int dst_type, int layout, hipStream_t s) {
  const int64_t P = hu->n_dst;
  if (P == 0 || nlev == 0) return MPG_SUCCESS;
  const size_t esz = (dst_type & MPG_TYPE_F32) ? 4 : 8;
  const int nout = edges && r1 == nullptr ? 1 : 2;
  if (hu->n_src == 0 || hv->n_src == 0) {   // one handle maps nothing: every point is unmapped in it, so every result is +0.0
    int rc = mpg_zero_planes(r0, esz, P, nlev, P, s);
    return rc || nout == 1 ? rc : mpg_zero_planes(r1, esz, P, nlev, P, s);
  }
  uint64_t ntile;
  int rc = am_grid(edges ? "mpg_wind_to_edges" : "mpg_wind_to_mesh", P, 1, &ntile);
  if (rc) return rc;
  const int nnz = hu->nnz_per_row;
  const bool levf = layout == MPG_LAYOUT_LEV_FAST && nlev > 1;   // (a single level is the same memory in both layouts)
  const TilePlan tp = am_tile_plan(nlev, esz, levf, (size_t)2 * nnz * AM_CELLS * (sizeof(double) + sizeof(int32_t)), nout);
  const WindPair a{hu->idx.p, hv->idx.p, hu->w.p, hv->w.p, c, s_, u, v, r0, r1, P, ldu, ldv, nlev, tp.kc, tp.S};
  return mpg_dispatch_types(src_type, dst_type, [&](auto ts, auto td) {
    typedef decltype(ts) TS;
    typedef decltype(td) TD;
    if (edges)
      return nout == 2 ? launch<TS, TD, EdgesBoth>(a, nnz, levf, (unsigned)ntile, tp.lds, s) : launch<TS, TD, EdgesNormal>(a, nnz, levf, (unsigned)ntile, tp.lds, s);
    return c ? launch<TS, TD, CellsRotated>(a, nnz, levf, (unsigned)ntile, tp.lds, s) : launch<TS, TD, CellsPlain>(a, nnz, levf, (unsigned)ntile, tp.lds, s);
  });
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_wind_pair() { return (const void *)&k_wind_pair<float, float, 4, true, CellsRotated>; }
