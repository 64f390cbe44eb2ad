// Winds onto mesh EDGES (mpg_wind_to_edges_dev): U on one stagger and V on another -- grid-relative on a Lambert grid -- onto the edge
// points of a mesh as the edge-normal wind `u` MPAS carries, and the tangential component when asked, in ONE pass.  The rotation to
// earth-relative winds (alpha at the point) and the projection onto the edge normal (theta = angleEdge) compose into one rotation by
// phi = theta - alpha, so the kernel reads two per-point numbers cn = cos(phi), sn = sin(phi).  Per (point, level):
//   a  = fma(wsum_fixed<NNZ>(w_u, U[idx_u]), 1.0, 0.0)    float64, the bits of mpg_regrid_to_mesh_dev(rh_u, dst F64, scale 1, offset 0)
//   b  = fma(wsum_fixed<NNZ>(w_v, V[idx_v]), 1.0, 0.0)
//   un = a * cn + b * sn        two products and one sum, each rounded (no contraction)
//   ut = b * cn - a * sn        TAN only
//   store (TD)un [, (TD)ut]     one rounding to the destination type
// A point unmapped in either handle gets +0.0 in every result.
//
// The kernel is k_wind_to_mesh's skeleton: a 256-thread workgroup owns AM_CELLS consecutive points in xcd_remap block order; indices and
// weights of both handles are staged through LDS once (apply_mesh.h am_stage_fixed; ONE set when the two handles are the same) and then
// held in registers with the point's cn / sn; lanes run along points, wave w takes levels w, w + 4, ...; two levels are gathered per
// step (4 x NNZ independent loads in flight).
//   [lev][edge]  every level's 64 results (twice with ut) go straight out (stream_store_lane)
//   [edge][lev]  results are staged in ONE LDS tile (am_tile_plan), or TWO with ut (am_tile_plan_pair), which leave through
//                am_drain_tile, in level chunks when they outgrow the tile cap
// No atomics, no allocation, no synchronisation with the host: the call is capturable in a hipGraph from the first call.
#pragma clang fp contract(off)
#include "apply_mesh.h"

struct WindToEdges {
  const int32_t *idx_u, *idx_v;   // [NNZ][P] each, -1 = unmapped; the same pointers for one handle given twice
  const double *w_u, *w_v;        // [NNZ][P] (not read for NNZ 1)
  const double *cn, *sn;          // [P]
  const void *u, *v;              // [nlev] planes ldu / ldv elements apart
  void *un, *ut;                  // nlev * P each, [lev][edge] or [edge][lev]; ut only read by the TAN kernels
  int64_t P, ldu, ldv;
  int nlev, kc, S;
};

template <typename TS, typename TD, int NNZ, bool LEVF, bool TAN>
__global__ __launch_bounds__(256) void k_wind_to_edges(WindToEdges a) {
  extern __shared__ double sw[];                       // sw[2][NNZ][64] | sidx[2][NNZ][64] | tile_n[64][S] [| tile_t[64][S]] in the destination type
  int32_t *sidx = (int32_t *)(sw + 2 * NNZ * AM_CELLS);
  TD *tile_n = (TD *)(sidx + 2 * NNZ * AM_CELLS);
  TD *tile_t = tile_n + AM_CELLS * a.S;                // (TAN only: the plan holds one tile otherwise)
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
  double cn = 1.0, sn = 0.0;
  if (in) {
    cn = a.cn[p0 + lane];
    sn = a.sn[p0 + lane];
  }
  const TS *su = (const TS *)a.u, *sv = (const TS *)a.v;
  TD *dn = (TD *)a.un, *dt = (TD *)a.ut;
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
      const double t1 = ra * cn, t2 = rb * sn;
      const TD rn = both ? (TD)(t1 + t2) : (TD)0.0;
      TD rt = (TD)0.0;
      if (TAN) {
        const double t3 = rb * cn, t4 = ra * sn;
        rt = both ? (TD)(t3 - t4) : (TD)0.0;
      }
      if (LEVF) {
        tile_n[lane * S + k] = rn;
        if (TAN) tile_t[lane * S + k] = rt;
      } else if (in) {
        const int64_t off = (int64_t)(k0 + k) * P + p0 + lane;
        stream_store_lane(rn, dn + off, (unsigned)lane * (unsigned)sizeof(TD));
        if (TAN) stream_store_lane(rt, dt + off, (unsigned)lane * (unsigned)sizeof(TD));
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
      am_drain_tile(tile_n, S, dn, p0, k0, ncell, kn, nlev, t, lane);
      if (TAN) am_drain_tile(tile_t, S, dt, p0, k0, ncell, kn, nlev, t, lane);
      if (k0 + a.kc < nlev) __syncthreads();   // the next chunk overwrites the tiles
    }
  }
}

template <typename TS, typename TD, int NNZ, bool TAN>
static int launch_layout(const WindToEdges &a, bool levf, unsigned ntile, size_t lds, hipStream_t s) {
  auto fn = levf ? k_wind_to_edges<TS, TD, NNZ, true, TAN> : k_wind_to_edges<TS, TD, NNZ, false, TAN>;
  int rc = am_allow_lds((const void *)fn, lds);
  if (rc) return rc;
  fn<<<ntile, 256, lds, s>>>(a);
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

// The API entry point has checked the handles (fixed, no pole caps, both 4 slots or both 1, one n_dst), the strides (ldu >= hu->n_src,
// ldv >= hv->n_src), the enums and that cn / sn / un are set; ut == nullptr: the normal component only.
int mpg_k_wind_to_edges(mpg_handle_s *hu, mpg_handle_s *hv, const double *cn, const double *sn, const void *u, const void *v, int src_type,
                        int64_t ldu, int64_t ldv, int nlev, void *un, void *ut, int dst_type, int layout, hipStream_t s) {
  const int64_t P = hu->n_dst;
  if (P == 0 || nlev == 0) return MPG_SUCCESS;
  const size_t esz = (dst_type & MPG_TYPE_F32) ? 4 : 8;
  const bool tan = ut != nullptr;
  if (hu->n_src == 0 || hv->n_src == 0) {   // one handle maps nothing: every point is unmapped in it, so every result is +0.0
    int rc = mpg_zero_planes(un, esz, P, nlev, P, s);
    return rc || !tan ? rc : mpg_zero_planes(ut, esz, P, nlev, P, s);
  }
  uint64_t ntile;
  int rc = am_grid("mpg_wind_to_edges", P, 1, &ntile);
  if (rc) return rc;
  const int nnz = hu->nnz_per_row;
  const bool levf = layout == MPG_LAYOUT_LEV_FAST && nlev > 1;   // (a single level is the same memory in both layouts)
  const size_t head = (size_t)2 * nnz * AM_CELLS * (sizeof(double) + sizeof(int32_t));
  const TilePlan tp = tan ? am_tile_plan_pair(nlev, esz, levf, head) : am_tile_plan(nlev, esz, levf, head);
  const WindToEdges a{hu->idx.p, hv->idx.p, hu->w.p, hv->w.p, cn, sn, u, v, un, ut, P, ldu, ldv, nlev, tp.kc, tp.S};
  return mpg_dispatch_types(src_type, dst_type, [&](auto ts, auto td) {
    typedef decltype(ts) TS;
    typedef decltype(td) TD;
    if (nnz == 4)
      return tan ? launch_layout<TS, TD, 4, true>(a, levf, (unsigned)ntile, tp.lds, s) : launch_layout<TS, TD, 4, false>(a, levf, (unsigned)ntile, tp.lds, s);
    return tan ? launch_layout<TS, TD, 1, true>(a, levf, (unsigned)ntile, tp.lds, s) : launch_layout<TS, TD, 1, false>(a, levf, (unsigned)ntile, tp.lds, s);
  });
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_wind_to_edges() { return (const void *)&k_wind_to_edges<float, float, 4, true, false>; }
