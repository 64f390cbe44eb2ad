// A wind as a VECTOR through one CSR handle (mpg_sphere_frames_dev, mpg_wind_vector_weights_dev, mpg_wind_vector_dev): ESMF 8.6's
// vectorRegrid.  (u, v) at a source point becomes a Cartesian 3-vector with the point's local frame, the three components are regridded
// with the handle's weights and the result is projected onto the destination point's frame.  The weights do not depend on the level, so
// the three steps fold into one 2 x 2 block per CSR entry q of row p, c = col[q]:
//   m00 = val[q] * ((e.x*D0.x + e.y*D0.y) + e.z*D0.z)    e = source D0 at c, n = source D1 at c, (D0, D1) the destination frame at p
//   m01 = val[q] * ((n.x*D0.x + n.y*D0.y) + n.z*D0.z)    m10, m11: the same against the destination D1
// computed once per (handle, frames) by k_vector_weights, and the hot path is k_wind_vector, per (point, level):
//   acc_kl = fma(m_kl[q], (double)src_l[col[q]], acc_kl)  from 0.0, the row's entries in stored order, whatever LDS chunk an entry arrives in
//   o0 = fma(acc00, 1.0, 0.0) + fma(acc01, 1.0, 0.0)      src_0 = U, src_1 = V: mpg_regrid_csr_to_mesh_dev of a from-weights handle with
//   o1 = fma(acc10, 1.0, 0.0) + fma(acc11, 1.0, 0.0)      values m00 on U plus the same with m01 on V, float64, added once
//   store (TD)o0 [, (TD)o1]                               one rounding to the destination type; an empty row gives (TD)(+0.0)
// Under MPG_POLEMETHOD_ALLAVG a cap row is then the mean of the source row's VECTORS seen from the cap point, which is a wind; the two
// scalar Regrids of k_wind_csr.hip give the row mean of each component there, which is not.
//
// The kernel has the workgroup shape of k_wind_csr's one-handle branch: a 256-thread workgroup owns AM_CELLS consecutive points in
// xcd_remap block order; col and the 2 NOUT coefficient planes of its 64 rows are staged through LDS as ONE run (apply_mesh.h CsrRunN),
// WV_CHUNK entries at a time.  Lanes run along rows, wave w takes levels w, w + 4, ..., WV_LB levels at a time (2 NOUT x WV_LB
// independent fma chains per lane); a run longer than one chunk is staged again for every batch of 4 * WV_LB levels.  A row's sum is
// sequential, so no bit depends on WV_LB, on WV_CHUNK or on the chunking, and long rows are not split across lanes.
// A row is walked two entries at a time: the 2 x 2 x WV_LB gathers of a pair are loaded into temporaries ahead of its fmas, and the next
// pair's are issued before the fmas of the pair at hand (profiles/r21_wind_csr.md: k_wind_csr waits for each of its eight gathers before
// it issues the next, which a cap row of nx entries walked by ONE lane pays in full; profiles/r22_wind_vector.md: what the compiler made
// of this loop, and what it bought).
// WV_CHUNK is 384, not AM_CHUNK: with four planes an entry takes 36 bytes of LDS, and 384 of them (13.8 KB with the row pointers) in
// front of at most 64 KB of tiles keep a workgroup below 80 KB, so that two fit the 160 KB of a CU whatever the level count; [lev][point]
// results need no tile and LDS does not limit the residency there.
//   [lev][point]  every level's 64 results per component go straight out (stream_store_lane)
//   [point][lev]  results are staged in NOUT LDS tiles, which leave one after the other through am_drain_tile, in level chunks when
//                 they outgrow the tile cap (apply_mesh.h am_tile_plan)
// No atomics, no allocation, no synchronisation with the host: the calls are capturable in a hipGraph from the first call.
#pragma clang fp contract(off)
#include "apply_mesh.h"
#include "wind_vector_checks.h"   // WV_LB, WV_CHUNK, WV_RP, wv_lds_head: shared with the host-side checks

static_assert(WV_ROWS == AM_CELLS, "the checks count the launch's blocks in AM_CELLS rows");

// ---- frames -----------------------------------------------------------------------------------------------------------------------------
// frames[6][n]: D0x D0y D0z D1x D1y D1z of n points (lon, lat in radians); c == nullptr: (east, north), else turned by (c, s)
__global__ __launch_bounds__(256) void k_sphere_frames(int64_t n, const double *__restrict__ lon, const double *__restrict__ lat,
                                                       const double *__restrict__ c, const double *__restrict__ s, double *__restrict__ f) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double sl = sin(lon[i]), cl = cos(lon[i]), sp = sin(lat[i]), cp = cos(lat[i]);
  const double e[3] = {-sl, cl, 0.0};
  const double nn[3] = {-sp * cl, -sp * sl, cp};
  if (c == nullptr) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      f[k * n + i] = e[k];
      f[(3 + k) * n + i] = nn[k];
    }
  } else {
    const double ci = c[i], si = s[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      f[k * n + i] = ci * e[k] + si * nn[k];
      f[(3 + k) * n + i] = ci * nn[k] - si * e[k];
    }
  }
}

// ---- blocks -----------------------------------------------------------------------------------------------------------------------------
// One thread per row: m[4][nnz] in the handle's entry order.  A set-up kernel: it runs once per (handle, frames).
__global__ __launch_bounds__(256) void k_vector_weights(int64_t P, int64_t ns, int64_t nnz, const int32_t *__restrict__ rowptr,
                                                        const int32_t *__restrict__ col, const double *__restrict__ val,
                                                        const double *__restrict__ sf, const double *__restrict__ df, double *__restrict__ m) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  double d0[3], d1[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    d0[k] = df[k * P + p];
    d1[k] = df[(3 + k) * P + p];
  }
  const int qe = rowptr[p + 1];
  for (int q = rowptr[p]; q < qe; ++q) {
    const int64_t cc = col[q];
    const double w = val[q];
    double e[3], nn[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      e[k] = sf[k * ns + cc];
      nn[k] = sf[(3 + k) * ns + cc];
    }
    m[q] = w * ((e[0] * d0[0] + e[1] * d0[1]) + e[2] * d0[2]);
    m[nnz + q] = w * ((nn[0] * d0[0] + nn[1] * d0[1]) + nn[2] * d0[2]);
    m[2 * nnz + q] = w * ((e[0] * d1[0] + e[1] * d1[1]) + e[2] * d1[2]);
    m[3 * nnz + q] = w * ((nn[0] * d1[0] + nn[1] * d1[1]) + nn[2] * d1[2]);
  }
}

// ---- the apply --------------------------------------------------------------------------------------------------------------------------
struct WindVec {
  const int32_t *rp;      // [P + 1] row pointers
  const int32_t *col;     // [nnz]
  const double *m;        // [4][nnz] m00 m01 m10 m11 (NOUT 1 reads the first two planes)
  const void *u, *v;      // [nlev] planes ldu / ldv elements apart
  void *r0, *r1;          // nlev * P each, [lev][point] or [point][lev]; r1 only touched with NOUT 2
  int64_t P, nnz, ldu, ldv;
  int nlev, kc, S;
};

template <typename TS, typename TD, bool LEVF, int NOUT>
__global__ __launch_bounds__(256) void k_wind_vector(WindVec a) {
  constexpr int NV = 2 * NOUT;
  extern __shared__ double sval[];                     // sval[NV][WV_CHUNK] | scol[WV_CHUNK] | srp[WV_RP] | tile0[64][S] [| tile1[64][S]]
  int32_t *scol = (int32_t *)(sval + NV * WV_CHUNK);
  int32_t *srp = scol + WV_CHUNK;
  TD *tile0 = (TD *)(srp + WV_RP);
  TD *tile1 = tile0 + AM_CELLS * a.S;                  // (NOUT 2 only: the plan holds one tile otherwise)
  const unsigned tl = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t P = a.P, p0 = (int64_t)tl * AM_CELLS;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nlev = a.nlev, S = a.S, kc = a.kc;
  const CsrRunN<NV, WV_CHUNK> run = am_csr_run_n<NV, WV_CHUNK>(a.rp, a.col, a.m, a.nnz, P, p0, t, srp, scol, sval);
  const int rb = srp[lane], re = srp[lane + 1];
  const bool in = p0 + lane < P;
  const TS *su = (const TS *)a.u, *sv = (const TS *)a.v;
  TD *d0 = (TD *)a.r0, *d1 = (TD *)a.r1;
  const int64_t ldu = a.ldu, ldv = a.ldv;
  const int ncell = (int)min((int64_t)AM_CELLS, P - p0);
  for (int k0 = 0; k0 < nlev; k0 += kc) {
    const int kn = min(kc, nlev - k0);
    for (int kb = 0; kb < kn; kb += 4 * WV_LB) {
      double acc[NV][WV_LB];
      const TS *pu[WV_LB], *pv[WV_LB];
#pragma unroll
      for (int j = 0; j < WV_LB; ++j) {
        const int k = kb + wave + 4 * j;
        const int64_t lev = k0 + (k < kn ? k : 0);      // a level slot past the chunk gathers level k0 and stores nothing
#pragma unroll
        for (int i = 0; i < NV; ++i) acc[i][j] = 0.0;
        pu[j] = su + lev * ldu;
        pv[j] = sv + lev * ldv;
      }
      for (int ch = 0; ch < run.nchunk; ++ch) {
        const int qa = run.enter(ch);
        const int b = max(rb, qa), e = min(re - qa, WV_CHUNK) + qa;
        // entries in pairs: the 2 x 2 x WV_LB gathers of a pair in flight together, and the next pair's issued ahead of this pair's fmas
        auto gather = [&](int q, TS *xu, TS *xv) {
          const int32_t cc = scol[q - qa];
#pragma unroll
          for (int j = 0; j < WV_LB; ++j) {
            xu[j] = pu[j][cc];
            xv[j] = pv[j][cc];
          }
        };
        auto widen = [](const TS *x, double *y) {
#pragma unroll
          for (int j = 0; j < WV_LB; ++j) y[j] = (double)x[j];
        };
        auto add = [&](int q, const double *yu, const double *yv) {   // entry q into every chain, in stored order
          double w[NV];
#pragma unroll
          for (int i = 0; i < NV; ++i) w[i] = sval[i * WV_CHUNK + q - qa];
#pragma unroll
          for (int j = 0; j < WV_LB; ++j) {
            acc[0][j] = fma(w[0], yu[j], acc[0][j]);
            acc[1][j] = fma(w[1], yv[j], acc[1][j]);
            if (NOUT == 2) {
              acc[NV - 2][j] = fma(w[NV - 2], yu[j], acc[NV - 2][j]);
              acc[NV - 1][j] = fma(w[NV - 1], yv[j], acc[NV - 1][j]);
            }
          }
        };
        TS xu0[WV_LB], xv0[WV_LB], xu1[WV_LB], xv1[WV_LB];
        if (b < e) gather(b, xu0, xv0);
        if (b + 1 < e) gather(b + 1, xu1, xv1);
        for (int q = b; q < e; q += 2) {
          double yu0[WV_LB], yv0[WV_LB], yu1[WV_LB], yv1[WV_LB];
          const bool two = q + 1 < e;
          widen(xu0, yu0);
          widen(xv0, yv0);
          if (two) {
            widen(xu1, yu1);
            widen(xv1, yv1);
          }
          if (q + 2 < e) gather(q + 2, xu0, xv0);
          if (q + 3 < e) gather(q + 3, xu1, xv1);
          add(q, yu0, yv0);
          if (two) add(q + 1, yu1, yv1);
        }
      }
#pragma unroll
      for (int j = 0; j < WV_LB; ++j) {
        const int k = kb + wave + 4 * j;
        if (k < kn) {
          // fma(x, 1.0, 0.0): the epilogue of mpg_regrid_csr_to_mesh_dev at scale 1, offset 0 (a -0.0 sum becomes +0.0 there too)
          const TD q0 = (TD)(fma(acc[0][j], 1.0, 0.0) + fma(acc[1][j], 1.0, 0.0));
          const TD q1 = NOUT == 2 ? (TD)(fma(acc[NV - 2][j], 1.0, 0.0) + fma(acc[NV - 1][j], 1.0, 0.0)) : (TD)0.0;
          if (LEVF) {
            tile0[lane * S + k] = q0;
            if (NOUT == 2) tile1[lane * S + k] = q1;
          } else if (in) {
            const int64_t off = (int64_t)(k0 + k) * P + p0 + lane;
            stream_store_lane(q0, d0 + off, (unsigned)lane * (unsigned)sizeof(TD));
            if (NOUT == 2) stream_store_lane(q1, d1 + off, (unsigned)lane * (unsigned)sizeof(TD));
          }
        }
      }
    }
    if (LEVF) {
      am_drain_tile(tile0, S, d0, p0, k0, ncell, kn, nlev, t, lane);
      if (NOUT == 2) am_drain_tile(tile1, S, d1, p0, k0, ncell, kn, nlev, t, lane);
      if (k0 + kc < nlev) __syncthreads();   // the next chunk overwrites the tiles
    }
  }
}

template <typename TS, typename TD, int NOUT>
static int launch(const WindVec &a, bool levf, unsigned ntile, size_t lds, hipStream_t s) {
  auto fn = levf ? k_wind_vector<TS, TD, true, NOUT> : k_wind_vector<TS, TD, false, NOUT>;
  int rc = am_allow_lds((const void *)fn, lds);
  if (rc) return rc;
  fn<<<ntile, 256, lds, s>>>(a);
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

// one thread per point in blocks of 256: the blocks of one launch
static int point_grid(const char *call, int64_t n, unsigned *nblock) {
  const uint64_t nb = ((uint64_t)n + 255) / 256;
  if (nb > 0x7fffffffull) {
    mpg_set_error("%s: %lld points exceed one launch", call, (long long)n);
    return MPG_ERR_OVERFLOW;
  }
  *nblock = (unsigned)nb;
  return MPG_SUCCESS;
}

// The API entry points have checked their arguments.
int mpg_k_sphere_frames(int64_t n, const double *lon, const double *lat, const double *c, const double *s_, double *frames, hipStream_t s) {
  if (n == 0) return MPG_SUCCESS;
  unsigned nb;
  int rc = point_grid("mpg_sphere_frames", n, &nb);
  if (rc) return rc;
  k_sphere_frames<<<nb, 256, 0, s>>>(n, lon, lat, c, s_, frames);
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

int mpg_k_wind_vector_weights(mpg_handle_s *h, const double *src_frames, const double *dst_frames, double *m, hipStream_t s) {
  if (h->n_dst == 0 || h->nnz == 0) return MPG_SUCCESS;
  unsigned nb;
  int rc = point_grid("mpg_wind_vector_weights", h->n_dst, &nb);
  if (rc) return rc;
  k_vector_weights<<<nb, 256, 0, s>>>(h->n_dst, h->n_src, h->nnz, h->rowptr.p, h->col.p, h->val.p, src_frames, dst_frames, m);
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

// r1 == nullptr: r0 alone, from the planes m00, m01
int mpg_k_wind_vector(mpg_handle_s *h, const double *m, const void *u, const void *v, int src_type, int64_t ldu, int64_t ldv, int nlev,
                      void *r0, void *r1, int dst_type, int layout, hipStream_t s) {
  const int64_t P = h->n_dst;
  if (P == 0 || nlev == 0) return MPG_SUCCESS;
  const size_t esz = (dst_type & MPG_TYPE_F32) ? 4 : 8;
  const int nout = r1 == nullptr ? 1 : 2;
  if (h->nnz == 0) {   // every row is empty: every result is +0.0
    int rc = mpg_zero_planes(r0, esz, P, nlev, P, s);
    return rc || nout == 1 ? rc : mpg_zero_planes(r1, esz, P, nlev, P, s);
  }
  uint64_t ntile;
  int rc = am_grid("mpg_wind_vector", P, 1, &ntile);
  if (rc) return rc;
  const bool levf = layout == MPG_LAYOUT_LEV_FAST && nlev > 1;   // (a single level is the same memory in both layouts)
  const TilePlan tp = am_tile_plan(nlev, esz, levf, wv_lds_head(nout), nout);
  const WindVec a{h->rowptr.p, h->col.p, m, u, v, r0, r1, P, h->nnz, ldu, ldv, nlev, tp.kc, tp.S};
  return mpg_dispatch_types(src_type, dst_type, [&](auto ts, auto td) {
    typedef decltype(ts) TS;
    typedef decltype(td) TD;
    return nout == 2 ? launch<TS, TD, 2>(a, levf, (unsigned)ntile, tp.lds, s) : launch<TS, TD, 1>(a, levf, (unsigned)ntile, tp.lds, s);
  });
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_wind_vector() { return (const void *)&k_wind_vector<float, float, true, 2>; }
