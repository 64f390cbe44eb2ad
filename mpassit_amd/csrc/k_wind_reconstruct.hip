// Winds from the edge-normal u a mesh carries (mpg_reconstruct_store, mpg_reconstruct_weights_dev, mpg_wind_reconstruct_dev): MPAS's
// mpas_reconstruct.  At cell c the Cartesian wind is V(k, c) = sum_i coeffs_reconstruct(:, i, c) * u(k, edgesOnCell(i, c)), projected on
// the cell's frame (east / north, or turned) or left as X / Y / Z.  The coefficients do not depend on the level, so the projection folds
// into NOUT (2 or 3) values per entry q of the CSR pattern of edgesOnCell, computed once per (handle, coefficients, frames) by
// k_reconstruct_weights; the hot path is k_wind_reconstruct, per (cell, level, k < NOUT):
//   acc_k = fma(m_k[q], (double)u[col[q]], acc_k)   from 0.0, the row's entries in stored order, whatever LDS chunk an entry arrives in
//   store (TD) fma(acc_k, 1.0, 0.0)                 one rounding to the destination type; an empty row gives (TD)(+0.0)
// Result k is bit for bit mpg_regrid_csr_to_mesh_dev of a from-weights handle with the values m_k at scale 1 and offset 0; col is staged
// once and u gathered once for all NOUT of them.
//
// A 256-thread workgroup owns AM_CELLS consecutive cells in xcd_remap block order; col and the NOUT planes of its 64 rows are staged
// through LDS as ONE run (apply_mesh.h CsrRunN), WR_CHUNK entries at a time.  A row's sum is sequential in every branch, so no bit
// depends on the layouts, on WR_LB, WR_UNROLL, WR_CHUNK or on the chunking.
//   [lev][edge] sources (SROWS false): k_wind_vector's shape with ONE gather per entry and level.  Lanes run along rows, wave w takes
//     levels w, w + 4, ..., WR_LB at a time: NOUT x WR_LB independent fma chains per lane.  Entries are walked in pairs, the next
//     pair's gathers issued ahead of this pair's fmas.  [lev][cell] results go straight out, [cell][lev] results through NOUT LDS tiles
//     and am_drain_tile.
//   [edge][lev] sources (SROWS true; MPAS file order, the production path): k_apply_csr_rows's shape.  Threads run along the block's
//     [cell][lev] run (RunCursor), so the lanes of a cell gather consecutive levels of the same source row; WR_UNROLL elements per thread
//     with NOUT accumulators each.  [cell][lev] results ARE that run and leave as one contiguous piece per output; [lev][cell] results
//     are written to an LDS tile per output along their rows and drained along their columns, a whole 64-cell segment per level.
// Tiles are am_tile_plan's: [cell][S], S odd (a wave's column accesses hit distinct banks), NOUT of them within AM_TILE_BYTES, in level
// chunks when all levels do not fit.
// Offsets are 64-bit: col * nlev + k ([edge][lev] sources), k * ld + col ([lev][edge] sources), k * P + p and p * nlev + k (results).
// LDS: an entry takes 4 + 8 NOUT bytes, at most 28.  WR_CHUNK = 512 entries and the row pointers are 512 * 28 + 272 = 14 608 bytes in
// front of at most 65 536 bytes of tiles: 80 144 bytes at worst, below the 81 920 that let two workgroups share the 160 KB of a CU whatever
// the level count.  At 55 levels and 3 float64 outputs the tiles are 3 x 64 x 33 x 8 = 50 688 bytes (level chunks of 32): 65 296 in all.
// No atomics, no allocation, no synchronisation with the host: the calls are capturable in a hipGraph from the first call.
#pragma clang fp contract(off)
#include "apply_mesh.h"
#include "wind_reconstruct_checks.h"   // WR_LB, WR_UNROLL, WR_CHUNK, WR_RP, wr_lds_head: shared with the host-side checks

static_assert(WR_ROWS == AM_CELLS, "the checks count the launch's blocks in AM_CELLS rows");

// ---- blocks -----------------------------------------------------------------------------------------------------------------------------
// One thread per row: m[nout][nnz] in the handle's entry order; slot i of row c reads coeffs[c][i][:].  df == nullptr: X, Y, Z.
// A set-up kernel: it runs once per (handle, coefficients, frames).
__global__ __launch_bounds__(256) void k_reconstruct_weights(int64_t P, int64_t nnz, int maxEdges, const int32_t *__restrict__ rowptr,
                                                             const double *__restrict__ val, const double *__restrict__ coeffs,
                                                             const double *__restrict__ df, double *__restrict__ m) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  double d0[3] = {0.0, 0.0, 0.0}, d1[3] = {0.0, 0.0, 0.0};
  if (df != nullptr) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      d0[k] = df[k * P + p];
      d1[k] = df[(3 + k) * P + p];
    }
  }
  const int qb = rowptr[p], qe = rowptr[p + 1];
  const double *cf = coeffs + p * (int64_t)maxEdges * 3;
  for (int q = qb; q < qe; ++q) {
    const double w = val[q];
    const double *c = cf + (int64_t)(q - qb) * 3;
    const double cx = c[0], cy = c[1], cz = c[2];
    if (df != nullptr) {
      m[q] = w * ((cx * d0[0] + cy * d0[1]) + cz * d0[2]);
      m[nnz + q] = w * ((cx * d1[0] + cy * d1[1]) + cz * d1[2]);
    } else {
      m[q] = w * cx;
      m[nnz + q] = w * cy;
      m[2 * nnz + q] = w * cz;
    }
  }
}

// ---- the apply --------------------------------------------------------------------------------------------------------------------------
struct WindRec {
  const int32_t *rp;      // [P + 1] row pointers
  const int32_t *col;     // [nnz]
  const double *m;        // [NOUT][nnz]
  const void *u;          // [nlev] planes ld elements apart, or [n_src][nlev]
  void *r[3];             // nlev * P each, [lev][cell] or [cell][lev]; r[2] only touched with NOUT 3
  int64_t P, nnz, ld;
  int nlev, kc, S;
};

// SROWS: the source is [edge][lev]; DROWS: the results are [cell][lev].  Tiles where SROWS != DROWS.
template <typename TS, typename TD, bool SROWS, bool DROWS, int NOUT>
__global__ __launch_bounds__(256) void k_wind_reconstruct(WindRec a) {
  extern __shared__ double sval[];                     // sval[NOUT][WR_CHUNK] | scol[WR_CHUNK] | srp[WR_RP] | NOUT x tile[64][S]
  int32_t *scol = (int32_t *)(sval + NOUT * WR_CHUNK);
  int32_t *srp = scol + WR_CHUNK;
  TD *tile = (TD *)(srp + WR_RP);
  const unsigned tl = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t P = a.P, p0 = (int64_t)tl * AM_CELLS;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nlev = a.nlev, S = a.S, kc = a.kc;
  const int TSZ = AM_CELLS * S;                        // elements of one tile
  const CsrRunN<NOUT, WR_CHUNK> run = am_csr_run_n<NOUT, WR_CHUNK>(a.rp, a.col, a.m, a.nnz, P, p0, t, srp, scol, sval);
  const TS *su = (const TS *)a.u;
  TD *d[NOUT];
#pragma unroll
  for (int i = 0; i < NOUT; ++i) d[i] = (TD *)a.r[i];
  const int ncell = (int)min((int64_t)AM_CELLS, P - p0);
  if constexpr (!SROWS) {
    const int rb = srp[lane], re = srp[lane + 1];
    const bool in = p0 + lane < P;
    const int64_t ld = a.ld;
    for (int k0 = 0; k0 < nlev; k0 += kc) {
      const int kn = min(kc, nlev - k0);
      for (int kb = 0; kb < kn; kb += 4 * WR_LB) {
        double acc[NOUT][WR_LB];
        const TS *pu[WR_LB];
#pragma unroll
        for (int j = 0; j < WR_LB; ++j) {
          const int k = kb + wave + 4 * j;
          const int64_t lev = k0 + (k < kn ? k : 0);      // a level slot past the chunk gathers level k0 and stores nothing
#pragma unroll
          for (int i = 0; i < NOUT; ++i) acc[i][j] = 0.0;
          pu[j] = su + lev * ld;
        }
        for (int ch = 0; ch < run.nchunk; ++ch) {
          const int qa = run.enter(ch);
          const int b = max(rb, qa), e = min(re - qa, WR_CHUNK) + qa;
          // entries in pairs: the WR_LB gathers of each in flight together, and the next pair's issued ahead of this pair's fmas
          auto gather = [&](int q, TS *x) {
            const int32_t cc = scol[q - qa];
#pragma unroll
            for (int j = 0; j < WR_LB; ++j) x[j] = pu[j][cc];
          };
          auto widen = [](const TS *x, double *y) {
#pragma unroll
            for (int j = 0; j < WR_LB; ++j) y[j] = (double)x[j];
          };
          auto add = [&](int q, const double *y) {   // entry q into every chain, in stored order
            double w[NOUT];
#pragma unroll
            for (int i = 0; i < NOUT; ++i) w[i] = sval[i * WR_CHUNK + q - qa];
#pragma unroll
            for (int j = 0; j < WR_LB; ++j) {
#pragma unroll
              for (int i = 0; i < NOUT; ++i) acc[i][j] = fma(w[i], y[j], acc[i][j]);
            }
          };
          TS x0[WR_LB], x1[WR_LB];
          if (b < e) gather(b, x0);
          if (b + 1 < e) gather(b + 1, x1);
          for (int q = b; q < e; q += 2) {
            double y0[WR_LB], y1[WR_LB];
            const bool two = q + 1 < e;
            widen(x0, y0);
            if (two) widen(x1, y1);
            if (q + 2 < e) gather(q + 2, x0);
            if (q + 3 < e) gather(q + 3, x1);
            add(q, y0);
            if (two) add(q + 1, y1);
          }
        }
#pragma unroll
        for (int j = 0; j < WR_LB; ++j) {
          const int k = kb + wave + 4 * j;
          if (k < kn) {
#pragma unroll
            for (int i = 0; i < NOUT; ++i) {
              // fma(x, 1.0, 0.0): the epilogue of mpg_regrid_csr_to_mesh_dev at scale 1, offset 0 (a -0.0 sum becomes +0.0 there too)
              const TD r = (TD)fma(acc[i][j], 1.0, 0.0);
              if (DROWS) {
                tile[i * TSZ + lane * S + k] = r;
              } else if (in) {
                stream_store_lane(r, d[i] + ((int64_t)(k0 + k) * P + p0 + lane), (unsigned)lane * (unsigned)sizeof(TD));
              }
            }
          }
        }
      }
      if (DROWS) {
#pragma unroll
        for (int i = 0; i < NOUT; ++i) am_drain_tile(tile + i * TSZ, S, d[i], p0, k0, ncell, kn, nlev, t, lane);
        if (k0 + kc < nlev) __syncthreads();   // the next chunk overwrites the tiles
      }
    }
  } else {
    for (int k0 = 0; k0 < nlev; k0 += kc) {   // (one chunk of all levels for [cell][lev] results)
      const int kn = min(kc, nlev - k0);
      const int total = ncell * kn;
      RunCursor cur(t, kn);
      for (int e0 = 0; e0 < total; e0 += WR_UNROLL * 256) {   // (workgroup-uniform: every thread meets the barriers of enter())
        double acc[WR_UNROLL][NOUT];
        int rb[WR_UNROLL], re[WR_UNROLL], at[WR_UNROLL];
        const TS *ps[WR_UNROLL];
#pragma unroll
        for (int v = 0; v < WR_UNROLL; ++v) {
          const bool ok = e0 + t + v * 256 < total;   // an element past the run's end walks an empty row and stores nothing
#pragma unroll
          for (int i = 0; i < NOUT; ++i) acc[v][i] = 0.0;
          rb[v] = ok ? srp[cur.cc] : 0;
          re[v] = ok ? srp[cur.cc + 1] : 0;
          ps[v] = su + (ok ? k0 + cur.kk : 0);
          at[v] = cur.cc * S + cur.kk;                // (its place in a [cell][S] tile)
          cur.next();
        }
        for (int ch = 0; ch < run.nchunk; ++ch) {
          const int qa = run.enter(ch);
          // this chunk's part of every element's row, as positions in the staged chunk: [b, b + n)
          int b[WR_UNROLL], n[WR_UNROLL], nmax = 0;
#pragma unroll
          for (int v = 0; v < WR_UNROLL; ++v) {
            b[v] = max(rb[v], qa) - qa;
            n[v] = min(re[v] - qa, WR_CHUNK) - b[v];
            nmax = max(nmax, n[v]);
          }
          for (int i = 0; i < nmax; ++i) {
#pragma unroll
            for (int v = 0; v < WR_UNROLL; ++v)
              if (i < n[v]) {
                const double x = (double)ps[v][(int64_t)scol[b[v] + i] * nlev];
#pragma unroll
                for (int o = 0; o < NOUT; ++o) acc[v][o] = fma(sval[o * WR_CHUNK + b[v] + i], x, acc[v][o]);
              }
          }
        }
#pragma unroll
        for (int v = 0; v < WR_UNROLL; ++v) {
          const int e = e0 + t + v * 256;
          if (e < total) {
#pragma unroll
            for (int o = 0; o < NOUT; ++o) {
              const TD r = (TD)fma(acc[v][o], 1.0, 0.0);
              if (DROWS) stream_store_lane(r, d[o] + (p0 * nlev + e), (unsigned)lane * (unsigned)sizeof(TD));   // (kn == nlev: the block's run)
              else tile[o * TSZ + at[v]] = r;
            }
          }
        }
      }
      if (!DROWS) {
        // level k0 + k of every tile leaves as the block's 64-cell segment of that level's plane; wave w takes levels w, w + 4, ...
        __syncthreads();
        for (int k = wave; k < kn; k += 4) {
          if (lane < ncell) {
            const int64_t off = (int64_t)(k0 + k) * P + p0 + lane;
#pragma unroll
            for (int o = 0; o < NOUT; ++o)
              stream_store_lane(tile[o * TSZ + lane * S + k], d[o] + off, (unsigned)lane * (unsigned)sizeof(TD));
          }
        }
        if (k0 + kc < nlev) __syncthreads();   // the next chunk overwrites the tiles
      }
    }
  }
}

template <typename TS, typename TD, int NOUT>
static int launch(const WindRec &a, bool srows, bool drows, unsigned ntile, size_t lds, hipStream_t s) {
  auto fn = srows ? (drows ? k_wind_reconstruct<TS, TD, true, true, NOUT> : k_wind_reconstruct<TS, TD, true, false, NOUT>)
                  : (drows ? k_wind_reconstruct<TS, TD, false, true, NOUT> : k_wind_reconstruct<TS, TD, false, false, NOUT>);
  int rc = am_allow_lds((const void *)fn, lds);
  if (rc) return rc;
  fn<<<ntile, 256, lds, s>>>(a);
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

// The API entry points have checked their arguments.
int mpg_k_reconstruct_weights(mpg_handle_s *h, int maxEdges, const double *coeffs, const double *dst_frames, double *m, hipStream_t s) {
  if (h->n_dst == 0 || h->nnz == 0) return MPG_SUCCESS;
  const uint64_t nb = ((uint64_t)h->n_dst + 255) / 256;
  if (nb > 0x7fffffffull) {
    mpg_set_error("mpg_reconstruct_weights: %lld cells exceed one launch", (long long)h->n_dst);
    return MPG_ERR_OVERFLOW;
  }
  k_reconstruct_weights<<<(unsigned)nb, 256, 0, s>>>(h->n_dst, h->nnz, maxEdges, h->rowptr.p, h->val.p, coeffs, dst_frames, m);
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

int mpg_k_wind_reconstruct(mpg_handle_s *h, const double *m, int nout, const void *u, int src_type, int src_layout, int64_t ldu, int nlev,
                           void *r0, void *r1, void *r2, int dst_type, int dst_layout, hipStream_t s) {
  const int64_t P = h->n_dst;
  if (P == 0 || nlev == 0) return MPG_SUCCESS;
  const size_t esz = (dst_type & MPG_TYPE_F32) ? 4 : 8;
  void *r[3] = {r0, r1, r2};
  if (h->nnz == 0) {   // every row is empty: every result is +0.0
    for (int i = 0; i < nout; ++i) {
      int rc = mpg_zero_planes(r[i], esz, P, nlev, P, s);
      if (rc) return rc;
    }
    return MPG_SUCCESS;
  }
  uint64_t ntile;
  int rc = am_grid("mpg_wind_reconstruct", P, 1, &ntile);
  if (rc) return rc;
  // (a single level is the same memory in both layouts, on either side)
  const bool srows = src_layout == MPG_LAYOUT_LEV_FAST && nlev > 1, drows = dst_layout == MPG_LAYOUT_LEV_FAST && nlev > 1;
  const TilePlan tp = am_tile_plan(nlev, esz, srows != drows, wr_lds_head(nout), nout);
  const WindRec a{h->rowptr.p, h->col.p, m, u, {r0, r1, r2}, P, h->nnz, ldu, nlev, tp.kc, tp.S};
  return mpg_dispatch_types(src_type, dst_type, [&](auto ts, auto td) {
    typedef decltype(ts) TS;
    typedef decltype(td) TD;
    return nout == 3 ? launch<TS, TD, 3>(a, srows, drows, (unsigned)ntile, tp.lds, s) : launch<TS, TD, 2>(a, srows, drows, (unsigned)ntile, tp.lds, s);
  });
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_wind_reconstruct() { return (const void *)&k_wind_reconstruct<float, float, true, false, 2>; }
