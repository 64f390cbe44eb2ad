// Masked Regrid (mpg_regrid_masked_dev): missing sources are skipped, the valid ones stand in for them above a threshold, the
// rest of the destination -- unmapped points included -- takes a fill value.  ESMF's dynamic masking / xESMF's skipna + na_thres
// on the weights of the UNMASKED Store.  Contract in include/mpassit_amd.h; per destination point p and level k, float64:
//     valid(q)  = idx_q >= 0  and  not src_mask[idx_q]  and  src(idx_q, k) not missing
//     Wt        = w_0 + w_1 + ...                       (stored order, every stored weight)
//     Wv        = the same sum, 0.0 for every invalid entry
//     N         = the unmasked kernels' own expression (wsum3 / the fma chains of k_apply_generic_t) with weight AND
//                 value of every invalid entry replaced by 0.0 -- a missing NaN never enters a product
//     defined   = Wv > 0 and Wv >= min_valid_frac * Wt
//     dst       = defined ? (TD) fma(N * (Wt / Wv), scale, offset) : (TD) fill_value
// With no invalid entry Wv and Wt are the same bits, Wt / Wv == 1.0 and the result is the unmasked typed Regrid's, bit for bit.
// No atomics; the expression is the same in every kernel below, so the two source layouts and any nfields batching give the same bits.
//
//   k_masked_cf   fixed nnz (1 / 3 / 4), cell-fast source: the lane gather of k_apply3_cf (k_apply.hip) -- 64 x 8 row-shifted tile,
//                 indices / weights / static mask read once per tile into registers, Wt once per point; the level loop loads,
//                 tests, forms N and Wv and SELECTS the result (no branch around the store: geom.h stream_store)
//   k_masked_lf   fixed nnz, level-fast source: the row gather of k_apply3_lf -- indices (-1 = never valid) and weights staged in
//                 LDS, lanes = levels over a wave-uniform row base, results transposed through an LDS tile [64][65] doubles per
//                 chunk of 64 levels (bounded whatever nlev is), stores with lanes = points
//   k_masked_csr  CSR (conservative, mpg_handle_from_weights), both layouts: one thread per point, two levels per pass over the row
#include "apply_mesh.h"
#include "masked_par.h"   // MaskPar, mk_missing: shared with the adjoint (k_transpose_masked.hip)

// defined ? epilogue(N * Wt / Wv) : fill -- one select; Wv == Wt gives the quotient 1.0 exactly
__device__ __forceinline__ double mk_resolve(double N, double Wt, double Wv, const MaskPar &m) {
#pragma clang fp contract(off)
  const bool def = (Wv > 0.0) && (Wv >= m.frac * Wt);
  const double v = N * (Wt / Wv);
  return def ? fma(v, m.scale, m.offset) : m.fill;
}

// one (point, level): w = the point's weights with the never-valid slots already zeroed, vbits = which slots can be valid at all
template <int NNZ>
__device__ __forceinline__ double mk_point(const double (&w)[NNZ], const double (&x)[NNZ], unsigned vbits, double Wt, const MaskPar &m) {
  double wk[NNZ], xk[NNZ], Wv = 0.0;
#pragma unroll
  for (int q = 0; q < NNZ; ++q) {
    const bool ok = ((vbits >> q) & 1u) && !mk_missing(x[q], m);
    wk[q] = ok ? w[q] : 0.0;
    xk[q] = ok ? x[q] : 0.0;
    Wv = q == 0 ? wk[0] : Wv + wk[q];
  }
  double N;
  if constexpr (NNZ == 1) N = xk[0];                                              // nearest neighbour: a copy
  else if constexpr (NNZ == 3) N = wsum3(wk[0], xk[0], wk[1], xk[1], wk[2], xk[2]);   // geom.h: the pinned pattern of every bilinear kernel
  else {
    N = 0.0;
#pragma unroll
    for (int q = 0; q < NNZ; ++q) N = fma(wk[q], xk[q], N);                        // k_apply_generic_t (wsum_fixed)
  }
  return mk_resolve(N, Wt, Wv, m);
}

template <int NNZ, typename TS, typename TD>
__global__ __launch_bounds__(256) void k_masked_cf(const int32_t *__restrict__ idx, const double *__restrict__ w, const TS *__restrict__ src,
                                                   TD *__restrict__ dst, int nx, int ny, int64_t nsrc, int nlev, int ntx, int nty, int64_t ld,
                                                   MaskPar m) {
  constexpr int RPT = 2, TY = 4 * RPT;
  const int64_t P = (int64_t)nx * ny;
  const unsigned ntile = (unsigned)ntx * nty;
  const unsigned lin = xcd_remap(blockIdx.x, gridDim.x);
  const unsigned tile = lin % ntile;
  const int f = lin / ntile;
  const int tx = tile % ntx, ty = tile / ntx;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j0 = ty * TY + wave * RPT;
  int32_t c[RPT][NNZ];
  double ww[RPT][NNZ], Wt[RPT];
  unsigned vb[RPT];
  bool act[RPT];
  int64_t po[RPT];
#pragma unroll
  for (int r = 0; r < RPT; ++r) {
    const int j = j0 + r;
    const int i = tx * 64 + lane - mpg_tile_shift(j, nx);   // row-shifted tile: aligned store segments (mpg_internal.h)
    act[r] = (i >= 0) && (i < nx) && (j < ny);
    const int64_t p = act[r] ? (int64_t)j * nx + i : 0;
    po[r] = p;
    vb[r] = 0;
    Wt[r] = 0.0;
#pragma unroll
    for (int q = 0; q < NNZ; ++q) {
      const int32_t ci = idx[q * P + p];
      const double wq = NNZ == 1 ? 1.0 : w[q * P + p];
      Wt[r] = q == 0 ? wq : Wt[r] + wq;
      const int32_t cc = max(ci, 0);
      bool v0 = ci >= 0;
      if (m.mask) v0 = v0 && m.mask[cc] == 0;   // gathered once per tile
      c[r][q] = cc;
      ww[r][q] = v0 ? wq : 0.0;
      vb[r] |= v0 ? 1u << q : 0u;
    }
  }
  const TS *s = src + (int64_t)f * nlev * nsrc;
  TD *d = dst + (int64_t)f * nlev * ld;
  for (int k = 0; k < nlev; ++k) {
    __syncthreads();   // level lock-step: lines shared between neighbouring rows are still in L1 / L2 (k_apply3_cf)
    double x[RPT][NNZ], v[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r)
#pragma unroll
      for (int q = 0; q < NNZ; ++q) x[r][q] = (double)s[c[r][q]];
#pragma unroll
    for (int r = 0; r < RPT; ++r) v[r] = mk_point<NNZ>(ww[r], x[r], vb[r], Wt[r], m);
#pragma unroll
    for (int r = 0; r < RPT; ++r)
      if (act[r]) stream_store_lane((TD)v[r], d + po[r], (unsigned)lane * (unsigned)sizeof(TD));   // geom.h: per lane
    s += nsrc;
    d += ld;
  }
}

template <int NNZ, typename TS, typename TD>
__global__ __launch_bounds__(512) void k_masked_lf(const int32_t *__restrict__ idx, const double *__restrict__ w, const TS *__restrict__ src,
                                                   TD *__restrict__ dst, int nx, int ny, int64_t nsrc, int nlev, int ntx, int nty, int64_t ld,
                                                   MaskPar m) {
  constexpr int WAVES = 8, PPW = 64 / WAVES, BATCH = 4;
  __shared__ double tile[64 * 65];     // [level of the chunk][65]: row pad 1, conflict-free column writes
  __shared__ double sw[NNZ * 64];      // the stored weights as they are (Wt needs them all)
  __shared__ int32_t sidx[NNZ * 64];   // -1: no such point, unmapped slot or statically masked source -- never valid
  const int64_t P = (int64_t)nx * ny;
  const unsigned ntile = (unsigned)ntx * nty;
  const unsigned lin = xcd_remap(blockIdx.x, gridDim.x);
  const unsigned tl = lin % ntile;
  const int fld = lin / ntile;
  const int tx = tl % ntx, ty = tl / ntx;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t < NNZ * 64) {
    const int pt = t & 63, q = t >> 6;
    const int j = ty, i = tx * 64 + pt - mpg_tile_shift(j, nx);
    const bool in = i >= 0 && i < nx && j < ny;
    const int64_t p = in ? (int64_t)j * nx + i : 0;
    const int32_t ci = idx[q * P + p];
    bool v0 = in && ci >= 0;
    if (m.mask) v0 = v0 && m.mask[max(ci, 0)] == 0;
    sidx[q * 64 + pt] = v0 ? ci : -1;
    sw[q * 64 + pt] = NNZ == 1 ? 1.0 : w[q * P + p];
  }
  __syncthreads();
  const int oj = ty, oi = tx * 64 + lane - mpg_tile_shift(oj, nx);
  const bool oact = oi >= 0 && oi < nx && oj < ny;
  const int64_t op = oact ? (int64_t)oj * nx + oi : 0;
  const TS *sf = src + (int64_t)fld * nlev * nsrc;
  TD *df = dst + (int64_t)fld * nlev * ld;
  for (int kb = 0; kb < nlev; kb += 64) {
    const int kk = min(kb + lane, nlev - 1);   // lanes past the last level redo it into tile rows nobody stores
#pragma unroll
    for (int q0 = 0; q0 < PPW; q0 += BATCH) {
      double v[BATCH];
#pragma unroll
      for (int u = 0; u < BATCH; ++u) {
        const int pt = wave * PPW + q0 + u;
        double wq[NNZ], x[NNZ], Wt = 0.0;
        unsigned vb = 0;
#pragma unroll
        for (int q = 0; q < NNZ; ++q) {
          const int32_t ci = __builtin_amdgcn_readfirstlane(sidx[q * 64 + pt]);   // wave-uniform row base: one coalesced row read
          const double wr = sw[q * 64 + pt];
          Wt = q == 0 ? wr : Wt + wr;
          wq[q] = ci >= 0 ? wr : 0.0;
          vb |= ci >= 0 ? 1u << q : 0u;
          x[q] = (double)sf[(int64_t)max(ci, 0) * nlev + kk];
        }
        v[u] = mk_point<NNZ>(wq, x, vb, Wt, m);
      }
#pragma unroll
      for (int u = 0; u < BATCH; ++u) tile[lane * 65 + wave * PPW + q0 + u] = v[u];
    }
    __syncthreads();
    const int nk = min(64, nlev - kb);
    if (oact)
      for (int kl = wave; kl < nk; kl += WAVES)
        stream_store_lane((TD)tile[kl * 65 + lane], df + (int64_t)(kb + kl) * ld + op, (unsigned)lane * (unsigned)sizeof(TD));
    __syncthreads();
  }
}

template <bool LEVF, typename TS, typename TD>
__global__ __launch_bounds__(256) void k_masked_csr(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                    const double *__restrict__ val, const TS *__restrict__ src, TD *__restrict__ dst, int64_t P,
                                                    int64_t nsrc, int nlev, int nblk, int64_t ld, MaskPar m) {
  const unsigned blk = blockIdx.x % nblk;
  const int fld = blockIdx.x / nblk;
  const int64_t p = (int64_t)blk * 256 + threadIdx.x;
  if (p >= P) return;
  const int b = rowptr[p], e = rowptr[p + 1];
  double Wt = 0.0;
  for (int q = b; q < e; ++q) Wt += val[q];
  const TS *sf = src + (int64_t)fld * nlev * nsrc;
  TD *df = dst + (int64_t)fld * nlev * ld + p;
  const unsigned lb = (unsigned)(threadIdx.x & 63) * (unsigned)sizeof(TD);
  // two levels per pass over the row; an odd nlev's last pass does level nlev - 1 twice (the same bits to the same address)
  for (int k = 0; k < nlev; k += 2) {
    const int k1 = min(k + 1, nlev - 1);
    double a0 = 0.0, a1 = 0.0, wv0 = 0.0, wv1 = 0.0;
    for (int q = b; q < e; ++q) {
      const int32_t ci = col[q];
      const double wq = val[q];
      const int64_t cc = max(ci, 0);
      bool v0 = ci >= 0;
      if (m.mask) v0 = v0 && m.mask[cc] == 0;
      const double x0 = (double)(LEVF ? sf[cc * nlev + k] : sf[(int64_t)k * nsrc + cc]);
      const double x1 = (double)(LEVF ? sf[cc * nlev + k1] : sf[(int64_t)k1 * nsrc + cc]);
      const bool ok0 = v0 && !mk_missing(x0, m), ok1 = v0 && !mk_missing(x1, m);
      const double w0 = ok0 ? wq : 0.0, w1 = ok1 ? wq : 0.0;
      a0 = fma(w0, ok0 ? x0 : 0.0, a0);   // the CSR form of k_apply_generic_t: its product and sum pattern
      a1 = fma(w1, ok1 ? x1 : 0.0, a1);
      wv0 += w0;
      wv1 += w1;
    }
    stream_store_lane((TD)mk_resolve(a0, Wt, wv0, m), df + (int64_t)k * ld, lb);
    stream_store_lane((TD)mk_resolve(a1, Wt, wv1, m), df + (int64_t)k1 * ld, lb);
  }
}

// a handle that maps nothing: every point is undefined
template <typename TD>
__global__ __launch_bounds__(256) void k_masked_fill(TD *__restrict__ dst, int64_t P, int nblk, int64_t ld, double fill) {
  const int64_t p = (int64_t)(blockIdx.x % nblk) * 256 + threadIdx.x;
  if (p < P) dst[(int64_t)(blockIdx.x / nblk) * ld + p] = (TD)fill;
}

template <typename TS, typename TD>
static int launch_masked(mpg_handle_s *h, const void *src_v, int lev_fast, int nlev, int nfields, void *dst_v, int64_t ld, const MaskPar &m,
                         hipStream_t s) {
  const TS *src = (const TS *)src_v;
  TD *dst = (TD *)dst_v;
  const int64_t P = h->n_dst;
  if (h->kind == MPG_KIND_CSR) {
    const int nblk = (int)((P + 255) / 256);
    if (lev_fast) k_masked_csr<true, TS, TD><<<(unsigned)nblk * nfields, 256, 0, s>>>(h->rowptr.p, h->col.p, h->val.p, src, dst, P, h->n_src, nlev, nblk, ld, m);
    else k_masked_csr<false, TS, TD><<<(unsigned)nblk * nfields, 256, 0, s>>>(h->rowptr.p, h->col.p, h->val.p, src, dst, P, h->n_src, nlev, nblk, ld, m);
    MPG_HIP(hipGetLastError());
    return MPG_SUCCESS;
  }
  int nx = h->nx_dst, ny = h->ny_dst;
  if ((int64_t)nx * ny != P) {   // a handle without a 2-D shape: one row
    nx = (int)P;
    ny = 1;
  }
  const int ntx = mpg_tile_ntx(nx, 64);
#define MASKED_FIXED(NNZ)                                                                                                                     \
  do {                                                                                                                                        \
    if (lev_fast) k_masked_lf<NNZ, TS, TD><<<(unsigned)ntx * ny * nfields, 512, 0, s>>>(h->idx.p, h->w.p, src, dst, nx, ny, h->n_src, nlev, ntx, ny, ld, m); \
    else k_masked_cf<NNZ, TS, TD><<<(unsigned)ntx * ((ny + 7) / 8) * nfields, 256, 0, s>>>(h->idx.p, h->w.p, src, dst, nx, ny, h->n_src, nlev, ntx, (ny + 7) / 8, ld, m); \
  } while (0)
  if (h->nnz_per_row == 3) MASKED_FIXED(3);
  else if (h->nnz_per_row == 4) MASKED_FIXED(4);
  else if (h->nnz_per_row == 1) MASKED_FIXED(1);
  else {
    mpg_set_error("mpg_regrid_masked: unsupported handle (%d weights per row)", h->nnz_per_row);
    return MPG_ERR_UNSUPPORTED;
  }
#undef MASKED_FIXED
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

int mpg_k_apply_masked(mpg_handle_s *h, const void *src, int src_type, int layout, int nlev, int nfields, void *dst, int dst_type, int64_t ld,
                       const mpg_mask_opts *o, hipStream_t s) {
  const int64_t P = h->n_dst;
  if (P == 0 || nlev == 0 || nfields == 0) return MPG_SUCCESS;
  if (ld == 0) ld = P;
  if (h->n_src == 0) {
    const int nblk = (int)((P + 255) / 256);
    const unsigned nwg = (unsigned)nblk * (unsigned)(nlev * nfields);
    if (dst_type & MPG_TYPE_F32) k_masked_fill<float><<<nwg, 256, 0, s>>>((float *)dst, P, nblk, ld, o->fill_value);
    else k_masked_fill<double><<<nwg, 256, 0, s>>>((double *)dst, P, nblk, ld, o->fill_value);
    MPG_HIP(hipGetLastError());
    return MPG_SUCCESS;
  }
  MaskPar m;
  m.mask = o->src_mask_dev;
  m.missing = o->missing_value;
  m.frac = o->min_valid_frac;
  m.fill = o->fill_value;
  m.scale = o->scale;
  m.offset = o->offset;
  m.use_nan = (o->flags & MPG_MISSING_NAN) != 0;
  m.use_val = (o->flags & MPG_MISSING_VALUE) != 0;
  const int lev_fast = layout == MPG_LAYOUT_LEV_FAST && nlev > 1;   // (a single level is the same memory in both layouts)
  return mpg_dispatch_types(src_type, dst_type, [&](auto ts, auto td) {   // (apply_mesh.h)
    return launch_masked<decltype(ts), decltype(td)>(h, src, lev_fast, nlev, nfields, dst, ld, m, s);
  });
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_apply_masked() { return (const void *)&k_masked_cf<3, float, float>; }
