// The adjoint of the masked Regrid (mpg_regrid_masked_transpose_dev): the derivative of mpg_regrid_masked_dev with respect to every
// valid source element, exactly +0.0 at every invalid one.  Contract in include/mpassit_amd.h; per destination point p, source c and
// level k, float64, nothing contracted (the pragma below holds for the whole file; the segment sum is explicit fma, transpose_seg.h):
//     valid(q), Wt, Wv, defined   those of the forward, word for word (k_apply_masked.hip: same order, same expressions)
//     h[k][p]   = defined ? ((double)g[k][p] * scale) * (Wt / Wv) : +0.0     a SELECT: a NaN of g at an undefined point reaches no source
//     acc       = fma(w_j, h[k][row_j], acc) from +0.0 over the transposed segment of c (mpg_regrid_transpose_dev's chain)
//     dst[c][k] = src_mask[c] == 0 and src(c, k) not missing ? (TD) acc : +0.0
// Two passes in stream order, no atomics:
//   pass 1, h into the caller's workspace [nfields][nlev][n_dst] float64 -- shaped like the forward, the source is read for validity only:
//     k_mratio_cf   fixed nnz (1 / 3 / 4), cell-fast source: the 64 x 8 row-shifted tile of k_masked_cf, indices / weights / static mask
//                   once per tile into registers, Wt once per point
//     k_mratio_lf   fixed nnz, level-fast source: indices (-1 = never valid) and weights staged in LDS, lanes = levels over a
//                   wave-uniform row base; Wv crosses an LDS tile [64][65] per chunk of 64 levels, g is read and h stored with lanes = points
//     k_mratio_csr  CSR, both layouts: one thread per point, two levels per pass over the row
//   pass 2, the transposed gathers of k_transpose.hip over h, each with one coalesced load of src(c, k) in the output's own layout, the
//   static-mask byte and the select at the store:
//     k_trm_short_cf / k_trm_short_lf   one lane per source, segment in registers (in the level-fast form the validity load rides the
//                                       drain loop of the LDS tile, which already runs along [cell][lev])
//     k_trm_long                        one wave per listed source, lanes = levels
#include <algorithm>

#include "apply_mesh.h"
#include "masked_par.h"
#pragma clang fp contract(off)
#include "transpose_seg.h"

#define TRM_LF_CELLS 64
#define TRM_LF_LEVS 64

// ---- pass 1 -----------------------------------------------------------------------------------------------------------------------
// Wv of one (point, level): w = the point's weights with the never-valid slots already zeroed (mk_point's sum, k_apply_masked.hip)
template <int NNZ>
__device__ __forceinline__ double mr_wv(const double (&w)[NNZ], const double (&x)[NNZ], unsigned vbits, const MaskPar &m) {
  double Wv = 0.0;
#pragma unroll
  for (int q = 0; q < NNZ; ++q) {
    const bool ok = ((vbits >> q) & 1u) && !mk_missing(x[q], m);
    const double wk = ok ? w[q] : 0.0;
    Wv = q == 0 ? wk : Wv + wk;
  }
  return Wv;
}
// defined ? (g * scale) * (Wt / Wv) : +0.0 -- the decision is mk_resolve's; two separately rounded products, one select
__device__ __forceinline__ double mr_h(double g, double Wt, double Wv, const MaskPar &m) {
  const bool def = (Wv > 0.0) && (Wv >= m.frac * Wt);
  const double v = (g * m.scale) * (Wt / Wv);
  return def ? v : 0.0;
}

template <int NNZ, typename TS, typename TG>
__global__ __launch_bounds__(256) void k_mratio_cf(const int32_t *__restrict__ idx, const double *__restrict__ w, const TS *__restrict__ src,
                                                   const TG *__restrict__ g, double *__restrict__ h, int nx, int ny, int64_t nsrc, int nlev, int ntx,
                                                   int nty, int64_t ldg, MaskPar m) {
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
    const int i = tx * 64 + lane - mpg_tile_shift(j, nx);
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
  const TG *gf = g + (int64_t)f * nlev * ldg;
  double *d = h + (int64_t)f * nlev * P;
  for (int k = 0; k < nlev; ++k) {
    __syncthreads();   // level lock-step, as k_masked_cf
    double x[RPT][NNZ], gv[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
#pragma unroll
      for (int q = 0; q < NNZ; ++q) x[r][q] = (double)s[c[r][q]];
      gv[r] = (double)gf[po[r]];
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r)
      if (act[r]) d[po[r]] = mr_h(gv[r], Wt[r], mr_wv<NNZ>(ww[r], x[r], vb[r], m), m);   // plain stores: pass 2 reads h next
    s += nsrc;
    gf += ldg;
    d += P;
  }
}

template <int NNZ, typename TS, typename TG>
__global__ __launch_bounds__(512) void k_mratio_lf(const int32_t *__restrict__ idx, const double *__restrict__ w, const TS *__restrict__ src,
                                                   const TG *__restrict__ g, double *__restrict__ h, int nx, int ny, int64_t nsrc, int nlev, int ntx,
                                                   int nty, int64_t ldg, MaskPar m) {
  constexpr int WAVES = 8, PPW = 64 / WAVES, BATCH = 4;
  __shared__ double tile[64 * 65];     // Wv [level of the chunk][65]: row pad 1, conflict-free column writes
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
  double oWt = 0.0;   // the drain's lanes are points: this lane's Wt, the forward's left-to-right sum
#pragma unroll
  for (int q = 0; q < NNZ; ++q) oWt = q == 0 ? sw[lane] : oWt + sw[q * 64 + lane];
  const TS *sf = src + (int64_t)fld * nlev * nsrc;
  const TG *gf = g + (int64_t)fld * nlev * ldg;
  double *hf = h + (int64_t)fld * nlev * P;
  for (int kb = 0; kb < nlev; kb += 64) {
    const int kk = min(kb + lane, nlev - 1);   // lanes past the last level redo it into tile rows nobody reads
#pragma unroll
    for (int q0 = 0; q0 < PPW; q0 += BATCH) {
      double v[BATCH];
#pragma unroll
      for (int u = 0; u < BATCH; ++u) {
        const int pt = wave * PPW + q0 + u;
        double wq[NNZ], x[NNZ];
        unsigned vb = 0;
#pragma unroll
        for (int q = 0; q < NNZ; ++q) {
          const int32_t ci = __builtin_amdgcn_readfirstlane(sidx[q * 64 + pt]);   // wave-uniform row base: one coalesced row read
          const double wr = sw[q * 64 + pt];
          wq[q] = ci >= 0 ? wr : 0.0;
          vb |= ci >= 0 ? 1u << q : 0u;
          x[q] = (double)sf[(int64_t)max(ci, 0) * nlev + kk];
        }
        v[u] = mr_wv<NNZ>(wq, x, vb, m);
      }
#pragma unroll
      for (int u = 0; u < BATCH; ++u) tile[lane * 65 + wave * PPW + q0 + u] = v[u];
    }
    __syncthreads();
    const int nk = min(64, nlev - kb);
    if (oact)
      for (int kl = wave; kl < nk; kl += WAVES) {
        const double gv = (double)gf[(int64_t)(kb + kl) * ldg + op];
        hf[(int64_t)(kb + kl) * P + op] = mr_h(gv, oWt, tile[kl * 65 + lane], m);
      }
    __syncthreads();
  }
}

template <bool LEVF, typename TS, typename TG>
__global__ __launch_bounds__(256) void k_mratio_csr(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                    const double *__restrict__ val, const TS *__restrict__ src, const TG *__restrict__ g,
                                                    double *__restrict__ h, int64_t P, int64_t nsrc, int nlev, int nblk, int64_t ldg, MaskPar m) {
  const unsigned blk = blockIdx.x % nblk;
  const int fld = blockIdx.x / nblk;
  const int64_t p = (int64_t)blk * 256 + threadIdx.x;
  if (p >= P) return;
  const int b = rowptr[p], e = rowptr[p + 1];
  double Wt = 0.0;
  for (int q = b; q < e; ++q) Wt += val[q];
  const TS *sf = src + (int64_t)fld * nlev * nsrc;
  const TG *gf = g + (int64_t)fld * nlev * ldg + p;
  double *hf = h + (int64_t)fld * nlev * P + p;
  // two levels per pass over the row; an odd nlev's last pass does level nlev - 1 twice (the same bits to the same address)
  for (int k = 0; k < nlev; k += 2) {
    const int k1 = min(k + 1, nlev - 1);
    double wv0 = 0.0, wv1 = 0.0;
    for (int q = b; q < e; ++q) {
      const int32_t ci = col[q];
      const double wq = val[q];
      const int64_t cc = max(ci, 0);
      bool v0 = ci >= 0;
      if (m.mask) v0 = v0 && m.mask[cc] == 0;
      const double x0 = (double)(LEVF ? sf[cc * nlev + k] : sf[(int64_t)k * nsrc + cc]);
      const double x1 = (double)(LEVF ? sf[cc * nlev + k1] : sf[(int64_t)k1 * nsrc + cc]);
      wv0 += (v0 && !mk_missing(x0, m)) ? wq : 0.0;
      wv1 += (v0 && !mk_missing(x1, m)) ? wq : 0.0;
    }
    hf[(int64_t)k * P] = mr_h((double)gf[(int64_t)k * ldg], Wt, wv0, m);
    hf[(int64_t)k1 * P] = mr_h((double)gf[(int64_t)k1 * ldg], Wt, wv1, m);
  }
}

// ---- pass 2 -----------------------------------------------------------------------------------------------------------------------
// cell-fast: src / dst [f][lev][cell]; 256 consecutive sources per workgroup, every level
template <typename TS, typename TD>
__global__ __launch_bounds__(256) void k_trm_short_cf(const int32_t *__restrict__ ptr, const int32_t *__restrict__ rows, const double *__restrict__ wts,
                                                      const double *__restrict__ h, const TS *__restrict__ src, TD *__restrict__ dst, int64_t n_src,
                                                      int64_t P, int nlev, int nblk, MaskPar m) {
  const int blk = blockIdx.x % nblk, f = blockIdx.x / nblk;
  const int64_t c = (int64_t)blk * 256 + threadIdx.x;
  int32_t r[TR_SHORT];
  double w[TR_SHORT];
  const int n = tr_load_seg<double>(ptr, rows, wts, c, c < n_src, r, w);
  const int nmax = tr_wave_max(n);
  if (c >= n_src) return;
  const bool use = !(m.mask && m.mask[c] != 0);
  const double *hf = h + (int64_t)f * nlev * P;
  const TS *sf = src + (int64_t)f * nlev * n_src + c;
  TD *df = dst + (int64_t)f * nlev * n_src + c;
#pragma unroll 2
  for (int k = 0; k < nlev; ++k) {
    const double x = (double)sf[(int64_t)k * n_src];
    const double acc = tr_seg_regs<double>(r, w, n, nmax, hf + (int64_t)k * P);
    df[(int64_t)k * n_src] = (use && !mk_missing(x, m)) ? (TD)acc : (TD)0.0;
  }
}

// level-fast: src / dst [f][cell][lev]; a tile of TRM_LF_CELLS sources, levels in chunks of TRM_LF_LEVS through LDS (k_tr_short_lf)
template <typename TS, typename TD>
__global__ __launch_bounds__(256) void k_trm_short_lf(const int32_t *__restrict__ ptr, const int32_t *__restrict__ rows, const double *__restrict__ wts,
                                                      const double *__restrict__ h, const TS *__restrict__ src, TD *__restrict__ dst, int64_t n_src,
                                                      int64_t P, int nlev, int ntile, MaskPar m) {
  __shared__ TD tile[TRM_LF_CELLS][TRM_LF_LEVS + 1];
  const int t = blockIdx.x % ntile, f = blockIdx.x / ntile;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t c0 = (int64_t)t * TRM_LF_CELLS, c = c0 + lane;
  const int ncell = (int)std::min<int64_t>(TRM_LF_CELLS, n_src - c0);
  int32_t r[TR_SHORT];
  double w[TR_SHORT];
  const int n = tr_load_seg<double>(ptr, rows, wts, c, c < n_src, r, w);
  const int nmax = tr_wave_max(n);
  const double *hf = h + (int64_t)f * nlev * P;
  const TS *sf = src + ((int64_t)f * n_src + c0) * nlev;
  TD *df = dst + ((int64_t)f * n_src + c0) * nlev;
  for (int k0 = 0; k0 < nlev; k0 += TRM_LF_LEVS) {
    const int kc = std::min(TRM_LF_LEVS, nlev - k0);
    for (int kk = wv; kk < kc; kk += 4) tile[lane][kk] = (TD)tr_seg_regs<double>(r, w, n, nmax, hf + (int64_t)(k0 + kk) * P);
    __syncthreads();
    const int tot = ncell * kc;
    for (int e = threadIdx.x; e < tot; e += 256) {
      const int cc = e / kc, kk = e - cc * kc;
      const int64_t at = (int64_t)cc * nlev + k0 + kk;
      const double x = (double)sf[at];   // the same consecutive [cell][lev] elements as the store
      const bool use = !(m.mask && m.mask[c0 + cc] != 0);
      df[at] = (use && !mk_missing(x, m)) ? tile[cc][kk] : (TD)0.0;
    }
    __syncthreads();
  }
}

// one wave per listed (long) source, lanes = levels
template <typename TS, typename TD, bool LEVF>
__global__ __launch_bounds__(256) void k_trm_long(const int32_t *__restrict__ ptr, const int32_t *__restrict__ rows, const double *__restrict__ wts,
                                                  const int32_t *__restrict__ lng, int nlong, int ngrp, const double *__restrict__ h,
                                                  const TS *__restrict__ src, TD *__restrict__ dst, int64_t n_src, int64_t P, int nlev, MaskPar m) {
  const int g = blockIdx.x % ngrp, f = blockIdx.x / ngrp;
  const int li = g * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (li >= nlong) return;
  const int64_t c = lng[li];
  const int32_t b = ptr[c], e = ptr[c + 1];
  const bool use = !(m.mask && m.mask[c] != 0);
  const double *hf = h + (int64_t)f * nlev * P;
  const TS *sf = src + (int64_t)f * nlev * n_src;
  TD *df = dst + (int64_t)f * nlev * n_src;
  for (int k = lane; k < nlev; k += 64) {
    const int64_t at = LEVF ? c * nlev + k : (int64_t)k * n_src + c;
    const double x = (double)sf[at];
    const double v = tr_seg_mem<double>(rows, wts, b, e, hf + (int64_t)k * P);
    df[at] = (use && !mk_missing(x, m)) ? (TD)v : (TD)0.0;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
template <typename TS, typename TG>
static int launch_mratio(mpg_handle_s *h, const void *src_v, bool levf, int nlev, int nfields, const void *g_v, int64_t ldg, double *work,
                         const MaskPar &m, hipStream_t s) {
  const TS *src = (const TS *)src_v;
  const TG *g = (const TG *)g_v;
  const int64_t P = h->n_dst;
  if (h->kind == MPG_KIND_CSR) {
    const int nblk = (int)((P + 255) / 256);
    if (levf) k_mratio_csr<true, TS, TG><<<(unsigned)nblk * nfields, 256, 0, s>>>(h->rowptr.p, h->col.p, h->val.p, src, g, work, P, h->n_src, nlev, nblk, ldg, m);
    else k_mratio_csr<false, TS, TG><<<(unsigned)nblk * nfields, 256, 0, s>>>(h->rowptr.p, h->col.p, h->val.p, src, g, work, P, h->n_src, nlev, nblk, ldg, m);
    MPG_HIP(hipGetLastError());
    return MPG_SUCCESS;
  }
  int nx = h->nx_dst, ny = h->ny_dst;
  if ((int64_t)nx * ny != P) {   // a handle without a 2-D shape: one row
    nx = (int)P;
    ny = 1;
  }
  const int ntx = mpg_tile_ntx(nx, 64);
#define MRATIO_FIXED(NNZ)                                                                                                                     \
  do {                                                                                                                                        \
    if (levf) k_mratio_lf<NNZ, TS, TG><<<(unsigned)ntx * ny * nfields, 512, 0, s>>>(h->idx.p, h->w.p, src, g, work, nx, ny, h->n_src, nlev, ntx, ny, ldg, m); \
    else k_mratio_cf<NNZ, TS, TG><<<(unsigned)ntx * ((ny + 7) / 8) * nfields, 256, 0, s>>>(h->idx.p, h->w.p, src, g, work, nx, ny, h->n_src, nlev, ntx, (ny + 7) / 8, ldg, m); \
  } while (0)
  if (h->nnz_per_row == 3) MRATIO_FIXED(3);
  else if (h->nnz_per_row == 4) MRATIO_FIXED(4);
  else if (h->nnz_per_row == 1) MRATIO_FIXED(1);
  else {
    mpg_set_error("mpg_regrid_masked_transpose: unsupported handle (%d weights per row)", h->nnz_per_row);
    return MPG_ERR_UNSUPPORTED;
  }
#undef MRATIO_FIXED
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

template <typename TS, typename TD>
static int launch_trm(mpg_handle_s *h, const double *work, const void *src_v, bool levf, int nlev, int nfields, void *dst_v, const MaskPar &m,
                      hipStream_t s) {
  const TS *src = (const TS *)src_v;
  TD *dst = (TD *)dst_v;
  const int64_t n_src = h->n_src, P = h->n_dst;
  if (levf) {
    const int ntile = (int)((n_src + TRM_LF_CELLS - 1) / TRM_LF_CELLS);
    k_trm_short_lf<TS, TD><<<(unsigned)ntile * nfields, 256, 0, s>>>(h->tr_ptr.p, h->tr_row.p, h->tr_w.p, work, src, dst, n_src, P, nlev, ntile, m);
  } else {
    const int nblk = (int)((n_src + 255) / 256);
    k_trm_short_cf<TS, TD><<<(unsigned)nblk * nfields, 256, 0, s>>>(h->tr_ptr.p, h->tr_row.p, h->tr_w.p, work, src, dst, n_src, P, nlev, nblk, m);
  }
  if (h->tr_nlong) {
    const int ngrp = (h->tr_nlong + 3) / 4;
    auto fn = levf ? k_trm_long<TS, TD, true> : k_trm_long<TS, TD, false>;
    fn<<<(unsigned)ngrp * nfields, 256, 0, s>>>(h->tr_ptr.p, h->tr_row.p, h->tr_w.p, h->tr_long.p, h->tr_nlong, ngrp, work, src, dst, n_src, P, nlev, m);
  }
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

// arguments checked by the API entry point (mpg_api.hip); ldg: the level stride of g in elements (0 = dense)
int mpg_k_transpose_masked(mpg_handle_s *h, const void *g, int g_type, int64_t ldg, const void *src, int src_type, int layout, int nlev, int nfields,
                           void *dst, int dst_type, const mpg_mask_opts *o, double *work, hipStream_t s) {
  const int64_t P = h->n_dst, n_src = h->n_src;
  const int64_t nplanes = (int64_t)nlev * nfields;
  if (nplanes == 0) return MPG_SUCCESS;
  if (n_src == 0 || P == 0) {   // nothing maps: h and every source are +0.0
    if (P) MPG_HIP(hipMemsetAsync(work, 0, sizeof(double) * (size_t)(nplanes * P), s));
    if (n_src) return mpg_zero_planes(dst, (dst_type & MPG_TYPE_F32) ? 4 : 8, n_src, nplanes, n_src, s);
    return MPG_SUCCESS;
  }
  int rc = mpg_k_transpose_build(h, s);
  if (rc) return rc;
  if (ldg == 0) ldg = P;
  MaskPar m;
  m.mask = o->src_mask_dev;
  m.missing = o->missing_value;
  m.frac = o->min_valid_frac;
  m.fill = 0.0;     // fill_value and offset have no derivative
  m.scale = o->scale;
  m.offset = 0.0;
  m.use_nan = (o->flags & MPG_MISSING_NAN) != 0;
  m.use_val = (o->flags & MPG_MISSING_VALUE) != 0;
  const bool levf = layout == MPG_LAYOUT_LEV_FAST && nlev > 1;   // (a single level is the same memory in both layouts)
  rc = mpg_dispatch_types(src_type, g_type, [&](auto ts, auto tg) {   // (apply_mesh.h)
    return launch_mratio<decltype(ts), decltype(tg)>(h, src, levf, nlev, nfields, g, ldg, work, m, s);
  });
  if (rc) return rc;
  return mpg_dispatch_types(src_type, dst_type, [&](auto ts, auto td) {
    return launch_trm<decltype(ts), decltype(td)>(h, work, src, levf, nlev, nfields, dst, m, s);
  });
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_transpose_masked() { return (const void *)&k_trm_short_cf<double, double>; }
