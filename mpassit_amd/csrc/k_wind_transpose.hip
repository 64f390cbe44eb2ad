// The adjoint of the wind chain (k_wind.hip; interp.F90:291-328) as ONE pass: the gradients of U (EDGE1) and V (EDGE2) back to the
// gradients of the mass-point winds --
//   s1 = A1^T gU,  s2 = A2^T gV          the two Regrids' transposes (k_transpose.hip: the same segment sum, transpose_seg.h)
//   gun = s1 (+ gUMASS'),  gvn = s2 (+ gVMASS')   the gradients of the forward's optional rotated mass winds
//   (guo, gvo) = R^T (gun, gvn)          the reverse mode of interp.F90:737-748 (k_rotate_t of k_apply.hip: the same expressions)
// The three-call chain writes s1 and s2, reads and rewrites both in the rotation: 8 float64 planes per level beside the gathers'
// 2 source planes; here the sums stay in registers: 2 planes gathered, 2 stored (4 with the optional gradients' 2 read).
//
// One lane per mass point, consecutive lanes consecutive i: both stores are whole coalesced rows, and neighbouring lanes gather
// neighbouring U / V points (a U point is referenced by the up to four CENTER points of its quad: the lines are shared through L1 / L2).
// Both handles' segments (row, weight) are loaded once into registers and reused for every level, the rotation constants once per
// lane.  Grid -> Grid handles have about four entries per CENTER point: where no lane of a wave has more, the 4-slot form runs, all
// eight gathers of a level ahead of the fmas.  A lane whose segment exceeds the register form (WT_SLOTS) sums it from memory (any length).
// No atomics; every value is one expression, the same for every launch shape: the bits of the chain.
#pragma clang fp contract(off)
#include "transpose_seg.h"

struct WindTrArgs {
  const int32_t *ptr1, *row1, *ptr2, *row2;   // transposed index of the EDGE1 / EDGE2 handle (NULL: that component is not produced)
  const double *w1, *w2;
  const double *cosa, *sina;                  // [ny][nx] (ROT only)
  const void *gu, *gv;                        // [nlev] planes of TS, ldu / ldv elements apart
  int64_t ldu, ldv;
  const double *gur, *gvr;                    // optional [nlev][ny][nx] (ROT only)
  double *gum, *gvm;                          // [nlev][ny][nx]
  int64_t NP;
  int nlev;
};

// the reverse mode of interp.F90:737-748 (k_rotate_t evaluates the same expressions in the same order)
__device__ __forceinline__ void wt_rotate_t(double gun, double gvn, double ca, double sa, double tana, double den, double &guo, double &gvo) {
  const double a = gvn / ca;
  const double t = a * sa;
  const double b = gun - t;
  guo = b / den;
  const double p = guo * tana;
  gvo = a + p;
}

// The register form here holds WT_SLOTS entries per handle, not k_transpose.hip's TR_SHORT: two segments are live at once, and with 16
// slots each the kernel needs 183 VGPRs (two waves per SIMD: too few to hide the gathers); Grid -> Grid segments rarely pass 6
#define WT_SLOTS 8

struct WtSeg {
  int32_t r[WT_SLOTS];
  double w[WT_SLOTS];
  int n = 0, nmax = 0;
  int32_t b = 0, e = 0;   // the segment in memory, for a lane whose segment is longer than WT_SLOTS (b == e otherwise)
};

template <typename TS>
__device__ __forceinline__ void wt_load(WtSeg &s, const int32_t *__restrict__ ptr, const int32_t *__restrict__ rows, const double *__restrict__ wts,
                                        int64_t c, bool act) {
  s.n = tr_load_seg<TS>(ptr, rows, wts, c, act, s.r, s.w);
  s.nmax = tr_wave_max(s.n);
  if (act) {
    const int32_t b = ptr[c], e = ptr[c + 1];
    if (e - b > WT_SLOTS) {
      s.b = b;
      s.e = e;
    }
  }
}

// U: rh_edge1 given, V: rh_edge2 given (ROT: both)
template <typename TS, bool ROT, bool U, bool V>
__global__ __launch_bounds__(256) void k_wind_destagger_t(const WindTrArgs a) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool act = c < a.NP;
  WtSeg s1, s2;
  if constexpr (U) wt_load<TS>(s1, a.ptr1, a.row1, a.w1, c, act);
  if constexpr (V) wt_load<TS>(s2, a.ptr2, a.row2, a.w2, c, act);
  const bool any_long = __any((s1.e > s1.b) || (s2.e > s2.b));
  const bool four = s1.nmax <= 4 && s2.nmax <= 4;   // wave-uniform
  if (!act) return;
  double ca = 1.0, sa = 0.0, tana = 0.0, den = 1.0;
  if constexpr (ROT) {
    ca = a.cosa[c];
    sa = a.sina[c];
    tana = sa / ca;
    den = ca + sa * tana;
  }
  const TS *pu = (const TS *)a.gu, *pv = (const TS *)a.gv;   // this level's planes: 64-bit pointer steps
  const double *pur = a.gur ? a.gur + c : nullptr, *pvr = a.gvr ? a.gvr + c : nullptr;
  double *ou = U ? a.gum + c : nullptr, *ov = V ? a.gvm + c : nullptr;
#pragma unroll 2
  for (int k = 0; k < a.nlev; ++k) {
    double gun = 0.0, gvn = 0.0, ru = 0.0, rv = 0.0;
    if constexpr (ROT) {   // issued with the gathers
      if (pur) ru = __builtin_nontemporal_load(pur);
      if (pvr) rv = __builtin_nontemporal_load(pvr);
    }
    if (four) {
      double vu[4], vv[4];
      if constexpr (U) tr_seg_gather4<TS, WT_SLOTS>(s1.r, pu, vu);
      if constexpr (V) tr_seg_gather4<TS, WT_SLOTS>(s2.r, pv, vv);
      if constexpr (U) gun = tr_seg_sum4(s1.w, vu, s1.n);
      if constexpr (V) gvn = tr_seg_sum4(s2.w, vv, s2.n);
    } else {
      if constexpr (U) gun = tr_seg_regs<TS>(s1.r, s1.w, s1.n, s1.nmax, pu);
      if constexpr (V) gvn = tr_seg_regs<TS>(s2.r, s2.w, s2.n, s2.nmax, pv);
    }
    if (any_long) {
      if constexpr (U)
        if (s1.e > s1.b) gun = tr_seg_mem<TS>(a.row1, a.w1, s1.b, s1.e, pu);
      if constexpr (V)
        if (s2.e > s2.b) gvn = tr_seg_mem<TS>(a.row2, a.w2, s2.b, s2.e, pv);
    }
    if constexpr (ROT) {
      if (pur) gun = gun + ru;
      if (pvr) gvn = gvn + rv;
      double guo, gvo;
      wt_rotate_t(gun, gvn, ca, sa, tana, den, guo, gvo);
      gun = guo;
      gvn = gvo;
    }
    if constexpr (U) __builtin_nontemporal_store(gun, ou);
    if constexpr (V) __builtin_nontemporal_store(gvn, ov);
    pu += a.ldu;
    pv += a.ldv;
    if (pur) pur += a.NP;
    if (pvr) pvr += a.NP;
    if constexpr (U) ou += a.NP;
    if constexpr (V) ov += a.NP;
  }
}

template <typename TS>
static int launch_wt(const WindTrArgs &a, bool rot, bool u, bool v, hipStream_t s) {
  const unsigned nwg = (unsigned)((a.NP + 255) / 256);
  if (rot) k_wind_destagger_t<TS, true, true, true><<<nwg, 256, 0, s>>>(a);
  else if (u && v) k_wind_destagger_t<TS, false, true, true><<<nwg, 256, 0, s>>>(a);
  else if (u) k_wind_destagger_t<TS, false, true, false><<<nwg, 256, 0, s>>>(a);
  else k_wind_destagger_t<TS, false, false, true><<<nwg, 256, 0, s>>>(a);
  MPG_HIP(hipGetLastError());
  return MPG_SUCCESS;
}

// h1 / h2: the CENTER -> EDGE1 / EDGE2 pair of one grid (mpg_wind_pair_dims; either may be NULL without a rotation); the arguments are
// checked by the API entry point.  The first call on a handle builds its transposed index (allocates, synchronises).
int mpg_k_wind_destagger_transpose(mpg_handle_s *h1, mpg_handle_s *h2, const double *cosa, const double *sina, const void *gu, const void *gv,
                                   int src_type, int64_t ldu, int64_t ldv, int nlev, const double *gur, const double *gvr, double *gum, double *gvm,
                                   hipStream_t s) {
  int nx, ny, rc;
  if ((rc = mpg_wind_pair_dims(h1, h2, &nx, &ny))) return rc;
  const bool rot = cosa != nullptr;
  if (rot && ((h1 && h1->n_pole) || (h2 && h2->n_pole))) return MPG_ERR_UNSUPPORTED;   // as the forward
  if (nlev == 0) return MPG_SUCCESS;
  for (mpg_handle_s *h : {h1, h2})
    if (h && (rc = mpg_k_transpose_build(h, s))) return rc;
  WindTrArgs a;
  a.ptr1 = h1 ? h1->tr_ptr.p : nullptr;
  a.row1 = h1 ? h1->tr_row.p : nullptr;
  a.w1 = h1 ? h1->tr_w.p : nullptr;
  a.ptr2 = h2 ? h2->tr_ptr.p : nullptr;
  a.row2 = h2 ? h2->tr_row.p : nullptr;
  a.w2 = h2 ? h2->tr_w.p : nullptr;
  a.cosa = cosa;
  a.sina = sina;
  a.gu = gu;
  a.gv = gv;
  a.ldu = ldu;
  a.ldv = ldv;
  a.gur = rot ? gur : nullptr;
  a.gvr = rot ? gvr : nullptr;
  a.gum = gum;
  a.gvm = gvm;
  a.NP = (int64_t)nx * ny;
  a.nlev = nlev;
  if (src_type & MPG_TYPE_F32) rc = launch_wt<float>(a, rot, h1 != nullptr, h2 != nullptr, s);
  else rc = launch_wt<double>(a, rot, h1 != nullptr, h2 != nullptr, s);
  if (rc) return rc;
  // pole caps of a periodic grid (no rotation there): the two CENTER rows rewritten with the pole term last, exactly as
  // mpg_regrid_transpose_dev ends
  if (h1 && (rc = mpg_k_transpose_pole(h1, gu, src_type, ldu, nlev, gum, s))) return rc;
  if (h2 && (rc = mpg_k_transpose_pole(h2, gv, src_type, ldv, nlev, gvm, s))) return rc;
  return MPG_SUCCESS;
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_wind_transpose() { return (const void *)&k_wind_destagger_t<double, true, true, true>; }
