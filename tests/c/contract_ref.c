/* An exact host restatement of the arithmetic include/mpassit_amd.h promises for the Regrid and wind calls ("contract by identity,
 * no tolerance"), written from the header's text: explicit fma() where the header says fma, separate * + - / everywhere else, nothing
 * else from libm.  Build with  gcc -O2 -fPIC -shared -ffp-contract=off  (tests/_contract_ref.py does): with contraction off the
 * compiler fuses nothing on its own, so every rounding below is the one written.
 *
 * Index conventions (those of the handle's getters): a fixed handle is idx / w [n_dst][nnz] with idx < 0 = unmapped; a CSR handle is
 * rowptr [n_dst + 1], col / val [nnz] in stored order.  A source is nfields slabs of nlev * n_src elements, [lev][src] or, with
 * src_lev_fast, [src][lev]; a result is nfields slabs of nlev * n_dst, [lev][point] or, with dst_lev_fast, [point][lev].
 *
 * `variant` selects a deliberately WRONG recipe (0 = the contract); the tests use them to show that their inputs can tell the
 * contract from its neighbours. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

enum {
  CR_REVERSED = 1,    /* slots (row entries) accumulated last to first */
  CR_MULADD = 2,      /* every fma of the accumulation as a rounded product and a rounded sum */
  CR_EPI_MULADD = 4,  /* the epilogue as acc * scale + offset */
  CR_EPI_SKIP = 8,    /* no epilogue at scale 1, offset 0 */
  CR_COLSORT = 16     /* a CSR row accumulated in ascending column order instead of stored order */
};

double cr_fma(double a, double b, double c) { return fma(a, b, c); }

void cr_fma_vec(const double *a, const double *b, const double *c, double *out, int64_t n) {
  for (int64_t i = 0; i < n; ++i) out[i] = fma(a[i], b[i], c[i]);
}

static double load(const void *src, int f32, int64_t i) { return f32 ? (double)((const float *)src)[i] : ((const double *)src)[i]; }

static void store(void *dst, int f32, int64_t i, double v) {
  if (f32) ((float *)dst)[i] = (float)v;
  else ((double *)dst)[i] = v;
}

static int64_t src_at(int src_lev_fast, int64_t n_src, int nlev, int64_t c, int k) { return src_lev_fast ? c * nlev + k : (int64_t)k * n_src + c; }

static int64_t dst_at(int dst_lev_fast, int64_t n_dst, int nlev, int64_t p, int k) { return dst_lev_fast ? p * nlev + k : (int64_t)k * n_dst + p; }

static double accum(double w, double x, double acc, int variant) { return (variant & CR_MULADD) ? w * x + acc : fma(w, x, acc); }

/* the header's wsum3: fma(w2, e, fma(w1, b, w0 * a)) */
static double wsum3(const double *w, const double *x, int variant) {
  if (variant & CR_REVERSED) return accum(w[0], x[0], accum(w[1], x[1], w[2] * x[2], variant), variant);
  return accum(w[2], x[2], accum(w[1], x[1], w[0] * x[0], variant), variant);
}

/* acc = fma(w[q], x[q], acc) from 0.0 in the order given */
static double chain(const double *w, const double *x, int n, int variant) {
  double acc = 0.0;
  if (variant & CR_REVERSED)
    for (int q = n - 1; q >= 0; --q) acc = accum(w[q], x[q], acc, variant);
  else
    for (int q = 0; q < n; ++q) acc = accum(w[q], x[q], acc, variant);
  return acc;
}

/* (dst type) fma(acc, scale, offset): the cast is store()'s */
static double epilogue(double acc, int on, double scale, double offset, int variant) {
  if (!on) return acc;
  if ((variant & CR_EPI_SKIP) && scale == 1.0 && offset == 0.0) return acc;
  if (variant & CR_EPI_MULADD) return acc * scale + offset;
  return fma(acc, scale, offset);
}

/* nnz 1: a copy; 3: wsum3; 4: the chain; unmapped (slot 0 < 0): +0.0 before the epilogue */
int cr_apply_fixed(const int32_t *idx, const double *w, int nnz, int64_t n_src, int64_t n_dst, const void *src, int src_f32, int src_lev_fast,
                   int nlev, int nfields, void *dst, int dst_f32, int dst_lev_fast, int epi, double scale, const double *offsets, int variant) {
  if (nnz != 1 && nnz != 3 && nnz != 4) return 1;
  for (int f = 0; f < nfields; ++f) {
    const int64_t sb = (int64_t)f * nlev * n_src, db = (int64_t)f * nlev * n_dst;
    const double offset = offsets ? offsets[f] : 0.0;
    for (int64_t p = 0; p < n_dst; ++p) {
      const int32_t *ci = idx + p * nnz;
      const double *wp = w + p * nnz;
      const int mapped = ci[0] >= 0;
      for (int k = 0; k < nlev; ++k) {
        double acc = 0.0;
        if (mapped) {
          double x[4];
          for (int q = 0; q < nnz; ++q) {
            if (ci[q] < 0 || ci[q] >= n_src) return 2;
            x[q] = load(src, src_f32, sb + src_at(src_lev_fast, n_src, nlev, ci[q], k));
          }
          acc = nnz == 1 ? x[0] : nnz == 3 ? wsum3(wp, x, variant) : chain(wp, x, 4, variant);
        }
        store(dst, dst_f32, db + dst_at(dst_lev_fast, n_dst, nlev, p, k), epilogue(acc, epi, scale, offset, variant));
      }
    }
  }
  return 0;
}

static const int32_t *sort_col;
static int by_col(const void *a, const void *b) {
  const int64_t i = *(const int64_t *)a, j = *(const int64_t *)b;
  if (sort_col[i] != sort_col[j]) return sort_col[i] < sort_col[j] ? -1 : 1;
  return i < j ? -1 : i > j;
}

/* the chain over a row in stored order; an empty row gives +0.0 */
int cr_apply_csr(const int64_t *rowptr, const int32_t *col, const double *val, int64_t n_src, int64_t n_dst, const void *src, int src_f32,
                 int src_lev_fast, int nlev, int nfields, void *dst, int dst_f32, int dst_lev_fast, int epi, double scale, const double *offsets,
                 int variant) {
  int64_t longest = 0;
  for (int64_t p = 0; p < n_dst; ++p)
    if (rowptr[p + 1] - rowptr[p] > longest) longest = rowptr[p + 1] - rowptr[p];
  int64_t *order = (int64_t *)malloc(sizeof(int64_t) * (size_t)(longest + 1));
  double *x = (double *)malloc(sizeof(double) * (size_t)(longest + 1)), *ww = (double *)malloc(sizeof(double) * (size_t)(longest + 1));
  int rc = 0;
  for (int64_t p = 0; p < n_dst && !rc; ++p) {
    const int64_t b = rowptr[p], n = rowptr[p + 1] - b;
    for (int64_t q = 0; q < n; ++q) order[q] = b + q;
    if (variant & CR_COLSORT) {
      sort_col = col;
      qsort(order, (size_t)n, sizeof(int64_t), by_col);
    }
    for (int64_t q = 0; q < n; ++q) {
      if (col[order[q]] < 0 || col[order[q]] >= n_src) rc = 2;
      ww[q] = val[order[q]];
    }
    if (rc) break;
    for (int f = 0; f < nfields; ++f) {
      const int64_t sb = (int64_t)f * nlev * n_src, db = (int64_t)f * nlev * n_dst;
      const double offset = offsets ? offsets[f] : 0.0;
      for (int k = 0; k < nlev; ++k) {
        for (int64_t q = 0; q < n; ++q) x[q] = load(src, src_f32, sb + src_at(src_lev_fast, n_src, nlev, col[order[q]], k));
        store(dst, dst_f32, db + dst_at(dst_lev_fast, n_dst, nlev, p, k), epilogue(chain(ww, x, (int)n, variant), epi, scale, offset, variant));
      }
    }
  }
  free(order);
  free(x);
  free(ww);
  return rc;
}

/* The masked recipe, header lines "valid(q) ... result".  nnz > 0: a fixed handle (idx / w), nnz == 0: a CSR handle (rowptr / col / val).
 * flags: 1 = a NaN is missing, 2 = an element equal to missing_value is missing. */
int cr_apply_masked(int nnz, const int32_t *idx, const double *w, const int64_t *rowptr, const int32_t *col, const double *val, int64_t n_src,
                    int64_t n_dst, const void *src, int src_f32, int src_lev_fast, int nlev, int nfields, void *dst, int dst_f32, int flags,
                    double missing_value, const uint8_t *src_mask, double min_valid_frac, double fill_value, double scale, double offset) {
  if (nnz != 0 && nnz != 1 && nnz != 3 && nnz != 4) return 1;
  int64_t longest = nnz;
  if (nnz == 0)
    for (int64_t p = 0; p < n_dst; ++p)
      if (rowptr[p + 1] - rowptr[p] > longest) longest = rowptr[p + 1] - rowptr[p];
  double *wk = (double *)malloc(sizeof(double) * (size_t)(longest + 1)), *xk = (double *)malloc(sizeof(double) * (size_t)(longest + 1));
  int rc = 0;
  for (int f = 0; f < nfields && !rc; ++f) {
    const int64_t sb = (int64_t)f * nlev * n_src, db = (int64_t)f * nlev * n_dst;
    for (int64_t p = 0; p < n_dst && !rc; ++p) {
      const int64_t b = nnz ? p * nnz : rowptr[p], n = nnz ? nnz : rowptr[p + 1] - rowptr[p];
      const int32_t *ci = nnz ? idx + b : col + b;
      const double *wp = nnz ? w + b : val + b;
      for (int k = 0; k < nlev; ++k) {
        double Wt = 0.0, Wv = 0.0;
        for (int64_t q = 0; q < n; ++q) {
          const double wq = nnz == 1 ? 1.0 : wp[q];
          int ok = ci[q] >= 0;
          double x = 0.0;
          if (ok) {
            if (ci[q] >= n_src) { rc = 2; break; }
            if (src_mask && src_mask[ci[q]]) ok = 0;
            x = load(src, src_f32, sb + src_at(src_lev_fast, n_src, nlev, ci[q], k));
            if ((flags & 1) && x != x) ok = 0;
            if ((flags & 2) && x == missing_value) ok = 0;
          }
          wk[q] = ok ? wq : 0.0;
          xk[q] = ok ? x : 0.0;
          Wt = q == 0 ? wq : Wt + wq;
          Wv = q == 0 ? wk[q] : Wv + wk[q];
        }
        if (rc) break;
        const double N = n == 0 ? 0.0 : nnz == 1 ? xk[0] : nnz == 3 ? wsum3(wk, xk, 0) : chain(wk, xk, (int)n, 0);
        const int defined = n > 0 && Wv > 0.0 && Wv >= min_valid_frac * Wt;
        const double ratio = Wt / Wv;
        const double scaled = N * ratio;
        store(dst, dst_f32, db + dst_at(0, n_dst, nlev, p, k), defined ? fma(scaled, scale, offset) : fill_value);
      }
    }
  }
  free(wk);
  free(xk);
  return rc;
}

/* The wind formulas, every product and sum rounded.  a, b: float64, the Regrids with epilogue (1, 0), in the layout of the results.
 * mode 0 (mesh): o0 = a * c - b * s, o1 = a * s + b * c, or o0 = a, o1 = b without angles.  mode 1 (edges): o0 = a * c + b * s,
 * o1 = b * c - a * s (o1 may be NULL).  unmapped[p] != 0: +0.0 in every result.  One cast to the destination type. */
int cr_wind_pair(int mode, const double *a, const double *b, const double *c, const double *s, const uint8_t *unmapped, int64_t n_dst, int nlev,
                 int dst_lev_fast, void *o0, void *o1, int dst_f32) {
  if (mode == 1 && (!c || !s)) return 1;
  for (int64_t p = 0; p < n_dst; ++p)
    for (int k = 0; k < nlev; ++k) {
      const int64_t i = dst_at(dst_lev_fast, n_dst, nlev, p, k);
      double r0, r1;
      if (unmapped[p]) r0 = r1 = 0.0;
      else if (mode == 0 && !c) {
        r0 = a[i];
        r1 = b[i];
      } else {
        const double ac = a[i] * c[p], bs = b[i] * s[p], as = a[i] * s[p], bc = b[i] * c[p];
        if (mode == 0) {
          r0 = ac - bs;
          r1 = as + bc;
        } else {
          r0 = ac + bs;
          r1 = bc - as;
        }
      }
      store(o0, dst_f32, i, r0);
      if (o1) store(o1, dst_f32, i, r1);
    }
  return 0;
}

/* mpg_regrid_transpose_dev, per (source c, level k): acc = fma(w_j, (double)g[k][row_j], acc) from +0.0 over the stored entries that
 * reference c, ascending by (destination point, slot) -- for a CSR handle by position, duplicates included --, then (dst type)acc, one
 * rounding; a source nothing references gets +0.0.  nnz > 0: a fixed handle (idx / w [n_dst][nnz], idx < 0 skipped; w NULL: weight 1,
 * a nearest handle); nnz == 0: a CSR handle.  g: nfields * nlev planes of n_dst, g_level_stride elements apart (0 = dense).
 * The pole term is NOT restated: cap_row [n_src] (may be NULL) comes back 1 on the sources of the CENTER rows that a cap with a non-zero
 * weight adds its term to, 0 elsewhere; those sources hold the segment sum alone here.
 * variant: CR_MULADD, and CR_REVERSED (the segment last entry first). */
int cr_apply_transpose(int nnz, const int32_t *idx, const double *w, const int64_t *rowptr, const int32_t *col, const double *val, int64_t n_src,
                       int64_t n_dst, const void *g, int g_f32, int64_t g_level_stride, int nlev, int nfields, void *dst, int dst_f32,
                       int dst_lev_fast, const int32_t *pole_src0, const double *pole_w, int64_t n_pole, int row_len, uint8_t *cap_row, int variant) {
  if (nnz != 0 && nnz != 1 && nnz != 3 && nnz != 4) return 1;
  const int64_t ld = g_level_stride ? g_level_stride : n_dst;
  if (ld < n_dst) return 3;
  const int64_t ne = nnz ? n_dst * nnz : rowptr[n_dst];
  int64_t *ptr = (int64_t *)calloc((size_t)n_src + 2, sizeof(int64_t));
  int64_t *rows = (int64_t *)malloc(sizeof(int64_t) * (size_t)(ne + 1));
  double *wts = (double *)malloc(sizeof(double) * (size_t)(ne + 1));
  int rc = 0;
  /* entries in (point, slot) order, dealt to their sources: each source's list is ascending by construction */
  for (int pass = 0; pass < 2 && !rc; ++pass) {
    for (int64_t p = 0; p < n_dst && !rc; ++p) {
      const int64_t b = nnz ? p * nnz : rowptr[p], e = nnz ? b + nnz : rowptr[p + 1];
      for (int64_t j = b; j < e; ++j) {
        const int32_t c = nnz ? idx[j] : col[j];
        if (c < 0 && nnz) continue;
        if (c < 0 || c >= n_src) { rc = 2; break; }
        if (pass == 0) ptr[c + 2]++;
        else {
          const int64_t at = ptr[c + 1]++;
          rows[at] = p;
          wts[at] = nnz ? (w ? w[j] : 1.0) : val[j];
        }
      }
    }
    if (pass == 0)
      for (int64_t c = 0; c < n_src; ++c) ptr[c + 2] += ptr[c + 1];   /* ptr[c + 1] = start of c; after the fill, ptr[c + 1] = its end */
  }
  /* now the segment of c is [ptr[c], ptr[c + 1]) */
  for (int f = 0; f < nfields && !rc; ++f)
    for (int k = 0; k < nlev; ++k) {
      const int64_t gb = ((int64_t)f * nlev + k) * ld, db = (int64_t)f * nlev * n_src;
      for (int64_t c = 0; c < n_src; ++c) {
        double acc = 0.0;
        if (variant & CR_REVERSED)
          for (int64_t j = ptr[c + 1] - 1; j >= ptr[c]; --j) acc = accum(wts[j], load(g, g_f32, gb + rows[j]), acc, variant);
        else
          for (int64_t j = ptr[c]; j < ptr[c + 1]; ++j) acc = accum(wts[j], load(g, g_f32, gb + rows[j]), acc, variant);
        store(dst, dst_f32, db + dst_at(dst_lev_fast, n_src, nlev, c, k), acc);
      }
    }
  if (cap_row) {
    for (int64_t c = 0; c < n_src; ++c) cap_row[c] = 0;
    for (int64_t q = 0; q < n_pole; ++q) {
      if (pole_w[q] == 0.0) continue;
      if (pole_src0[q] < 0 || pole_src0[q] + (int64_t)row_len > n_src) { rc = 2; break; }
      for (int i = 0; i < row_len; ++i) cap_row[pole_src0[q] + i] = 1;
    }
  }
  free(ptr);
  free(rows);
  free(wts);
  return rc;
}

/* mpg_rotate_winds[_dev], in place on u, v [nlev][npts]: the seven operations of the header, each rounded and nothing contracted */
void cr_rotate(int64_t npts, int nlev, const double *cosa, const double *sina, double *u, double *v) {
  for (int64_t p = 0; p < npts; ++p) {
    const double ca = cosa[p], sa = sina[p];
    const double tana = sa / ca;
    const double sat = sa * tana;
    const double den = ca + sat;
    for (int k = 0; k < nlev; ++k) {
      const int64_t q = (int64_t)k * npts + p;
      const double uo = u[q], vo = v[q];
      const double t1 = vo * tana;
      const double s1 = uo + t1;
      const double un = s1 / den;
      const double t2 = un * sa;
      const double d2 = vo - t2;
      u[q] = un;
      v[q] = d2 / ca;
    }
  }
}

static void swap_bytes(void *p, int n) {
  unsigned char *b = (unsigned char *)p;
  for (int i = 0; i < n / 2; ++i) {
    const unsigned char t = b[i];
    b[i] = b[n - 1 - i];
    b[n - 1 - i] = t;
  }
}

/* mpg_wind_destagger[_pitched]_dev / mpg_wind_destagger: cr_rotate on copies of the mass winds [nlev][n_mass] (cosa NULL: none), then
 * the 4-slot chain of cr_apply_fixed on the EDGE1 handle (idx1 / w1 [n1][4], U from the rotated umass) and the EDGE2 handle (idx2 / w2
 * [n2][4], V from the rotated vmass); a NULL idx: that component is not produced.  dst_type 0 (float64): the sum as it stands; 1 (float32),
 * 2 (float64 big-endian), 3 (float32 big-endian): (TD)fma(sum, 1.0, 0.0), a big-endian result being the byte-reversed bits.  u / v:
 * nlev planes, dst_level_stride elements apart (0 = dense); elements between the planes are not written.  urot / vrot (may be NULL):
 * the rotated mass winds. */
int cr_wind_destagger(const int32_t *idx1, const double *w1, int64_t n1, const int32_t *idx2, const double *w2, int64_t n2, int64_t n_mass,
                      const double *cosa, const double *sina, const double *umass, const double *vmass, int nlev, void *u, void *v, int dst_type,
                      int64_t dst_level_stride, double *urot, double *vrot) {
  const size_t nl = (size_t)n_mass * (size_t)nlev;
  double *um = NULL, *vm = NULL;
  if (cosa) {
    if (!sina || !umass || !vmass) return 1;
    um = (double *)malloc(sizeof(double) * (nl + 1));
    vm = (double *)malloc(sizeof(double) * (nl + 1));
    for (size_t i = 0; i < nl; ++i) {
      um[i] = umass[i];
      vm[i] = vmass[i];
    }
    cr_rotate(n_mass, nlev, cosa, sina, um, vm);
    if (urot) for (size_t i = 0; i < nl; ++i) urot[i] = um[i];
    if (vrot) for (size_t i = 0; i < nl; ++i) vrot[i] = vm[i];
  }
  const int f32 = dst_type & 1, be = dst_type & 2, typed = dst_type != 0;
  int rc = 0;
  for (int comp = 0; comp < 2 && !rc; ++comp) {
    const int32_t *idx = comp ? idx2 : idx1;
    const double *w = comp ? w2 : w1;
    const int64_t n = comp ? n2 : n1;
    const double *src = comp ? (vm ? vm : vmass) : (um ? um : umass);
    void *out = comp ? v : u;
    if (!idx) continue;
    if (!src || !out) { rc = 1; break; }
    const int64_t ld = dst_level_stride ? dst_level_stride : n;
    if (ld < n) { rc = 3; break; }
    double *plane = (double *)malloc(sizeof(double) * (size_t)(n + 1));
    const double zero = 0.0;
    for (int k = 0; k < nlev && !rc; ++k) {
      rc = cr_apply_fixed(idx, w, 4, n_mass, n, src + (size_t)k * (size_t)n_mass, 0, 0, 1, 1, plane, 0, 0, typed, 1.0, &zero, 0);
      for (int64_t p = 0; p < n && !rc; ++p) {
        const int64_t at = (int64_t)k * ld + p;
        if (f32) {
          ((float *)out)[at] = (float)plane[p];
          if (be) swap_bytes((float *)out + at, 4);
        } else {
          ((double *)out)[at] = plane[p];
          if (be) swap_bytes((double *)out + at, 8);
        }
      }
    }
    free(plane);
  }
  free(um);
  free(vm);
  return rc;
}
