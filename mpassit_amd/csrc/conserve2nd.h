// Second-order conservative regridding (mpg_handle_conserve2nd, k_conserve2nd.hip): the arithmetic of include/mpassit_amd.h's
// second-order section, one text for device and host.
//
// c2_tri_area: the signed area of a spherical triangle, E = 2 atan(x) with x = num / den the tangent of the half excess (sph_tri_area's
// num and den, geom.h), written with + - * / sqrt alone: atan(x) = 2 atan(x / (1 + sqrt(1 + x * x))) halves the angle until |x| < 2^-10,
// the series x - x^3/3 + x^5/5 - x^7/7 follows (exact to the last bit there), and the halvings are undone by powers of two.
// No atan2: a library function has the bits of its library, and the header, this text and the numpy mirror must agree bit for bit.
// c2_moment_add: one fan triangle's share of a piece's moment, a_t * ((p_0 + p_t) + p_{t+1}) / 3.  c2_poly_moment: area and moment of a
// polygon's fan from slot 0.  C2Sten: the 2 x 2 least-squares matrix of a stencil, its determinant test and b_k = M^-1 d_k written out
// with det.  c2_offset: delta_q.  c2_t: the factor of one (entry, stencil position) pair.
// Every operation is rounded on its own: include it AFTER `#pragma clang fp contract(off)` (k_conserve2nd.hip), or build with
// -ffp-contract=off (tests/c/conserve2nd_test.cpp).  Only + - * / sqrt.  Plain C++ without HIP intrinsics, as patch.h.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define C2_FN __host__ __device__ __forceinline__
#else
#define C2_FN inline
#endif

#define C2_DET_TOL 0x1p-26   // a stencil passes when det > 2^-26 * (M00 * M11): a definition, not a tuning constant
#define C2_HALF_TOL 0x1p-10  // the half-angle steps end below this |x|
#define C2_MAX_HALVINGS 64   // |x| falls below 2^-10 within 2 + log2 steps of any finite x; a NaN leaves through this bound

C2_FN double c2_dot(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// signed area of the spherical triangle a, b, c (unit vectors), counter-clockwise positive.  den <= 0 (an excess of pi or more: no cell
// polygon's fan triangle) gives 0.0
C2_FN double c2_tri_area(const double *a, const double *b, const double *c) {
  const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, v[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const double w[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
  const double num = c2_dot(a, w);
  const double den = ((1.0 + c2_dot(a, b)) + c2_dot(b, c)) + c2_dot(c, a);
  if (!(den > 0.0)) return 0.0;
  double x = num / den, scale = 2.0;
  for (int k = 0; k < C2_MAX_HALVINGS && !(fabs(x) < C2_HALF_TOL); ++k) {
    x = x / (1.0 + sqrt(1.0 + x * x));
    scale = scale * 2.0;
  }
  const double x2 = x * x;
  return scale * (x * (1.0 - x2 * (1.0 / 3.0 - x2 * (1.0 / 5.0 - x2 * (1.0 / 7.0)))));
}

// m += a * ((p0 + p1) + p2) / 3, per component
C2_FN void c2_moment_add(double a, const double *p0, const double *p1, const double *p2, double *m) {
  for (int k = 0; k < 3; ++k) {
    const double c = ((p0[k] + p1[k]) + p2[k]) / 3.0;
    m[k] = m[k] + a * c;
  }
}

// the fan from slot 0 of the polygon p [n][3]: the signed area (0.0 for n < 3) and the moment m [3], both from 0.0 in slot order
C2_FN double c2_poly_moment(const double (*p)[3], int n, double *m) {
  double area = 0.0;
  m[0] = m[1] = m[2] = 0.0;
  for (int t = 1; t + 1 < n; ++t) {
    const double a = c2_tri_area(p[0], p[t], p[t + 1]);
    area = area + a;
    c2_moment_add(a, p[0], p[t], p[t + 1], m);
  }
  return area;
}

// the unit vector of the moment m; false (g untouched) when its length is not > 0
C2_FN bool c2_unit(const double *m, double *g) {
  const double r = sqrt(c2_dot(m, m));
  if (!(r > 0.0)) return false;
  g[0] = m[0] / r;
  g[1] = m[1] / r;
  g[2] = m[2] / r;
  return true;
}

struct C2Sten {
  double m00, m01, m11, det;
  int n;
};
C2_FN void c2_sten_init(C2Sten &s) {
  s.m00 = s.m01 = s.m11 = s.det = 0.0;
  s.n = 0;
}
// d_k = ((G_k - G_i) . e1, (G_k - G_i) . e2)
C2_FN void c2_sten_d(const double *Gi, const double *Gk, const double *e1, const double *e2, double &dx, double &dy) {
  const double d[3] = {Gk[0] - Gi[0], Gk[1] - Gi[1], Gk[2] - Gi[2]};
  dx = c2_dot(d, e1);
  dy = c2_dot(d, e2);
}
C2_FN void c2_sten_add(C2Sten &s, double dx, double dy) {
  s.m00 = s.m00 + dx * dx;
  s.m01 = s.m01 + dx * dy;
  s.m11 = s.m11 + dy * dy;
  ++s.n;
}
// after the last c2_sten_add: det, and whether the stencil passes (at least two neighbours, det > 2^-26 * (M00 * M11))
C2_FN bool c2_sten_pass(C2Sten &s) {
  const double p = s.m00 * s.m11;
  s.det = p - s.m01 * s.m01;
  return s.n >= 2 && s.det > C2_DET_TOL * p;
}
// b_k = M^-1 d_k of a passing stencil
C2_FN void c2_sten_b(const C2Sten &s, double dx, double dy, double &bx, double &by) {
  bx = (s.m11 * dx - s.m01 * dy) / s.det;
  by = (s.m00 * dy - s.m01 * dx) / s.det;
}

// the whole solve on n neighbour offsets d [n][2] in ascending neighbour order: b [n][2] and bi [2] = -sum b_k -> passes.  A stencil that
// fails writes nothing to b and bi = 0
C2_FN bool c2_stencil(const double (*d)[2], int n, double (*b)[2], double *bi) {
  C2Sten s;
  c2_sten_init(s);
  for (int k = 0; k < n; ++k) c2_sten_add(s, d[k][0], d[k][1]);
  bi[0] = bi[1] = 0.0;
  if (!c2_sten_pass(s)) return false;
  double sx = 0.0, sy = 0.0;
  for (int k = 0; k < n; ++k) {
    c2_sten_b(s, d[k][0], d[k][1], b[k][0], b[k][1]);
    sx = sx + b[k][0];
    sy = sy + b[k][1];
  }
  bi[0] = -sx;
  bi[1] = -sy;
  return true;
}

// delta_q = ((m_q / A_q - M_i / A_i) . e1, ( ... ) . e2); 0 when A_q <= 0 or A_i <= 0
C2_FN void c2_offset(const double *mq, double Aq, const double *Mi, double Ai, const double *e1, const double *e2, double &dx, double &dy) {
  dx = dy = 0.0;
  if (!(Aq > 0.0) || !(Ai > 0.0)) return;
  const double d[3] = {mq[0] / Aq - Mi[0] / Ai, mq[1] / Aq - Mi[1] / Ai, mq[2] / Aq - Mi[2] / Ai};
  dx = c2_dot(d, e1);
  dy = c2_dot(d, e2);
}

// the factor of stencil position (bx, by) for an entry with offset (dx, dy); own: the position is the entry's source cell itself
C2_FN double c2_t(double dx, double dy, double bx, double by, bool own) {
  const double g = (dx * bx) + (dy * by);
  return own ? 1.0 + g : g;
}
