// The second-order conservative arithmetic (mpassit_amd/csrc/conserve2nd.h) on the host, on exact inputs.  A stand-alone program:
//   g++ -std=c++17 -ffp-contract=off tests/c/conserve2nd_test.cpp -o conserve2nd_test && ./conserve2nd_test
#include <cmath>
#include <cstdio>

#include "../../mpassit_amd/csrc/conserve2nd.h"

static int g_fail = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      ++g_fail;                     \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);     \
      std::printf("\n");            \
    }                               \
  } while (0)

static void unit(double x, double y, double z, double *p) {
  const double r = std::sqrt(x * x + y * y + z * z);
  p[0] = x / r; p[1] = y / r; p[2] = z / r;
}

// 2 atan2(num, den) in long double: what c2_tri_area stands for
static double ref_area(const double *a, const double *b, const double *c) {
  const long double u[3] = {(long double)b[0] - a[0], (long double)b[1] - a[1], (long double)b[2] - a[2]};
  const long double v[3] = {(long double)c[0] - a[0], (long double)c[1] - a[1], (long double)c[2] - a[2]};
  const long double num = a[0] * (u[1] * v[2] - u[2] * v[1]) + a[1] * (u[2] * v[0] - u[0] * v[2]) + a[2] * (u[0] * v[1] - u[1] * v[0]);
  long double den = 1.0L;
  for (int k = 0; k < 3; ++k) den += (long double)a[k] * b[k] + (long double)b[k] * c[k] + (long double)c[k] * a[k];
  return (double)(2.0L * atan2l(num, den));
}

static void test_area() {
  // the octant: area pi / 2 exactly (num = den = 1), four half-angle steps and the series
  const double a[3] = {1, 0, 0}, b[3] = {0, 1, 0}, c[3] = {0, 0, 1};
  const double oct = c2_tri_area(a, b, c);
  CHECK(std::fabs(oct - M_PI / 2) <= 4e-16 * M_PI, "octant area %.17g", oct);
  CHECK(c2_tri_area(a, c, b) == -oct, "the reversed triangle has the negated area");
  // a sweep of sizes from 1e-7 to 1 radian against 2 atan2 in long double: a few units in the last place
  double worst = 0.0;
  for (int k = 0; k <= 28; ++k) {
    const double h = std::pow(10.0, -7.0 + 0.25 * k);
    double p[3], q[3], r[3];
    unit(1.0, 0.3 * h, -0.2 * h, p);
    unit(1.0, -0.5 * h, 0.4 * h, q);
    unit(1.0, 0.6 * h, 0.7 * h, r);
    const double got = c2_tri_area(p, q, r), want = ref_area(p, q, r);
    const double rel = std::fabs(got - want) / std::fabs(want);
    worst = rel > worst ? rel : worst;
  }
  std::printf("area: worst relative distance from 2 atan2 %.3e\n", worst);
  CHECK(worst <= 4e-15, "area sweep %.3e", worst);
  // an excess of pi or more (den <= 0) is no cell's: 0
  double e[3], f[3];
  unit(-0.5, 0.75, 0.0, e);
  unit(-0.5, -0.75, 0.0, f);
  CHECK(c2_tri_area(a, e, f) == 0.0, "den <= 0 gives 0");
}

static void test_moment() {
  // one triangle: m = a * (p0 + p1 + p2) / 3
  const double p[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  double m[3];
  const double ar = c2_poly_moment(p, 3, m);
  CHECK(ar == c2_tri_area(p[0], p[1], p[2]), "a triangle's fan is the triangle");
  for (int k = 0; k < 3; ++k) CHECK(std::fabs(m[k] - ar / 3.0) <= 2e-16, "triangle moment[%d] %.17g", k, m[k]);
  // a square about the z axis split along either diagonal: the same area and moment (symmetry), the moment along z
  const double h = 0.0078125;
  double s[4][3], t[4][3];
  unit(h, h, 1, s[0]); unit(-h, h, 1, s[1]); unit(-h, -h, 1, s[2]); unit(h, -h, 1, s[3]);
  for (int k = 0; k < 4; ++k)
    for (int c = 0; c < 3; ++c) t[k][c] = s[(k + 1) % 4][c];
  double ms[3], mt[3];
  const double as = c2_poly_moment(s, 4, ms), at = c2_poly_moment(t, 4, mt);
  CHECK(as > 0.0 && std::fabs(as - at) <= 4e-16 * as, "square areas %.17g %.17g", as, at);
  CHECK(std::fabs(ms[2] - mt[2]) <= 4e-16 * as, "square moments %.17g %.17g", ms[2], mt[2]);
  CHECK(std::fabs(ms[0]) <= 1e-18 && std::fabs(ms[1]) <= 1e-18 && std::fabs(mt[0]) <= 1e-18 && std::fabs(mt[1]) <= 1e-18, "the moment lies on the axis");
  const double want = ref_area(s[0], s[1], s[2]) + ref_area(s[0], s[2], s[3]);
  CHECK(std::fabs(as - want) <= 1e-13 * want, "square area %.17g against %.17g", as, want);
  double g[3];
  CHECK(c2_unit(ms, g) && g[2] == 1.0 && std::fabs(g[0]) <= 1e-14 && std::fabs(g[1]) <= 1e-14, "the centroid is the axis");
  const double zero[3] = {0, 0, 0};
  g[0] = 7.0;
  CHECK(!c2_unit(zero, g) && g[0] == 7.0, "a zero moment leaves the fallback in place");
  // the clockwise square: negated area, negated moment
  double r[4][3], mr[3];
  for (int k = 0; k < 4; ++k)
    for (int c = 0; c < 3; ++c) r[k][c] = s[3 - k][c];
  const double arv = c2_poly_moment(r, 4, mr);
  CHECK(arv < 0.0 && std::fabs(arv + as) <= 4e-16 * as && mr[2] < 0.0, "clockwise: %.17g", arv);
  std::printf("moment: checked\n");
}

static void test_stencil() {
  double b[8][2], bi[2];
  // the symmetric cross at h = 1/2: M = diag(1/2, 1/2), b_k = 2 d_k exactly
  const double cross[4][2] = {{0.5, 0}, {-0.5, 0}, {0, 0.5}, {0, -0.5}};
  CHECK(c2_stencil(cross, 4, b, bi), "the cross passes");
  for (int k = 0; k < 4; ++k) CHECK(b[k][0] == 2 * cross[k][0] && b[k][1] == 2 * cross[k][1], "cross b[%d] = (%g, %g)", k, b[k][0], b[k][1]);
  CHECK(bi[0] == 0.0 && bi[1] == 0.0, "cross b_i = 0");
  std::printf("cross: pass\n");
  // collinear, one and zero neighbours: first order
  const double line[3][2] = {{0.25, 0}, {0.5, 0}, {-0.25, 0}};
  CHECK(!c2_stencil(line, 3, b, bi) && bi[0] == 0.0 && bi[1] == 0.0, "collinear neighbours fail");
  const double tilted[3][2] = {{0.25, 0.5}, {0.5, 1.0}, {-0.25, -0.5}};
  CHECK(!c2_stencil(tilted, 3, b, bi), "collinear neighbours on a tilted line fail");
  CHECK(!c2_stencil(cross, 1, b, bi) && bi[0] == 0.0, "one neighbour fails");
  CHECK(!c2_stencil(cross, 0, b, bi) && bi[1] == 0.0, "zero neighbours fail");
  std::printf("collinear: fail\none neighbour: fail\nzero neighbours: fail\n");
  // an irregular stencil: sum b = 0 by construction, and sum_k b_k d_k^T = I (a linear field's gradient is reproduced)
  const double irr[6][2] = {{0.31, 0.02}, {0.11, 0.27}, {-0.23, 0.19}, {-0.29, -0.08}, {-0.05, -0.33}, {0.21, -0.24}};
  CHECK(c2_stencil(irr, 6, b, bi), "the irregular stencil passes");
  double sx = 0.0, sy = 0.0, g[2][2] = {{0, 0}, {0, 0}};
  for (int k = 0; k < 6; ++k) {
    sx = sx + b[k][0];
    sy = sy + b[k][1];
    for (int r = 0; r < 2; ++r)
      for (int c = 0; c < 2; ++c) g[r][c] += b[k][r] * irr[k][c];
  }
  CHECK(bi[0] + sx == 0.0 && bi[1] + sy == 0.0, "sum b = 0 exactly: %g %g", bi[0] + sx, bi[1] + sy);
  CHECK(std::fabs(g[0][0] - 1) <= 1e-14 && std::fabs(g[1][1] - 1) <= 1e-14 && std::fabs(g[0][1]) <= 1e-14 && std::fabs(g[1][0]) <= 1e-14,
        "sum b d^T = I: %g %g %g %g", g[0][0], g[0][1], g[1][0], g[1][1]);
  std::printf("irregular: pass, sum b = 0\n");
  // near-collinear on either side of the 2^-26 rule: d = (1, 1), (-1, -1), (0, eta) has M = [[2, 2], [2, 2 + eta^2]], every number exact:
  // det = 2 eta^2 against 2^-26 * (4 + 2 eta^2)
  const double e_pass = 0x1p-12, e_fail = 0x1p-13;
  const double near1[3][2] = {{1, 1}, {-1, -1}, {0, e_pass}}, near2[3][2] = {{1, 1}, {-1, -1}, {0, e_fail}};
  CHECK(c2_stencil(near1, 3, b, bi), "eta = 2^-12: det = 2^-23 > 2^-24 + 2^-49");
  CHECK(!c2_stencil(near2, 3, b, bi), "eta = 2^-13: det = 2^-25 < 2^-24 + 2^-51");
  std::printf("near-collinear 2^-12: pass\nnear-collinear 2^-13: fail\n");
}

static void test_offsets() {
  const double e1[3] = {1, 0, 0}, e2[3] = {0, 1, 0};
  const double mq[3] = {0.5, 0.25, 2.0}, Mi[3] = {1.0, 1.0, 8.0};
  double dx, dy;
  c2_offset(mq, 2.0, Mi, 8.0, e1, e2, dx, dy);
  CHECK(dx == 0.125 && dy == 0.0, "offset (%g, %g)", dx, dy);
  c2_offset(mq, 0.0, Mi, 8.0, e1, e2, dx, dy);
  CHECK(dx == 0.0 && dy == 0.0, "A_q = 0: no offset");
  c2_offset(mq, 2.0, Mi, 0.0, e1, e2, dx, dy);
  CHECK(dx == 0.0 && dy == 0.0, "A_i = 0: no offset");
  CHECK(c2_t(0.125, 0.5, 2.0, 4.0, false) == 2.25 && c2_t(0.125, 0.5, 2.0, 4.0, true) == 3.25, "t");
  CHECK(c2_t(0.125, 0.5, 0.0, 0.0, true) == 1.0, "a failing stencil's own entry is 1");
  std::printf("offsets: checked\n");
}

int main() {
  test_area();
  test_moment();
  test_stencil();
  test_offsets();
  std::printf(g_fail ? "%d checks FAILED\n" : "ok\n", g_fail);
  return g_fail ? 1 : 0;
}
