// Host test of mpassit_amd/csrc/patch.h (tests/test_patch_host.py builds and runs it): the text the kernels of k_patch.hip compile, on
// exact lattice inputs.  The points of a case are (i * s, j * s, 1) with integers i, j and s = 2^-6 about the centre (0, 0, 1), whose frame
// is e1 = x, e2 = y; the shape values of a least-squares fit do not depend on the scale of the coordinates, so the expected values come
// from the integer lattice itself in rational arithmetic (__int128 fractions, Gaussian elimination on the normal equations).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <vector>

#include "../../mpassit_amd/csrc/patch.h"

static int g_fail = 0;
#define CHECK(c, ...)                                   \
  do {                                                  \
    if (!(c)) {                                         \
      printf("FAIL %s:%d: ", __FILE__, __LINE__);       \
      printf(__VA_ARGS__);                              \
      printf("\n");                                     \
      ++g_fail;                                         \
    }                                                   \
  } while (0)

typedef __int128 i128;
static i128 gcd128(i128 a, i128 b) {
  if (a < 0) a = -a;
  if (b < 0) b = -b;
  while (b) {
    i128 t = a % b;
    a = b;
    b = t;
  }
  return a ? a : 1;
}
struct Q {
  i128 n, d;
  Q(long long v = 0) : n(v), d(1) {}
  Q(i128 a, i128 b) : n(a), d(b) {
    if (d < 0) { n = -n; d = -d; }
    i128 g = gcd128(n, d);
    n /= g; d /= g;
  }
  Q operator+(const Q &o) const { return Q(n * o.d + o.n * d, d * o.d); }
  Q operator-(const Q &o) const { return Q(n * o.d - o.n * d, d * o.d); }
  Q operator*(const Q &o) const { return Q(n * o.n, d * o.d); }
  Q operator/(const Q &o) const { return Q(n * o.d, d * o.n); }
  bool zero() const { return n == 0; }
  long double val() const { return (long double)n / (long double)d; }
};

static void phi_int(long long u, long long v, int M, Q *phi) {
  phi[0] = Q(1); phi[1] = Q(u); phi[2] = Q(v);
  if (M == 6) { phi[3] = Q(u * u); phi[4] = Q(u * v); phi[5] = Q(v * v); }
}

// the exact shape values of the degree-(M == 6 ? 2 : 1) fit through the lattice points at the lattice point p; false: G is singular
static bool exact_shape(const std::vector<std::pair<int, int>> &pts, int pu, int pv, int M, std::vector<long double> &L) {
  Q A[6][7];
  for (auto &q : pts) {
    Q phi[6];
    phi_int(q.first, q.second, M, phi);
    for (int a = 0; a < M; ++a)
      for (int b = 0; b < M; ++b) A[a][b] = A[a][b] + phi[a] * phi[b];
  }
  Q rhs[6];
  phi_int(pu, pv, M, rhs);
  for (int a = 0; a < M; ++a) A[a][M] = rhs[a];
  for (int k = 0; k < M; ++k) {
    int p = k;
    while (p < M && A[p][k].zero()) ++p;
    if (p == M) return false;
    for (int j = 0; j <= M; ++j) std::swap(A[k][j], A[p][j]);
    for (int i = 0; i < M; ++i) {
      if (i == k || A[i][k].zero()) continue;
      const Q f = A[i][k] / A[k][k];
      for (int j = k; j <= M; ++j) A[i][j] = A[i][j] - f * A[k][j];
    }
  }
  L.clear();
  for (auto &q : pts) {
    Q phi[6], acc;
    phi_int(q.first, q.second, M, phi);
    for (int a = 0; a < M; ++a) acc = acc + phi[a] * (A[a][M] / A[a][a]);
    L.push_back(acc.val());
  }
  return true;
}

// a point set given as a mesh: cells with coordinates, triangles of three cells (one "vertex" each), and each cell's listed vertices
struct Case {
  std::vector<double> x, y, z;
  std::vector<int32_t> voc, tri;
  int maxEdges = 0;
  int64_t nV = 0;
  PtSrc src() const {
    PtSrc s;
    s.x = x.data(); s.y = y.data(); s.z = z.data();
    s.voc = voc.empty() ? nullptr : voc.data();
    s.tri = tri.empty() ? nullptr : tri.data();
    s.maxEdges = maxEdges; s.nV = nV; s.snx = 0; s.sny = 0;
    return s;
  }
};
static const double S = 0x1p-6;
static Case mesh_case(const std::vector<std::pair<int, int>> &cells, const std::vector<std::vector<int>> &tris, int maxEdges = 8) {
  Case c;
  for (auto &q : cells) { c.x.push_back(q.first * S); c.y.push_back(q.second * S); c.z.push_back(1.0); }
  c.maxEdges = maxEdges;
  c.nV = (int64_t)tris.size();
  c.tri.assign(3 * tris.size(), -1);
  c.voc.assign(cells.size() * maxEdges, 0);
  std::vector<int> used(cells.size(), 0);
  for (size_t v = 0; v < tris.size(); ++v)
    for (int k = 0; k < 3; ++k) {
      const int cell = tris[v][k];
      c.tri[k * tris.size() + v] = cell;
      if (cell >= 0) c.voc[cell * maxEdges + used[cell]++] = (int32_t)v + 1;
    }
  return c;
}
static Case grid_case(int snx, int sny, bool coincident = false) {
  Case c;
  for (int j = 0; j < sny; ++j)
    for (int i = 0; i < snx; ++i) { c.x.push_back(coincident ? 0.0 : i * S); c.y.push_back(coincident ? 0.0 : j * S); c.z.push_back(1.0); }
  return c;
}
static PtSrc grid_src(const Case &c, int snx, int sny) {
  PtSrc s = c.src();
  s.snx = snx; s.sny = sny;
  return s;
}

// node c's attempt and its shape values at the point (px, py, 1) -> (ids, L)
static int run_slot(const PtSrc &s, int32_t c, double px, double py, std::vector<int32_t> &ids, std::vector<double> &L) {
  int32_t a[PT_MAX_PNTS], b[PT_MAX_PNTS];
  const int att = pt_attempt(s, c, a, b);
  const double P[3] = {px, py, 1.0};
  ids.clear(); L.clear();
  pt_slot(s, c, att, P, a, b, [&](int32_t id, double l) { ids.push_back(id); L.push_back(l); });
  return att;
}

// lattice coordinates are doubled so that p may sit at half points (small integers keep the __int128 fractions far from overflow)
static void expect(const char *name, const PtSrc &s, const std::vector<std::pair<int, int>> &cells, int32_t c, int pu2, int pv2, int want_att,
                   const std::vector<int> &want_ids) {
  std::vector<int32_t> ids;
  std::vector<double> L;
  const double cx = s.x[c], cy = s.y[c];
  const int att = run_slot(s, c, cx + pu2 * (S / 2), cy + pv2 * (S / 2), ids, L);
  CHECK(att == want_att, "%s: attempt %d, expected %d", name, att, want_att);
  CHECK(ids.size() == want_ids.size(), "%s: %zu ids, expected %zu", name, ids.size(), want_ids.size());
  for (size_t k = 0; k < ids.size() && k < want_ids.size(); ++k) CHECK(ids[k] == want_ids[k], "%s: id %zu is %d, expected %d", name, k, ids[k], want_ids[k]);
  double sum = 0.0;
  for (double l : L) sum += l;
  CHECK(fabs(sum - 1.0) <= 64 * 0x1p-52, "%s: the shape values sum to 1 %+g", name, sum - 1.0);
  if (att == PT_ATT_D) {
    CHECK(L.size() == 1 && L[0] == 1.0 && ids[0] == c, "%s: degree 0 is the node itself with value 1", name);
    printf("%s: attempt D\n", name);
    return;
  }
  std::vector<std::pair<int, int>> pts;
  const int cu = cells[c].first, cv = cells[c].second;
  for (int id : want_ids) pts.push_back({2 * (cells[id].first - cu), 2 * (cells[id].second - cv)});
  std::vector<long double> E;
  const bool ok = exact_shape(pts, pu2, pv2, att == PT_ATT_C ? 3 : 6, E);
  CHECK(ok, "%s: the exact normal equations are singular", name);
  double worst = 0.0;
  for (size_t k = 0; ok && k < L.size() && k < E.size(); ++k) worst = fmax(worst, (double)fabsl((long double)L[k] - E[k]));
  CHECK(worst <= 1e-12, "%s: worst |L - exact| = %g", name, worst);
  printf("%s: attempt %c, %zu points, worst |L - exact| %.3g, sum - 1 %+.3g\n", name, "ABCD"[att], L.size(), worst, sum - 1.0);
}

static std::vector<std::pair<int, int>> grid_cells(int snx, int sny) {
  std::vector<std::pair<int, int>> v;
  for (int j = 0; j < sny; ++j)
    for (int i = 0; i < snx; ++i) v.push_back({i, j});
  return v;
}
static std::vector<int> iota(int n) {
  std::vector<int> v(n);
  for (int i = 0; i < n; ++i) v[i] = i;
  return v;
}

int main() {
  // the frame of a generic unit vector is orthonormal, and the centre (0, 0, 1) has e1 = x, e2 = y
  {
    const double n[3] = {0.48, -0.6, 0.64};
    double e1[3], e2[3];
    pt_frame(n, e1, e2);
    CHECK(fabs(pt_dot(n, e1)) < 4e-16 && fabs(pt_dot(n, e2)) < 4e-16 && fabs(pt_dot(e1, e2)) < 4e-16, "frame: not orthogonal");
    CHECK(fabs(pt_dot(e1, e1) - 1) < 4e-16 && fabs(pt_dot(e2, e2) - 1) < 4e-16, "frame: not unit");
    const double t[3] = {0.5, 0.5, 0.70710678118654757};   // a tie between x and y: the lowest axis
    pt_frame(t, e1, e2);
    CHECK(e1[0] > 0.7 && fabs(e1[1]) < 0.6, "frame: the lowest axis on ties");
    const double z[3] = {0.0, 0.0, 1.0};
    pt_frame(z, e1, e2);
    CHECK(e1[0] == 1.0 && e1[1] == 0.0 && e1[2] == 0.0 && e2[0] == 0.0 && e2[1] == 1.0 && e2[2] == 0.0, "frame: the pole's frame");
    printf("frame: checked\n");
  }
  // a 3 x 3 block of a grid stagger: attempt A, from the centre, from a corner (the window keeps a full block) and off the lattice
  {
    Case c = grid_case(3, 3);
    PtSrc s = grid_src(c, 3, 3);
    auto cells = grid_cells(3, 3);
    expect("3x3 centre", s, cells, 4, 1, -2, PT_ATT_A, iota(9));
    expect("3x3 corner", s, cells, 0, 3, 1, PT_ATT_A, iota(9));
    Case c5 = grid_case(5, 4);
    PtSrc s5 = grid_src(c5, 5, 4);
    auto cells5 = grid_cells(5, 4);
    expect("5x4 border", s5, cells5, 19, -1, -3, PT_ATT_A, {7, 8, 9, 12, 13, 14, 17, 18, 19});
    expect("5x4 inner", s5, cells5, 7, 2, 2, PT_ATT_A, {1, 2, 3, 6, 7, 8, 11, 12, 13});
  }
  // a 2 x 3 block: six points, G of rank 5 (v * v = v on two rows), a grid has no ring 2: falls to C
  {
    Case c = grid_case(3, 2);
    PtSrc s = grid_src(c, 3, 2);
    expect("2x3 block", s, grid_cells(3, 2), 1, 1, 2, PT_ATT_C, iota(6));
    Case d = grid_case(2, 5);
    PtSrc sd = grid_src(d, 2, 5);
    expect("5x2 block", sd, grid_cells(2, 5), 4, 1, 1, PT_ATT_C, {2, 3, 4, 5, 6, 7});
    Case e = grid_case(2, 2);
    PtSrc se = grid_src(e, 2, 2);
    expect("2x2 block", se, grid_cells(2, 2), 3, -1, -1, PT_ATT_C, iota(4));
  }
  // five points of a mesh (an open fan: N2 = N1, too few for degree 2): C
  {
    std::vector<std::pair<int, int>> cells = {{0, 0}, {2, 0}, {1, 2}, {-1, 2}, {-2, 0}};
    Case c = mesh_case(cells, {{0, 1, 2}, {0, 2, 3}, {0, 3, 4}});
    expect("five points", c.src(), cells, 0, 1, 1, PT_ATT_C, iota(5));
  }
  // three collinear points: degree 1 is rank deficient too: D; two points; one point; a coincident patch (h = 0)
  {
    std::vector<std::pair<int, int>> cells = {{0, 0}, {1, 0}, {2, 0}};
    Case c = mesh_case(cells, {{0, 1, 2}});
    expect("three collinear", c.src(), cells, 1, 1, 0, PT_ATT_D, {1});
    Case two = grid_case(2, 1);
    expect("two points", grid_src(two, 2, 1), grid_cells(2, 1), 0, 1, 0, PT_ATT_D, {0});
    Case lone = mesh_case({{0, 0}, {1, 0}, {0, 1}}, {{0, 1, -1}});
    expect("invalid triangle", lone.src(), {{0, 0}, {1, 0}, {0, 1}}, 0, 1, 0, PT_ATT_D, {0});
    Case co = grid_case(3, 3, true);
    expect("coincident", grid_src(co, 3, 3), grid_cells(3, 3), 4, 0, 0, PT_ATT_D, {4});
  }
  // a valence-4 cell of a mesh: N1 has five points, N2 is the whole 3 x 3 block: B, with the values of the 3 x 3 fit
  {
    auto cells = grid_cells(3, 3);
    Case c = mesh_case(cells, {{4, 1, 3}, {4, 1, 5}, {4, 3, 7}, {4, 5, 7}, {0, 1, 3}, {1, 2, 5}, {3, 6, 7}, {5, 7, 8}});
    int32_t a[PT_MAX_PNTS];
    PtSrc s = c.src();
    CHECK(s.ring1(4, a) == 5 && a[0] == 1 && a[4] == 7, "valence 4: N1");
    expect("valence 4", s, cells, 4, 1, -2, PT_ATT_B, iota(9));
  }
  // a hexagon and its centre (the lattice of a sheared hexagon keeps the coordinates integral): A, seven points for six coefficients
  {
    std::vector<std::pair<int, int>> cells = {{0, 0}, {2, 0}, {1, 2}, {-1, 2}, {-2, 0}, {-1, -2}, {1, -2}};
    Case c = mesh_case(cells, {{0, 1, 2}, {0, 2, 3}, {0, 3, 4}, {0, 4, 5}, {0, 5, 6}, {0, 6, 1}});
    expect("hexagon", c.src(), cells, 0, 1, 1, PT_ATT_A, iota(7));
    expect("hexagon at a node", c.src(), cells, 0, 4, 0, PT_ATT_A, iota(7));
  }
  // a pentagon and its centre: six points, exactly determined: L at node j is the j-th unit vector
  {
    Case c;
    c.x.push_back(0.0); c.y.push_back(0.0); c.z.push_back(1.0);
    for (int k = 0; k < 5; ++k) {
      const double a = 2.0 * M_PI * k / 5.0 + 0.3;
      c.x.push_back(0.02 * cos(a)); c.y.push_back(0.02 * sin(a)); c.z.push_back(sqrt(1.0 - 0.0004));
    }
    std::vector<std::vector<int>> tris = {{0, 1, 2}, {0, 2, 3}, {0, 3, 4}, {0, 4, 5}, {0, 5, 1}};
    Case t = mesh_case({{0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}}, tris);
    c.voc = t.voc; c.tri = t.tri; c.maxEdges = t.maxEdges; c.nV = t.nV;
    PtSrc s = c.src();
    int32_t a[PT_MAX_PNTS], b[PT_MAX_PNTS];
    const int att = pt_attempt(s, 0, a, b);
    CHECK(att == PT_ATT_A, "pentagon: attempt %d", att);
    double worst = 0.0;
    for (int j = 0; j < 6; ++j) {
      const double P[3] = {c.x[j], c.y[j], c.z[j]};
      int pos = 0;
      pt_slot(s, 0, att, P, a, b, [&](int32_t id, double l) {
        CHECK(id == pos, "pentagon: id");
        worst = fmax(worst, fabs(l - (pos == j ? 1.0 : 0.0)));
        ++pos;
      });
      CHECK(pos == 6, "pentagon: six points");
    }
    CHECK(worst <= 1e-12, "pentagon: worst |L - unit vector| = %g", worst);
    printf("pentagon: attempt A, exactly determined, worst |L - unit vector| %.3g\n", worst);
  }
  // a patch beyond PT_MAX_PNTS points: a cell with 16 disjoint triangles (33 cells): D
  {
    std::vector<std::pair<int, int>> cells = {{0, 0}};
    std::vector<std::vector<int>> tris;
    for (int k = 0; k < 16; ++k) {
      cells.push_back({k + 1, 1}); cells.push_back({k + 1, 2});
      tris.push_back({0, 2 * k + 1, 2 * k + 2});
    }
    Case c = mesh_case(cells, tris, 16);
    int32_t a[PT_MAX_PNTS];
    CHECK(c.src().ring1(0, a) == PT_MAX_PNTS + 1, "33 points: ring1 reports the overflow");
    expect("33 points", c.src(), cells, 0, 1, 1, PT_ATT_D, {0});
  }
  // the ordered merge: duplicates across slots, all 3 * 32 candidates distinct, the cap
  {
    int32_t col[PT_MAX_SLOTS * PT_MAX_PNTS];
    double val[PT_MAX_SLOTS * PT_MAX_PNTS];
    int n = 0;
    std::map<int32_t, double> want;
    unsigned r = 12345u;
    for (int s = 0; s < 3; ++s) {
      std::vector<int32_t> ids;
      for (int k = 0; k < 12; ++k) { r = r * 1664525u + 1013904223u; ids.push_back((int32_t)((r >> 16) % 20)); }
      std::sort(ids.begin(), ids.end());
      ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
      for (int32_t id : ids) {
        r = r * 1664525u + 1013904223u;
        const double term = ((int)(r >> 8) % 2001 - 1000) / 1024.0 / 3.0;
        CHECK(pt_row_add(col, val, n, PT_MAX_SLOTS * PT_MAX_PNTS, id, term), "merge: refused");
        want[id] = (want.count(id) ? want[id] : 0.0) + term;   // the same order: (slot, position)
      }
    }
    CHECK((size_t)n == want.size(), "merge: %d columns, expected %zu", n, want.size());
    int k = 0;
    for (auto &e : want) {
      CHECK(col[k] == e.first && val[k] == e.second, "merge: column %d", k);
      ++k;
    }
    n = 0;
    CHECK(pt_row_add(col, val, n, 4, 7, -0.0) && val[0] == 0.0 && !signbit(val[0]), "merge: a new column starts from 0.0 + term");
    n = 0;
    int m = 0;
    int32_t set[PT_MAX_SLOTS * PT_MAX_PNTS];
    for (int s = 0; s < 3; ++s)
      for (int q = 0; q < PT_MAX_PNTS; ++q) {   // 96 distinct ids, interleaved across the slots
        const int32_t id = 3 * (PT_MAX_PNTS - 1 - q) + s;
        CHECK(pt_row_add(col, val, n, PT_MAX_SLOTS * PT_MAX_PNTS, id, 1.0 + id), "merge: refused");
        CHECK(pt_set_add(set, m, PT_MAX_SLOTS * PT_MAX_PNTS, id) && pt_set_add(set, m, PT_MAX_SLOTS * PT_MAX_PNTS, id), "set: refused");
      }
    CHECK(n == 96 && m == 96, "merge: %d / %d of 96 candidates", n, m);
    for (int q = 0; q < 96; ++q) CHECK(col[q] == q && set[q] == q && val[q] == 1.0 + q, "merge: 96 candidates, column %d", q);
    n = 2;
    col[0] = 1; col[1] = 5;
    CHECK(!pt_row_add(col, val, n, 2, 3, 1.0) && n == 2 && col[0] == 1 && col[1] == 5, "merge: a full row refuses a new column and stays as it is");
    CHECK(pt_row_add(col, val, n, 2, 5, 1.0) && n == 2, "merge: a full row still takes a known column");
    printf("merge: checked\n");
  }
  if (g_fail) {
    printf("%d checks failed\n", g_fail);
    return 1;
  }
  printf("ok\n");
  return 0;
}
