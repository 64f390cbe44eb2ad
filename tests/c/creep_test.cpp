// Host test of mpassit_amd/csrc/creep.h (tests/test_creep_host.py builds and runs it): the text the kernels of k_creep.hip compile.  The
// grid neighbourhoods at the smallest shapes; the mesh neighbourhoods through PtSrc::ring1 on a hexagon, a rim cell with an invalid
// triangle and a bare cell; the level predicate; and the ordered merge-and-divide on dyadic values, where every sum and every division by
// m = 1, 2, 8 is exact, so the expected row is known without rounding -- once through cr_merge_row and once the way the device goes
// (a stable sort by column, cr_sum_div over every run), which must give the same bits.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../mpassit_amd/csrc/creep.h"

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

typedef std::vector<int32_t> Ids;

static Ids grid_nb(int snx, int sny, int32_t p) {
  int32_t ids[8];
  const int n = cr_neighbours_grid(snx, sny, p, ids);
  return Ids(ids, ids + n);
}

static void expect_ids(const char *what, const Ids &got, const Ids &want) {
  CHECK(got == want, "%s: %zu neighbours, %zu expected", what, got.size(), want.size());
  CHECK(std::is_sorted(got.begin(), got.end()), "%s: not ascending", what);
}

static void test_grid() {
  expect_ids("1x1", grid_nb(1, 1, 0), {});
  expect_ids("1x5 end", grid_nb(1, 5, 0), {1});
  expect_ids("1x5 middle", grid_nb(1, 5, 2), {1, 3});
  expect_ids("1x5 last", grid_nb(1, 5, 4), {3});
  expect_ids("5x1 middle", grid_nb(5, 1, 2), {1, 3});
  for (int p = 0; p < 4; ++p) {
    Ids want;
    for (int q = 0; q < 4; ++q)
      if (q != p) want.push_back(q);
    expect_ids("2x2", grid_nb(2, 2, p), want);
  }
  expect_ids("3x3 corner", grid_nb(3, 3, 0), {1, 3, 4});
  expect_ids("3x3 far corner", grid_nb(3, 3, 8), {4, 5, 7});
  expect_ids("3x3 edge", grid_nb(3, 3, 1), {0, 2, 3, 4, 5});
  expect_ids("3x3 left edge", grid_nb(3, 3, 3), {0, 1, 4, 6, 7});
  expect_ids("3x3 centre", grid_nb(3, 3, 4), {0, 1, 2, 3, 5, 6, 7, 8});
  expect_ids("4x3 border: no shifted window", grid_nb(4, 3, 3), {2, 6, 7});
  // through the destination set, as the kernels call it
  PtSrc d{};
  d.snx = 3; d.sny = 3;
  int32_t ids[CR_MAX_NB];
  const int n = cr_neighbours(d, 4, ids);
  CHECK(n == 8 && ids[0] == 0 && ids[3] == 3 && ids[4] == 5 && ids[7] == 8, "cr_neighbours on a grid");
  printf("grid: checked\n");
}

// a hexagon (cell 0) with its six neighbours 1 .. 6: vertex v (1-based v + 1) is shared by cells 0, v + 1 and (v + 1) % 6 + 1.  Cell 7 is
// a rim cell: it lists vertex 7 (triangle 1, 2, 7: valid) and vertex 8, whose triangle lacks a cell (-1).  Cell 8 is bare.
static void test_mesh() {
  const int nC = 9, mE = 6, nV = 8;
  std::vector<int32_t> voc(nC * mE, 0), tri(3 * nV, -1);
  for (int v = 0; v < 6; ++v) {
    tri[v] = 0; tri[nV + v] = v + 1; tri[2 * nV + v] = (v + 1) % 6 + 1;
    voc[0 * mE + v] = v + 1;
  }
  for (int c = 1; c <= 6; ++c) {   // neighbour c lists the two hexagon vertices it touches: v = c - 1 and v = c - 2 (mod 6)
    voc[c * mE + 0] = c;
    voc[c * mE + 1] = (c + 4) % 6 + 1;
  }
  tri[6] = 1; tri[nV + 6] = 2; tri[2 * nV + 6] = 7;       // vertex 7 (index 6): cells 1, 2, 7
  tri[7] = 2; tri[nV + 7] = -1; tri[2 * nV + 7] = 7;      // vertex 8 (index 7): one cell missing
  voc[1 * mE + 2] = 7; voc[2 * mE + 2] = 7;
  voc[7 * mE + 0] = 7; voc[7 * mE + 1] = 8; voc[7 * mE + 2] = 99;   // (99: beyond nV, skipped as ring1 skips it)
  PtSrc d{};
  d.voc = voc.data(); d.tri = tri.data(); d.maxEdges = mE; d.nV = nV;
  int32_t ids[CR_MAX_NB];
  int n = cr_neighbours(d, 0, ids);
  expect_ids("hexagon centre", Ids(ids, ids + n), {1, 2, 3, 4, 5, 6});
  n = cr_neighbours(d, 7, ids);
  expect_ids("rim cell: the invalid triangle adds nothing", Ids(ids, ids + n), {1, 2});
  n = cr_neighbours(d, 1, ids);
  expect_ids("hexagon neighbour", Ids(ids, ids + n), {0, 2, 6, 7});
  n = cr_neighbours(d, 8, ids);
  expect_ids("bare cell", Ids(ids, ids + n), {});
  // N1 itself still holds the cell: the neighbours are ring1 minus p, not a copy of it
  int32_t ring[PT_MAX_PNTS];
  CHECK(d.ring1(0, ring) == 7 && ring[0] == 0, "ring1 holds the cell itself");
  printf("mesh: checked\n");
}

static void test_levels() {
  const int32_t level[6] = {0, 1, CR_UNASSIGNED, CR_SKIPPED, 2, 0};
  const int32_t a[2] = {2, 3}, b[3] = {2, 1, 3}, c[1] = {4};
  CHECK(!cr_joins(level, a, 2, 1) && !cr_joins(level, a, 2, 2), "unassigned and skipped neighbours contribute nothing");
  CHECK(cr_joins(level, b, 3, 2) && !cr_joins(level, b, 3, 1) && !cr_joins(level, b, 3, 3), "level 1 neighbour: level 2 only");
  CHECK(cr_joins(level, c, 1, 3) && !cr_joins(level, c, 0, 3), "no neighbours, no level");
  CHECK(CR_UNASSIGNED < 0 && CR_SKIPPED < 0 && CR_UNASSIGNED != CR_SKIPPED, "markers are no levels");
  printf("levels: checked\n");
}

// the device's way: a stable sort of the candidates by column, one cr_sum_div per run
static int by_sort(const std::vector<int32_t> &cc, const std::vector<double> &cv, int m, std::vector<int32_t> &col, std::vector<double> &val) {
  std::vector<int> idx(cc.size());
  for (size_t k = 0; k < idx.size(); ++k) idx[k] = (int)k;
  std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return cc[x] < cc[y]; });
  col.clear(); val.clear();
  for (size_t i = 0; i < idx.size();) {
    size_t len = 1;
    while (i + len < idx.size() && cc[idx[i + len]] == cc[idx[i]]) ++len;
    col.push_back(cc[idx[i]]);
    val.push_back(cr_sum_div((int64_t)len, [&](int64_t k) { return cv[idx[i + k]]; }, m));
    i += len;
  }
  return (int)col.size();
}

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

static void merge_case(const char *what, const std::vector<std::vector<std::pair<int32_t, double>>> &rows, const std::vector<int32_t> &wcol,
                       const std::vector<double> &wval) {
  std::vector<int32_t> cc;
  std::vector<double> cv;
  for (const auto &r : rows)
    for (const auto &e : r) {
      cc.push_back(e.first);
      cv.push_back(e.second);
    }
  const int m = (int)rows.size();
  std::vector<int32_t> col(cc.size() + 1);
  std::vector<double> val(cc.size() + 1);
  const int n = cr_merge_row(cc.data(), cv.data(), (int64_t)cc.size(), m, col.data(), val.data(), (int)cc.size());
  CHECK(n == (int)wcol.size(), "%s: %d columns, %zu expected", what, n, wcol.size());
  for (int k = 0; k < n && k < (int)wcol.size(); ++k)
    CHECK(col[k] == wcol[k] && same_bits(val[k], wval[k]), "%s: entry %d is (%d, %a), expected (%d, %a)", what, k, col[k], val[k], wcol[k], wval[k]);
  std::vector<int32_t> scol;
  std::vector<double> sval;
  const int ns = by_sort(cc, cv, m, scol, sval);
  CHECK(ns == n, "%s: the sorted path has %d columns, the merge %d", what, ns, n);
  for (int k = 0; k < n && k < ns; ++k) CHECK(scol[k] == col[k] && same_bits(sval[k], val[k]), "%s: the sorted path differs at entry %d", what, k);
  if (!wcol.empty()) CHECK(cr_merge_row(cc.data(), cv.data(), (int64_t)cc.size(), m, col.data(), val.data(), (int)wcol.size() - 1) == -1, "%s: the cap", what);
}

static void test_merge() {
  // m = 1: the neighbour's row sorted and merged; values that appear once are copied exactly (0.1 and 1/3 are not dyadic)
  merge_case("m = 1", {{{9, 0.1}, {2, 0.25}, {9, 0.5}, {4, 1.0 / 3.0}, {2, 0.125}}}, {2, 4, 9}, {0.375, 1.0 / 3.0, (0.0 + 0.1) + 0.5});
  // m = 2: the exact half-sum, a column of one row only is halved, a zero value stays in the row
  merge_case("m = 2", {{{5, 0.5}, {1, 0.25}, {7, 0.0}}, {{1, 0.75}, {6, 0.125}, {5, -0.5}}}, {1, 5, 6, 7}, {0.5, 0.0, 0.0625, 0.0});
  // m = 8: eight contributors, a duplicate column inside one of them is one term each
  std::vector<std::vector<std::pair<int32_t, double>>> rows;
  for (int q = 0; q < 8; ++q) rows.push_back({{3, 0.125 * (q + 1)}, {100 - q, 1.0}});
  rows[4].push_back({3, 2.0});
  std::vector<int32_t> wcol = {3};
  std::vector<double> wval = {(0.125 * 36 + 2.0) / 8.0};
  for (int q = 7; q >= 0; --q) {
    wcol.push_back(100 - q);
    wval.push_back(0.125);
  }
  merge_case("m = 8", rows, wcol, wval);
  // the order of the sum is the candidates': (2^53 + 1) + (-2^53) is 0 in that order (the 1 is lost), 1 in the other
  const double big = 9007199254740992.0;
  merge_case("order", {{{0, big}}, {{0, 1.0}}, {{0, -big}}, {{0, 0.0}}}, {0}, {0.0});
  merge_case("order reversed", {{{0, big}}, {{0, -big}}, {{0, 1.0}}, {{0, 0.0}}}, {0}, {0.25});
  // -0.0 alone: 0.0 + -0.0 = +0.0, as every column starts from 0.0
  merge_case("minus zero", {{{1, -0.0}}}, {1}, {0.0});
  printf("merge: checked\n");
}

int main() {
  test_grid();
  test_mesh();
  test_levels();
  test_merge();
  if (g_fail) {
    printf("%d FAILED\n", g_fail);
    return 1;
  }
  printf("ok\n");
  return 0;
}
