// Host run of the K-nearest search and the extrapolation weights (mpassit_amd/csrc/knn.h): the text the kernels compile, on trees built here.
//   knn_search returns the K smallest (d2, id) pairs of a brute-force sort -- ties to the lower id at every rank, exact duplicates among
//   the items, K above the number of items included -- through both tree kinds, and its stack stays within WalkCap<>::NEAREST;
//   knn_weights obeys the coincidence rule, keeps the order, equals rational arithmetic for e == 2 on exact inputs, and sums to 1 within
//   K eps.
// Coordinates are multiples of 1/8 in [0, 4): every squared distance is exact in double, so equal distances are equal bit for bit.
// Exit status 0 and a last line "ok" when everything holds.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../mpassit_amd/csrc/knn.h"

static unsigned long long rng_state = 0x2545f4914f6cdd1dull;
static unsigned rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (unsigned)(rng_state >> 33);
}
static double coord() { return (rnd() % 32) / 8.0; }

struct Pt {
  double x, y, z;
};
static double dist2(const Pt &a, const Pt &b) { return ((a.x - b.x) * (a.x - b.x) + (a.y - b.y) * (a.y - b.y)) + (a.z - b.z) * (a.z - b.z); }
static double boxdist2(const Pt &p, const double *bx) {
  const double dx = std::max(std::max(bx[0] - p.x, p.x - bx[3]), 0.0), dy = std::max(std::max(bx[1] - p.y, p.y - bx[4]), 0.0),
               dz = std::max(std::max(bx[2] - p.z, p.z - bx[5]), 0.0);
  return (dx * dx + dy * dy) + dz * dz;
}
static void box_add(double *bx, const double *c) {
  for (int k = 0; k < 3; ++k) {
    bx[k] = std::min(bx[k], c[k]);
    bx[3 + k] = std::max(bx[3 + k], c[3 + k]);
  }
}
static void box_empty(double *bx) {
  bx[0] = bx[1] = bx[2] = 1e9;
  bx[3] = bx[4] = bx[5] = -1e9;
}

static int failures = 0;
#define CHECK(cond, ...)          \
  do {                            \
    if (!(cond)) {                \
      ++failures;                 \
      std::printf("FAIL: ");      \
      std::printf(__VA_ARGS__);   \
      std::printf("\n");          \
    }                             \
  } while (0)

// items(node, f): f(id, point) for every item of leaf `node`; pts / ids: all items, for the brute force
template <int K, class Tree, class Items>
static void check_knn(const Tree &t, const std::vector<Pt> &pts, const std::vector<int> &ids, Items items, const char *what, int *deepest) {
  int wrong = 0;
  const int n = (int)pts.size(), want = std::min(n, K);
  for (int q = 0; q < 120; ++q) {
    // a third of the queries is an exact copy of an item, a third sits on the lattice, a third half a lattice step off: ties every way
    Pt p = {coord(), coord(), coord()};
    if (q % 3 == 0) p = pts[(size_t)(rnd() % (unsigned)n)];
    if (q % 3 == 2) p.x += 1.0 / 16.0;
    std::vector<std::pair<double, int>> all((size_t)n);
    for (int i = 0; i < n; ++i) all[(size_t)i] = {dist2(p, pts[(size_t)i]), ids[(size_t)i]};
    std::sort(all.begin(), all.end());
    KBest<K> best;
    knn_search(
        t, [&](const double *bx) { return boxdist2(p, bx); },
        [&](int node, auto f) { items(node, [&](int id, const Pt &s) { f(dist2(p, s), (int32_t)id); }); }, best, deepest);
    bool bad = best.n != want;
    for (int k = 0; k < K; ++k) {
      if (k < want) bad = bad || best.d2[k] != all[(size_t)k].first || best.id[k] != all[(size_t)k].second;
      else bad = bad || best.d2[k] != INFINITY || best.id[k] != 0x7fffffff;
    }
    wrong += bad;
  }
  CHECK(wrong == 0, "%s, K = %d: %d of 120 lists differ from the brute-force sort", what, K, wrong);
}

template <class Tree, class Items>
static void check_all_k(const Tree &t, const std::vector<Pt> &pts, const std::vector<int> &ids, Items items, const char *what) {
  int deepest = 0;
  check_knn<1>(t, pts, ids, items, what, &deepest);
  check_knn<2>(t, pts, ids, items, what, &deepest);
  check_knn<3>(t, pts, ids, items, what, &deepest);
  check_knn<4>(t, pts, ids, items, what, &deepest);
  check_knn<8>(t, pts, ids, items, what, &deepest);
  std::printf("%s: knn stack %d of %d\n", what, deepest, WalkCap<Tree>::NEAREST);
  CHECK(deepest <= WalkCap<Tree>::NEAREST, "%s: knn stack %d above its bound", what, deepest);
}

// the point pyramid of npx x npy points: leaves of MPG_PYR_B0 x MPG_PYR_B0 points, the last row / column of leaves ragged
static void test_pyramid(int npx, int npy) {
  const int lx = (npx + MPG_PYR_B0 - 1) / MPG_PYR_B0, ly = (npy + MPG_PYR_B0 - 1) / MPG_PYR_B0;
  std::vector<Pt> pts((size_t)npx * npy);
  std::vector<int> ids(pts.size());
  for (size_t i = 0; i < pts.size(); ++i) {
    pts[i] = (i % 7 == 3) ? pts[i - 3] : Pt{coord(), coord(), coord()};   // exact duplicates of earlier points
    ids[i] = (int)i;
  }
  PyramidView v;
  v.nlev = 0;
  int64_t total = 0;
  for (int nx = lx, ny = ly;; nx = (nx + 1) / 2, ny = (ny + 1) / 2) {
    v.nx[v.nlev] = nx;
    v.ny[v.nlev] = ny;
    v.off[v.nlev++] = total;
    total += (int64_t)nx * ny;
    if (nx == 1 && ny == 1) break;
  }
  v.off[v.nlev] = total;
  std::vector<double> box(6 * (size_t)total);
  for (int64_t n = 0; n < total; ++n) box_empty(&box[6 * n]);
  for (int j = 0; j < npy; ++j)
    for (int i = 0; i < npx; ++i) {
      const Pt &p = pts[(size_t)j * npx + i];
      const double c[6] = {p.x, p.y, p.z, p.x, p.y, p.z};
      box_add(&box[6 * ((int64_t)(j / MPG_PYR_B0) * lx + i / MPG_PYR_B0)], c);
    }
  for (int l = 1; l < v.nlev; ++l)
    for (int j = 0; j < v.ny[l - 1]; ++j)
      for (int i = 0; i < v.nx[l - 1]; ++i)
        box_add(&box[6 * (v.off[l] + (int64_t)(j / 2) * v.nx[l] + i / 2)], &box[6 * (v.off[l - 1] + (int64_t)j * v.nx[l - 1] + i)]);
  v.box = box.data();
  char what[64];
  std::snprintf(what, sizeof what, "grid %d x %d", npx, npy);
  const PyrTree t{v};
  check_all_k(t, pts, ids,
              [&](int node, auto f) {
                const int bi = node % lx, bj = node / lx;
                for (int j = bj * MPG_PYR_B0; j < std::min(bj * MPG_PYR_B0 + MPG_PYR_B0, npy); ++j)
                  for (int i = bi * MPG_PYR_B0; i < std::min(bi * MPG_PYR_B0 + MPG_PYR_B0, npx); ++i) f(j * npx + i, pts[(size_t)j * npx + i]);
              },
              what);
}

// BVH over n items sorted by a space-filling key of the lattice, ids a permutation
static void test_bvh(int n) {
  std::vector<Pt> pts((size_t)n);
  std::vector<int32_t> sid((size_t)n);
  for (int i = 0; i < n; ++i) pts[(size_t)i] = (i % 5 == 4) ? pts[(size_t)i - 2] : Pt{coord(), coord(), coord()};   // exact duplicates
  std::vector<int> order((size_t)n);
  for (int i = 0; i < n; ++i) order[(size_t)i] = i;
  auto key = [&](int i) { return ((int)(pts[(size_t)i].x) * 4 + (int)(pts[(size_t)i].y)) * 4 + (int)(pts[(size_t)i].z); };
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key(a) < key(b); });
  std::vector<Pt> sorted((size_t)n);
  std::vector<int> ids((size_t)n);
  for (int i = 0; i < n; ++i) {
    sorted[(size_t)i] = pts[(size_t)order[(size_t)i]];
    sid[(size_t)i] = order[(size_t)i];
    ids[(size_t)i] = order[(size_t)i];
  }
  BvhView v;
  v.n = n;
  v.sid = sid.data();
  v.nlev = 0;
  int64_t total = 0;
  for (int64_t cnt = (n + MPG_BVH_LEAF - 1) / MPG_BVH_LEAF;; cnt = (cnt + MPG_BVH_FAN - 1) / MPG_BVH_FAN) {
    v.nnodes[v.nlev] = cnt;
    v.off[v.nlev++] = total;
    total += cnt;
    if (cnt == 1) break;
  }
  v.off[v.nlev] = total;
  std::vector<double> box(6 * (size_t)total);
  for (int64_t k = 0; k < total; ++k) box_empty(&box[6 * k]);
  for (int i = 0; i < n; ++i) {
    const Pt &p = sorted[(size_t)i];
    const double c[6] = {p.x, p.y, p.z, p.x, p.y, p.z};
    box_add(&box[6 * (i / MPG_BVH_LEAF)], c);
  }
  for (int l = 1; l < v.nlev; ++l)
    for (int64_t c = 0; c < v.nnodes[l - 1]; ++c) box_add(&box[6 * (v.off[l] + c / MPG_BVH_FAN)], &box[6 * (v.off[l - 1] + c)]);
  v.box = box.data();
  char what[64];
  std::snprintf(what, sizeof what, "bvh %d", n);
  const BvhTree t{v};
  check_all_k(t, sorted, ids,
              [&](int node, auto f) {
                for (int64_t i = (int64_t)node * MPG_BVH_LEAF; i < std::min<int64_t>(n, ((int64_t)node + 1) * MPG_BVH_LEAF); ++i)
                  f(v.sid[i], sorted[(size_t)i]);
              },
              what);
}

// w == the double nearest to num / den (small positive integers): |w - num / den| <= ulp(w) / 2, in integers
static bool is_rounded_quotient(double w, long long num, long long den) {
  int ex;
  const double m = std::frexp(w, &ex);                 // w = m * 2^ex, m in [0.5, 1)
  const long long M = (long long)std::ldexp(m, 53);    // w = M * 2^(ex - 53), M an integer of 53 bits
  const int s = 53 - ex;                               // w = M / 2^s
  if (s < 0 || s > 70) return false;
  const __int128 diff = (__int128)M * den - ((__int128)num << s);   // (w - num / den) * den * 2^s
  const __int128 a = diff < 0 ? -diff : diff;
  return 2 * a <= den;
}

static void test_weights() {
  // the coincidence rule, nearest-source-to-destination, a single neighbour, nothing at all
  {
    double d[4] = {0.0, 0.5, 1.0, 2.0}, w[4] = {-1, -1, -1, -1};
    CHECK(knn_weights(d, 4, true, 2.0, w) == 1 && w[0] == 1.0, "a coincident nearest point must give one entry of weight 1");
    double d1[4] = {0.25, 0.5, 1.0, 2.0};
    CHECK(knn_weights(d1, 4, false, 2.0, w) == 1 && w[0] == 1.0, "nearest source to destination must give one entry of weight 1");
    CHECK(knn_weights(d1, 1, true, 3.5, w) == 1 && w[0] == 1.0, "one neighbour must have weight 1");
    CHECK(knn_weights(d1, 0, true, 2.0, w) == 0, "no neighbour, no entry");
  }
  // e == 2 on exact inputs: d2 = 1, 2, 4, 8 -> t = 1, 1/2, 1/4, 1/8, S = 15/8, w_i = (8 t_i) / 15 correctly rounded; k below K too
  {
    double d[8] = {1, 2, 4, 8, 16, 32, 64, 128}, w[8];
    const long long num[8] = {128, 64, 32, 16, 8, 4, 2, 1};
    for (int k = 2; k <= 8; ++k) {
      long long den = 0;
      for (int i = 0; i < k; ++i) den += num[i];
      CHECK(knn_weights(d, k, true, 2.0, w) == k, "e == 2: %d entries expected", k);
      for (int i = 0; i < k; ++i) CHECK(is_rounded_quotient(w[i], num[i], den), "e == 2, k = %d: w[%d] = %.17g is not %lld / %lld rounded", k, i, w[i], num[i], den);
    }
    // d2 = 3/64 and 5/64, 7/64: r_i is a rounded quotient itself; check the definition step by step against the same IEEE operations
    double e3[4] = {3.0 / 64, 5.0 / 64, 7.0 / 64, 7.0 / 64}, w3[4];
    CHECK(knn_weights(e3, 4, true, 2.0, w3) == 4, "four entries expected");
    const volatile double r1 = e3[0] / e3[1], r2 = e3[0] / e3[2];
    const volatile double S = ((1.0 + r1) + r2) + r2;
    CHECK(w3[0] == 1.0 / S && w3[1] == r1 / S && w3[2] == r2 / S && w3[3] == w3[2], "e == 2: the stated order of operations");
    CHECK(is_rounded_quotient(r1, 3, 5) && is_rounded_quotient(r2, 3, 7), "the quotients themselves");
  }
  // random exact distances, e in {2, 1, 3.5}: the order is kept, every weight in [0, 1], the sum within K eps of 1
  for (int trial = 0; trial < 2000; ++trial) {
    double d[8], w[8];
    const int k = 1 + (int)(rnd() % 8);
    double acc = (1 + rnd() % 64) / 64.0;
    for (int i = 0; i < 8; ++i) {
      d[i] = acc;
      acc += (rnd() % 3 == 0) ? 0.0 : (rnd() % 512) / 64.0;   // equal distances among them
    }
    const double e = trial % 3 == 0 ? 2.0 : trial % 3 == 1 ? 1.0 : 3.5;
    const int got = knn_weights(d, k, true, e, w);
    double sum = 0.0;
    bool ordered = true, inside = true;
    for (int i = 0; i < got; ++i) {
      sum += w[i];
      inside = inside && w[i] >= 0.0 && w[i] <= 1.0;
      if (i > 0) ordered = ordered && w[i] <= w[i - 1] && (d[i] != d[i - 1] || w[i] == w[i - 1]);
    }
    CHECK(got == k && ordered && inside, "trial %d: k = %d, e = %g: got %d entries, ordered %d, inside %d", trial, k, e, got, (int)ordered, (int)inside);
    CHECK(std::fabs(sum - 1.0) <= k * DBL_EPSILON, "trial %d: k = %d, e = %g: the weights sum to 1 %+.3g", trial, k, e, sum - 1.0);
  }
  // a far neighbour underflows to weight 0 and nothing overflows
  {
    double d[2] = {1e-300, 4.0}, w[2];
    CHECK(knn_weights(d, 2, true, 8.0, w) == 2 && w[0] == 1.0 && w[1] == 0.0, "a far neighbour may underflow to 0: %g %g", w[0], w[1]);
  }
  // the entry count a CSR output may have: 2^31 - 2 at most
  CHECK(knn_nnz_fits(0) && knn_nnz_fits(2147483646ll) && !knn_nnz_fits(2147483647ll) && !knn_nnz_fits(1ll << 40) && !knn_nnz_fits(-1),
        "a CSR handle holds at most 2^31 - 2 entries");
  std::printf("weights: checked\n");
}

int main() {
  for (int n : {1, 5, 8, 9, 64, 65, 600}) test_bvh(n);
  const int grids[4][2] = {{5, 3}, {4, 4}, {9, 7}, {33, 17}};
  for (const auto &g : grids) test_pyramid(g[0], g[1]);
  test_weights();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
