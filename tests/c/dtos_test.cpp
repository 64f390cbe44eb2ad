// Host run of the nearest-destination-to-source search and its value rule (mpassit_amd/csrc/dtos.h over knn.h, knn_mask.h and tree_walk.h):
// the text the kernels of k_store_dtos.hip compile, on trees built here.
//   For every tree and every mask (none, all items masked, all but one): dtos_nearest / dtos_nearest_masked return the brute-force minimum of
//   (d2, id) over the unmasked items, -1 when none is left; queries are random lattice points, copies of an item, and points equidistant
//   from two items (the midpoint of two items, whose two squared distances are equal bit for bit on this lattice); the walk's stack stays
//   within WalkCap<>::NEAREST.  A constructed tie far apart in the tree goes to the lower id, to the higher one when the lower is masked.
//   dtos_value gives 1.0 under the sum rule and the rounded quotient 1 / n under the mean rule for n = 1 .. 600.
// Coordinates are multiples of 1/8 in [0, 4): every squared distance is exact in double, so equal distances are equal bit for bit.
// Exit status 0 and a last line "ok" when everything holds.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../../mpassit_amd/csrc/dtos.h"

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

// the destination set as a tree with its items: pos[id] = the item's point, leaf_items[leaf] = the ids a leaf body visits, in its order
template <class Tree>
struct Case {
  const Tree &t;
  std::vector<Pt> pos;
  std::vector<std::vector<int>> leaf_items;
  std::string what;
};

static int brute(const std::vector<Pt> &pos, const std::vector<uint8_t> &mask, const Pt &q) {
  int best = -1;
  double bd = 0.0;
  for (int i = 0; i < (int)pos.size(); ++i) {
    if (mask[(size_t)i]) continue;
    const double d = dist2(q, pos[(size_t)i]);
    if (best < 0 || d < bd) {   // (ascending id: an equal distance keeps the lower id)
      best = i;
      bd = d;
    }
  }
  return best;
}

template <class Tree>
static int search(const Case<Tree> &c, const std::vector<uint8_t> *mask, const std::vector<uint8_t> *alive, const Pt &q, int *deepest) {
  auto bound = [&](const double *bx) { return boxdist2(q, bx); };
  if (!mask)
    return dtos_nearest(
        c.t, bound,
        [&](int node, auto f) {
          for (int id : c.leaf_items[(size_t)node]) f(dist2(q, c.pos[(size_t)id]), (int32_t)id);
        },
        deepest);
  return dtos_nearest_masked(
      c.t, alive->data(), bound,
      [&](int node, auto f) {
        for (int id : c.leaf_items[(size_t)node])
          if (!(*mask)[(size_t)id]) f(dist2(q, c.pos[(size_t)id]), (int32_t)id);   // the mask first, as the kernels' leaf bodies
      },
      deepest);
}

static long long ties_met = 0;

template <class Tree>
static void check_case(const Case<Tree> &c) {
  const int n = (int)c.pos.size();
  struct M {
    const char *name;
    bool use;
    std::vector<uint8_t> m;
  };
  std::vector<M> masks;
  masks.push_back({"no mask", false, std::vector<uint8_t>((size_t)n, 0)});
  masks.push_back({"all alive", true, std::vector<uint8_t>((size_t)n, 0)});
  masks.push_back({"none alive", true, std::vector<uint8_t>((size_t)n, 1)});
  {
    std::vector<uint8_t> m((size_t)n, 1);
    m[(size_t)(rnd() % (unsigned)n)] = 0;
    masks.push_back({"one alive", true, m});
    std::vector<uint8_t> r((size_t)n, 0);
    for (int i = 0; i < n; ++i) r[(size_t)i] = rnd() % 3 == 0;
    masks.push_back({"random third", true, r});
  }
  int deepest = 0;
  for (const M &mk : masks) {
    std::vector<uint8_t> alive((size_t)alive_total_nodes(c.t), 2);
    alive_build_host(
        c.t,
        [&](int leaf) {
          for (int id : c.leaf_items[(size_t)leaf])
            if (!mk.m[(size_t)id]) return true;
          return false;
        },
        alive.data());
    int wrong = 0;
    for (int q = 0; q < 90; ++q) {
      Pt p = {coord(), coord(), coord()};
      if (q % 3 == 0) p = c.pos[(size_t)(rnd() % (unsigned)n)];   // a copy of an item (masked or not)
      if (q % 3 == 2) {                                          // equidistant from two items: their midpoint (sixteenths: still exact)
        const Pt &a = c.pos[(size_t)(rnd() % (unsigned)n)], &b = c.pos[(size_t)(rnd() % (unsigned)n)];
        p = Pt{0.5 * (a.x + b.x), 0.5 * (a.y + b.y), 0.5 * (a.z + b.z)};
        ties_met += dist2(p, a) == dist2(p, b);
      }
      const int want = brute(c.pos, mk.m, p);
      const int got = search(c, mk.use ? &mk.m : nullptr, &alive, p, &deepest);
      wrong += got != want;
    }
    CHECK(wrong == 0, "%s, %s: %d of 90 answers differ from the brute-force (d2, id) minimum", c.what.c_str(), mk.name, wrong);
  }
  std::printf("%s: dtos stack %d of %d\n", c.what.c_str(), deepest, WalkCap<Tree>::NEAREST);
  CHECK(deepest <= WalkCap<Tree>::NEAREST, "%s: stack %d above its bound", c.what.c_str(), deepest);
}

// the point pyramid of npx x npy points: leaves of MPG_PYR_B0 x MPG_PYR_B0 points, the last row / column of leaves ragged
static void test_pyramid(int npx, int npy) {
  const int lx = (npx + MPG_PYR_B0 - 1) / MPG_PYR_B0, ly = (npy + MPG_PYR_B0 - 1) / MPG_PYR_B0;
  std::vector<Pt> pts((size_t)npx * npy);
  for (size_t i = 0; i < pts.size(); ++i) pts[i] = (i % 7 == 3) ? pts[i - 3] : Pt{coord(), coord(), coord()};   // exact duplicates of earlier points
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
  const PyrTree t{v};
  Case<PyrTree> c{t, pts, std::vector<std::vector<int>>((size_t)lx * ly), ""};
  for (int j = 0; j < npy; ++j)
    for (int i = 0; i < npx; ++i) {
      const Pt &p = pts[(size_t)j * npx + i];
      const double b[6] = {p.x, p.y, p.z, p.x, p.y, p.z};
      const int leaf = (j / MPG_PYR_B0) * lx + i / MPG_PYR_B0;
      box_add(&box[6 * (size_t)leaf], b);
      c.leaf_items[(size_t)leaf].push_back(j * npx + i);   // (row by row inside the block: the kernels' order)
    }
  for (int l = 1; l < v.nlev; ++l)
    for (int j = 0; j < v.ny[l - 1]; ++j)
      for (int i = 0; i < v.nx[l - 1]; ++i)
        box_add(&box[6 * (v.off[l] + (int64_t)(j / 2) * v.nx[l] + i / 2)], &box[6 * (v.off[l - 1] + (int64_t)j * v.nx[l - 1] + i)]);
  v.box = box.data();
  char what[64];
  std::snprintf(what, sizeof what, "grid %d x %d", npx, npy);
  c.what = what;
  check_case(c);
}

struct BvhCase {
  BvhView v;
  std::vector<int32_t> sid;
  std::vector<double> box;
};
// BVH over the points `pts` (id = position in pts) sorted by a space-filling key of the lattice
static void build_bvh(const std::vector<Pt> &pts, BvhCase &b, std::vector<std::vector<int>> &leaf_items) {
  const int n = (int)pts.size();
  std::vector<int> order((size_t)n);
  for (int i = 0; i < n; ++i) order[(size_t)i] = i;
  auto key = [&](int i) { return ((int)(pts[(size_t)i].x) * 4 + (int)(pts[(size_t)i].y)) * 4 + (int)(pts[(size_t)i].z); };
  std::stable_sort(order.begin(), order.end(), [&](int a, int c) { return key(a) < key(c); });
  b.sid.assign(order.begin(), order.end());
  b.v.n = n;
  b.v.sid = b.sid.data();
  b.v.nlev = 0;
  int64_t total = 0;
  for (int64_t cnt = (n + MPG_BVH_LEAF - 1) / MPG_BVH_LEAF;; cnt = (cnt + MPG_BVH_FAN - 1) / MPG_BVH_FAN) {
    b.v.nnodes[b.v.nlev] = cnt;
    b.v.off[b.v.nlev++] = total;
    total += cnt;
    if (cnt == 1) break;
  }
  b.v.off[b.v.nlev] = total;
  b.box.assign(6 * (size_t)total, 0.0);
  for (int64_t k = 0; k < total; ++k) box_empty(&b.box[6 * k]);
  leaf_items.assign((size_t)b.v.nnodes[0], std::vector<int>());
  for (int i = 0; i < n; ++i) {
    const Pt &p = pts[(size_t)order[(size_t)i]];
    const double c[6] = {p.x, p.y, p.z, p.x, p.y, p.z};
    box_add(&b.box[6 * (size_t)(i / MPG_BVH_LEAF)], c);
    leaf_items[(size_t)(i / MPG_BVH_LEAF)].push_back(order[(size_t)i]);
  }
  for (int l = 1; l < b.v.nlev; ++l)
    for (int64_t c = 0; c < b.v.nnodes[l - 1]; ++c) box_add(&b.box[6 * (b.v.off[l] + c / MPG_BVH_FAN)], &b.box[6 * (b.v.off[l - 1] + c)]);
  b.v.box = b.box.data();
}

static void test_bvh(int n) {
  std::vector<Pt> pts((size_t)n);
  for (int i = 0; i < n; ++i) pts[(size_t)i] = (i % 5 == 4) ? pts[(size_t)i - 2] : Pt{coord(), coord(), coord()};   // exact duplicates
  BvhCase b;
  std::vector<std::vector<int>> leaf_items;
  build_bvh(pts, b, leaf_items);
  const BvhTree t{b.v};
  char what[64];
  std::snprintf(what, sizeof what, "bvh %d", n);
  Case<BvhTree> c{t, pts, leaf_items, what};
  check_case(c);
}

// Two items at the same distance from the query, far apart in the tree: the lower id wins unless it is masked, then the higher one does
static void test_tie() {
  std::vector<Pt> pts(40);
  for (size_t i = 0; i < pts.size(); ++i) pts[i] = Pt{3.0 + (rnd() % 8) / 8.0, 3.0 + (rnd() % 8) / 8.0, 3.0 + (rnd() % 8) / 8.0};
  const Pt q = {1.0, 1.0, 1.0};
  pts[5] = Pt{0.5, 1.0, 1.0};    // d2 = 1/4
  pts[31] = Pt{1.0, 1.5, 1.0};   // d2 = 1/4: a tie with id 5
  BvhCase b;
  std::vector<std::vector<int>> leaf_items;
  build_bvh(pts, b, leaf_items);
  const BvhTree t{b.v};
  Case<BvhTree> c{t, pts, leaf_items, "tie"};
  std::vector<uint8_t> none(pts.size(), 0), low(pts.size(), 0), alive((size_t)alive_total_nodes(t));
  low[5] = 1;
  CHECK(search(c, nullptr, nullptr, q, nullptr) == 5, "tie, no mask: the lower id");
  for (int masked_low = 0; masked_low < 2; ++masked_low) {
    const std::vector<uint8_t> &mask = masked_low ? low : none;
    alive_build_host(
        t,
        [&](int leaf) {
          for (int id : leaf_items[(size_t)leaf])
            if (!mask[(size_t)id]) return true;
          return false;
        },
        alive.data());
    const int got = search(c, &mask, &alive, q, nullptr);
    CHECK(got == (masked_low ? 31 : 5), "tie, lower id %s: id %d", masked_low ? "masked" : "unmasked", got);
  }
  std::printf("tie: checked\n");
}

// w == the double nearest to 1 / den: |w * den - 1| <= ulp(w) * den / 2, in integers
static bool is_rounded_reciprocal(double w, long long den) {
  int ex;
  const double m = std::frexp(w, &ex);
  const long long M = (long long)std::ldexp(m, 53);
  const int s = 53 - ex;
  if (s < 0 || s > 70) return false;
  const __int128 diff = (__int128)M * den - ((__int128)1 << s);
  const __int128 a = diff < 0 ? -diff : diff;
  return 2 * a <= den;
}

static void test_values() {
  int bad = 0;
  for (int n = 1; n <= 600; ++n) {
    const double w = dtos_value(DTOS_MEAN, n);
    bad += !(w == 1.0 / (double)n && is_rounded_reciprocal(w, n));
    bad += dtos_value(DTOS_SUM, n) != 1.0;
  }
  CHECK(bad == 0, "the value rule: %d of 1200 values differ from 1.0 / the rounded 1 / n", bad);
  CHECK(dtos_value(DTOS_MEAN, 1) == 1.0 && dtos_value(DTOS_MEAN, 4) == 0.25, "the mean of one entry is 1, of four 1/4");
  std::printf("values: checked\n");
}

int main() {
  for (int n : {1, 8, 9, 65, 600}) test_bvh(n);
  const int grids[3][2] = {{4, 4}, {5, 3}, {33, 17}};
  for (const auto &g : grids) test_pyramid(g[0], g[1]);
  test_tie();
  test_values();
  std::printf("equidistant queries met: %lld\n", ties_met);
  CHECK(ties_met > 100, "the midpoint queries must be equidistant from their two items");
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
