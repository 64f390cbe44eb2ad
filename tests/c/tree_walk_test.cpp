// Host run of the Stores' two tree walks (mpassit_amd/csrc/tree_walk.h): the text the kernels compile, on trees built here.
//   walk_filter with a predicate that accepts every box reaches every leaf exactly once, from the root and from untested seeds below
//   it, and its stack stays within WalkCap<>::FILTER;
//   walk_nearest returns the brute-force nearest item, ties to the lowest id, on items with exact duplicates, within WalkCap<>::NEAREST.
// Coordinates are multiples of 1/8 in [0, 4): every squared distance is exact in double, so equal distances are equal bit for bit.
// Exit status 0 and a last line "ok" when everything holds.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../mpassit_amd/csrc/tree_walk.h"

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (unsigned)(rng_state >> 33);
}
static double coord() { return (rnd() % 32) / 8.0; }

struct Pt {
  double x, y, z;
};
static double dist2(const Pt &a, const Pt &b) { return (a.x - b.x) * (a.x - b.x) + (a.y - b.y) * (a.y - b.y) + (a.z - b.z) * (a.z - b.z); }
static double boxdist2(const Pt &p, const double *bx) {
  const double dx = std::max(std::max(bx[0] - p.x, p.x - bx[3]), 0.0), dy = std::max(std::max(bx[1] - p.y, p.y - bx[4]), 0.0),
               dz = std::max(std::max(bx[2] - p.z, p.z - bx[5]), 0.0);
  return dx * dx + dy * dy + dz * dz;
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

// every leaf exactly once, the stack within its bound
template <class Tree>
static void check_filter(const Tree &t, int64_t nleaf, const char *what) {
  std::vector<int> seen((size_t)nleaf, 0);
  int deepest = 0;
  walk_filter(
      t, walk_enc<Tree>(t.top(), 0), true, [](const double *) { return true; },
      [&](int node) {
        ++seen[(size_t)node];
        return false;
      },
      &deepest);
  int64_t bad = 0;
  for (int64_t i = 0; i < nleaf; ++i) bad += seen[(size_t)i] != 1;
  std::printf("%s: %lld leaves, %d levels, filter stack %d of %d\n", what, (long long)nleaf, t.top() + 1, deepest, WalkCap<Tree>::FILTER);
  CHECK(bad == 0, "%s: %lld leaves not visited exactly once", what, (long long)bad);
  CHECK(deepest <= WalkCap<Tree>::FILTER, "%s: filter stack %d above its bound", what, deepest);
  // a leaf that stops the walk is the last one visited
  int visits = 0;
  walk_filter(t, walk_enc<Tree>(t.top(), 0), true, [](const double *) { return true; }, [&](int) { return ++visits == 1; });
  CHECK(visits == 1, "%s: the walk went on after a leaf stopped it", what);
  // entries below the root (seeds that were tested where they were queued): started untested from every node of the level under the
  // root the walks reach every leaf exactly once between them, although the predicate rejects these very nodes; started tested, none
  if (t.top() >= 1) {
    const int lev = t.top() - 1;
    std::vector<int> again((size_t)nleaf, 0);
    int tested = 0;
    for (int k = 0; k < Tree::FAN; ++k) {
      const int c = t.child(t.top(), 0, k);
      if (c < 0) continue;
      const double *own = t.box(lev, c);
      auto not_own = [&](const double *bx) { return bx != own; };
      auto count = [&](int node) {
        ++again[(size_t)node];
        return false;
      };
      walk_filter(t, walk_enc<Tree>(lev, c), false, not_own, count);
      walk_filter(t, walk_enc<Tree>(lev, c), true, not_own, [&](int) { return ++tested < 0; });
    }
    int64_t bad2 = 0;
    for (int64_t i = 0; i < nleaf; ++i) bad2 += again[(size_t)i] != 1;
    CHECK(bad2 == 0, "%s: %lld leaves not visited exactly once from the untested seeds", what, (long long)bad2);
    CHECK(tested == 0, "%s: %d leaves reached through a seed its own test rejects", what, tested);
  }
}

// items(node, f): f(id, point) for every item of leaf `node`
template <class Tree, class Items>
static void check_nearest(const Tree &t, const std::vector<Pt> &pts, const std::vector<int> &ids, Items items, const char *what) {
  int deepest = 0, wrong = 0;
  for (int q = 0; q < 200; ++q) {
    // half of the queries sit exactly on an item, the others half a lattice step off: ties either way
    Pt p = {coord(), coord(), coord()};
    if (q & 1) p.x += 1.0 / 16.0;
    double bd = 1e300;
    int bid = 0x7fffffff;
    for (size_t i = 0; i < pts.size(); ++i) {
      const double d = dist2(p, pts[i]);
      if (d < bd || (d == bd && ids[i] < bid)) {
        bd = d;
        bid = ids[i];
      }
    }
    double best = 1e300;
    int best_id = 0x7fffffff;
    walk_nearest(
        t, [&](const double *bx) { return boxdist2(p, bx); }, best,
        [&](int node) {
          items(node, [&](int id, const Pt &s) {
            const double d = dist2(p, s);
            if (d < best || (d == best && id < best_id)) {
              best = d;
              best_id = id;
            }
          });
          return false;
        },
        &deepest);
    wrong += best_id != bid || best != bd;
  }
  std::printf("%s: nearest stack %d of %d\n", what, deepest, WalkCap<Tree>::NEAREST);
  CHECK(wrong == 0, "%s: %d of 200 nearest answers differ from brute force", what, wrong);
  CHECK(deepest <= WalkCap<Tree>::NEAREST, "%s: nearest stack %d above its bound", what, deepest);
}

// pyramid over lx x ly leaves of MPG_PYR_B0 x MPG_PYR_B0 points (the last row and column of leaves hold one point row / column less)
static void test_pyramid(int lx, int ly) {
  const int npx = lx * MPG_PYR_B0 - (lx > 1), npy = ly * MPG_PYR_B0 - (ly > 1);
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
  CHECK(v.nlev <= MPG_PYR_MAXLEV, "pyramid %d x %d: %d levels", lx, ly, v.nlev);
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
  std::snprintf(what, sizeof what, "pyramid %d x %d", lx, ly);
  const PyrTree t{v};
  CHECK(walk_fits<PyrTree>((int64_t)lx * ly), "%s: leaves do not fit", what);
  check_filter(t, (int64_t)lx * ly, what);
  check_nearest(t, pts, ids,
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
  CHECK(v.nlev <= MPG_BVH_MAXLEV, "bvh %d: %d levels", n, v.nlev);
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
  check_filter(t, v.nnodes[0], what);
  check_nearest(t, sorted, ids,
                [&](int node, auto f) {
                  for (int64_t i = (int64_t)node * MPG_BVH_LEAF; i < std::min<int64_t>(n, ((int64_t)node + 1) * MPG_BVH_LEAF); ++i)
                    f(v.sid[i], sorted[(size_t)i]);
                },
                what);
}

int main() {
  const int pyr[6][2] = {{1, 1}, {4, 4}, {5, 3}, {17, 9}, {129, 65}, {1025, 3}};
  for (const auto &p : pyr) test_pyramid(p[0], p[1]);
  for (int n : {1, 8, 9, 65, 4097}) test_bvh(n);
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
