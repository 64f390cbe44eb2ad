// Host run of the masked K-nearest search (mpassit_amd/csrc/knn_mask.h over knn.h and tree_walk.h) and of mpg_handle_mask's row rule
// (mpassit_amd/csrc/handle_mask.h): the text the kernels compile, on trees built here.
//   For every tree, every mask and K in {1, 2, 3, 4, 8}: knn_search_masked returns the K smallest (d2, id) pairs of a brute-force sort over
//   the UNMASKED items, n == min(K, unmasked); the leaf body is never called for a leaf without an unmasked item (the calls are counted);
//   an all-masked tree makes no leaf call at all; the stack stays within WalkCap<>::NEAREST; a constructed tie picks the higher id exactly
//   when the lower one is masked.
//   hm_entry_row equals rational arithmetic on exact inputs under both norms, empties a row whose kept sum is <= 0, and returns a row with
//   nothing masked bit for bit.
// Coordinates are multiples of 1/8 in [0, 4): every squared distance is exact in double, so equal distances are equal bit for bit.
// Exit status 0 and a last line "ok" when everything holds.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../mpassit_amd/csrc/handle_mask.h"
#include "../../mpassit_amd/csrc/knn_mask.h"

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
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

// A tree with its items: pos[id] = the item's point, leaf_of[id] = its leaf, items_of(leaf) = the ids a leaf body visits, in its order
template <class Tree>
struct Case {
  const Tree &t;
  std::vector<Pt> pos;
  std::vector<int> leaf_of;
  std::vector<std::vector<int>> leaf_items;
  std::string what;
};

static long long leaf_calls = 0, dead_leaf_calls = 0;

template <int K, class Tree>
static void check_knn(const Case<Tree> &c, const std::vector<uint8_t> &mask, const std::vector<uint8_t> &alive, const char *mname, int *deepest) {
  const int n = (int)c.pos.size();
  int unmasked = 0;
  for (int i = 0; i < n; ++i) unmasked += !mask[(size_t)i];
  const int want = std::min(unmasked, K);
  int wrong = 0;
  for (int q = 0; q < 60; ++q) {
    Pt p = {coord(), coord(), coord()};
    if (q % 3 == 0) p = c.pos[(size_t)(rnd() % (unsigned)n)];   // a copy of an item (masked or not)
    if (q % 3 == 2) p.x += 1.0 / 16.0;
    std::vector<std::pair<double, int>> all;
    for (int i = 0; i < n; ++i)
      if (!mask[(size_t)i]) all.push_back({dist2(p, c.pos[(size_t)i]), i});
    std::sort(all.begin(), all.end());
    KBest<K> best;
    knn_search_masked(
        c.t, alive.data(), [&](const double *bx) { return boxdist2(p, bx); },
        [&](int node, auto f) {
          ++leaf_calls;
          bool any = false;
          for (int id : c.leaf_items[(size_t)node]) {
            if (mask[(size_t)id]) continue;   // the mask first, as the kernels' leaf bodies
            any = true;
            f(dist2(p, c.pos[(size_t)id]), (int32_t)id);
          }
          dead_leaf_calls += !any;
        },
        best, deepest);
    bool bad = best.n != want;
    for (int k = 0; k < K; ++k) {
      if (k < want) bad = bad || best.d2[k] != all[(size_t)k].first || best.id[k] != all[(size_t)k].second;
      else bad = bad || best.d2[k] != INFINITY || best.id[k] != 0x7fffffff;
    }
    wrong += bad;
  }
  CHECK(wrong == 0, "%s, mask %s, K = %d: %d of 60 lists differ from the brute-force sort over the unmasked items", c.what.c_str(), mname, K, wrong);
}

template <class Tree>
static void check_masks(const Case<Tree> &c) {
  const int n = (int)c.pos.size();
  const int nleaf = (int)c.leaf_items.size();
  struct M {
    const char *name;
    std::vector<uint8_t> m;
  };
  std::vector<M> masks;
  masks.push_back({"none", std::vector<uint8_t>((size_t)n, 0)});
  masks.push_back({"all", std::vector<uint8_t>((size_t)n, 1)});
  {
    std::vector<uint8_t> m((size_t)n, 1);
    m[(size_t)(rnd() % (unsigned)n)] = 0;
    masks.push_back({"all but one", m});
    std::vector<uint8_t> m3((size_t)n, 1);   // all but three (all but n where the tree has fewer)
    for (int left = std::min(n, 3); left > 0;) {
      const size_t i = (size_t)(rnd() % (unsigned)n);
      if (m3[i]) {
        m3[i] = 0;
        --left;
      }
    }
    masks.push_back({"all but three", m3});
  }
  {
    std::vector<uint8_t> m((size_t)n, 0);   // one whole leaf: 8 sorted sites, or a 4 x 4 block
    for (int id : c.leaf_items[(size_t)(nleaf / 2)]) m[(size_t)id] = 1;
    masks.push_back({"one leaf", m});
  }
  {
    std::vector<uint8_t> m((size_t)n, 0);   // every item of one half-space
    for (int i = 0; i < n; ++i) m[(size_t)i] = c.pos[(size_t)i].x < 2.0;
    masks.push_back({"half-space", m});
  }
  {
    std::vector<uint8_t> m((size_t)n, 0);
    for (int i = 0; i < n; ++i) m[(size_t)i] = rnd() % 3 == 0;
    masks.push_back({"random third", m});
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
    bool any = false, bytes = true;
    for (int i = 0; i < n; ++i) any = any || !mk.m[(size_t)i];
    for (uint8_t a : alive) bytes = bytes && a <= 1;
    CHECK(bytes, "%s, mask %s: every node has its alive byte", c.what.c_str(), mk.name);
    CHECK(alive_root(c.t, alive.data()) == any, "%s, mask %s: the root is alive exactly when an item is unmasked", c.what.c_str(), mk.name);
    const long long calls0 = leaf_calls;
    check_knn<1>(c, mk.m, alive, mk.name, &deepest);
    check_knn<2>(c, mk.m, alive, mk.name, &deepest);
    check_knn<3>(c, mk.m, alive, mk.name, &deepest);
    check_knn<4>(c, mk.m, alive, mk.name, &deepest);
    check_knn<8>(c, mk.m, alive, mk.name, &deepest);
    if (!any) CHECK(leaf_calls == calls0, "%s: an all-masked tree made %lld leaf calls", c.what.c_str(), leaf_calls - calls0);
    else CHECK(leaf_calls > calls0, "%s, mask %s: no leaf call at all", c.what.c_str(), mk.name);
  }
  std::printf("%s: knn stack %d of %d\n", c.what.c_str(), deepest, WalkCap<AliveTree<Tree>>::NEAREST);
  CHECK(deepest <= WalkCap<AliveTree<Tree>>::NEAREST, "%s: knn stack %d above its bound", c.what.c_str(), deepest);
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
  Case<PyrTree> c{t, pts, std::vector<int>(pts.size()), std::vector<std::vector<int>>((size_t)lx * ly), ""};
  for (int j = 0; j < npy; ++j)
    for (int i = 0; i < npx; ++i) {
      const Pt &p = pts[(size_t)j * npx + i];
      const double b[6] = {p.x, p.y, p.z, p.x, p.y, p.z};
      const int leaf = (j / MPG_PYR_B0) * lx + i / MPG_PYR_B0;
      box_add(&box[6 * (size_t)leaf], b);
      c.leaf_of[(size_t)j * npx + i] = leaf;
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
  check_masks(c);
}

struct BvhCase {
  BvhView v;
  std::vector<int32_t> sid;
  std::vector<double> box;
};
// BVH over the points `pts` (id = position in pts) sorted by a space-filling key of the lattice
static void build_bvh(const std::vector<Pt> &pts, BvhCase &b, std::vector<int> &leaf_of, std::vector<std::vector<int>> &leaf_items) {
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
  leaf_of.assign((size_t)n, 0);
  leaf_items.assign((size_t)b.v.nnodes[0], std::vector<int>());
  for (int i = 0; i < n; ++i) {
    const Pt &p = pts[(size_t)order[(size_t)i]];
    const double c[6] = {p.x, p.y, p.z, p.x, p.y, p.z};
    box_add(&b.box[6 * (size_t)(i / MPG_BVH_LEAF)], c);
    leaf_of[(size_t)order[(size_t)i]] = i / MPG_BVH_LEAF;
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
  std::vector<int> leaf_of;
  std::vector<std::vector<int>> leaf_items;
  build_bvh(pts, b, leaf_of, leaf_items);
  const BvhTree t{b.v};
  char what[64];
  std::snprintf(what, sizeof what, "bvh %d", n);
  Case<BvhTree> c{t, pts, leaf_of, leaf_items, what};
  check_masks(c);
}

// Two items at the same distance from the query, far apart in the tree: the lower id wins unless it is masked, then the higher one does
static void test_tie() {
  std::vector<Pt> pts(40);
  for (size_t i = 0; i < pts.size(); ++i) pts[i] = Pt{3.0 + (rnd() % 8) / 8.0, 3.0 + (rnd() % 8) / 8.0, 3.0 + (rnd() % 8) / 8.0};
  const Pt q = {1.0, 1.0, 1.0};
  pts[5] = Pt{0.5, 1.0, 1.0};    // d2 = 1/4
  pts[31] = Pt{1.0, 1.5, 1.0};   // d2 = 1/4: a tie with id 5
  BvhCase b;
  std::vector<int> leaf_of;
  std::vector<std::vector<int>> leaf_items;
  build_bvh(pts, b, leaf_of, leaf_items);
  const BvhTree t{b.v};
  for (int masked_low = 0; masked_low < 2; ++masked_low) {
    std::vector<uint8_t> mask(pts.size(), 0);
    mask[5] = (uint8_t)masked_low;
    std::vector<uint8_t> alive((size_t)alive_total_nodes(t));
    alive_build_host(
        t,
        [&](int leaf) {
          for (int id : leaf_items[(size_t)leaf])
            if (!mask[(size_t)id]) return true;
          return false;
        },
        alive.data());
    KBest<2> best;
    knn_search_masked(
        t, alive.data(), [&](const double *bx) { return boxdist2(q, bx); },
        [&](int node, auto f) {
          for (int id : leaf_items[(size_t)node])
            if (!mask[(size_t)id]) f(dist2(q, pts[(size_t)id]), (int32_t)id);
        },
        best);
    CHECK(best.d2[0] == 0.25 && best.id[0] == (masked_low ? 31 : 5), "tie, lower id %s: rank 0 is id %d", masked_low ? "masked" : "unmasked", best.id[0]);
    if (!masked_low) CHECK(best.d2[1] == 0.25 && best.id[1] == 31, "tie: rank 1 is id %d", best.id[1]);
    else CHECK(best.id[1] != 5 && best.d2[1] > 0.25, "tie, lower id masked: the masked item must not appear");
  }
  std::printf("tie: checked\n");
}

// w == the double nearest to num / den (positive integers): |w - num / den| <= ulp(w) / 2, in integers
static bool is_rounded_quotient(double w, long long num, long long den) {
  int ex;
  const double m = std::frexp(w, &ex);
  const long long M = (long long)std::ldexp(m, 53);
  const int s = 53 - ex;
  if (s < 0 || s > 70) return false;
  const __int128 diff = (__int128)M * den - ((__int128)num << s);
  const __int128 a = diff < 0 ? -diff : diff;
  return 2 * a <= den;
}

static void test_row_rule() {
  // values k / 64: every partial sum is exact, so Wk is the rational sum and w / Wk the rounded quotient of two integers
  const int32_t col[6] = {4, 0, 7, 2, 9, 5};
  const long long num[6] = {3, 5, 7, 11, 13, 2};
  double val[6];
  for (int q = 0; q < 6; ++q) val[q] = num[q] / 64.0;
  uint8_t mask[10] = {0, 0, 1, 0, 0, 0, 0, 1, 0, 0};   // columns 2 and 7 masked: entries 2 and 3 go
  const long long kept_sum = 3 + 5 + 13 + 2;
  const int kept_at[4] = {0, 1, 4, 5};
  for (int norm = 0; norm < 2; ++norm) {
    int32_t oc[6];
    double ov[6], f = -1.0, f0 = -1.0;
    const int len0 = hm_entry_row(col, val, 6, mask, norm, 0.75, nullptr, nullptr, &f0);
    const int len = hm_entry_row(col, val, 6, mask, norm, 0.75, oc, ov, &f);
    CHECK(len == 4 && len0 == 4 && f == f0, "norm %d: the length pass and the fill pass agree (%d, %d)", norm, len0, len);
    for (int k = 0; k < 4; ++k) {
      CHECK(oc[k] == col[kept_at[k]], "norm %d: kept entries stay in stored order", norm);
      if (norm == HM_NORM_DSTAREA) CHECK(ov[k] == val[kept_at[k]], "DSTAREA: values unchanged");
      else CHECK(is_rounded_quotient(ov[k], num[kept_at[k]], kept_sum), "FRACAREA: w'[%d] = %.17g is not %lld / %lld rounded", k, ov[k], num[kept_at[k]], kept_sum);
    }
    if (norm == HM_NORM_DSTAREA) CHECK(f == kept_sum / 64.0, "DSTAREA: frac' = Wk");
    else CHECK(f == 0.75 * (kept_sum / 64.0), "FRACAREA: frac' = frac * Wk (exact here)");
    // nothing masked: bit for bit, frac included (a NaN payload and a negative zero among the values)
    double odd[3] = {-0.0, std::nan("7"), 0.1}, oo[3];
    const int32_t oc3[3] = {1, 3, 4};
    int32_t occ[3];
    double ff = 0.0;
    const double fin = 0.1 + 0.2;
    CHECK(hm_entry_row(oc3, odd, 3, mask, norm, fin, occ, oo, &ff) == 3 && std::memcmp(oo, odd, sizeof odd) == 0 && std::memcmp(occ, oc3, sizeof oc3) == 0 &&
              std::memcmp(&ff, &fin, sizeof fin) == 0,
          "norm %d: a row with nothing masked comes back bit for bit", norm);
    CHECK(hm_entry_row(oc3, odd, 3, nullptr, norm, fin, occ, oo, &ff) == 3 && std::memcmp(oo, odd, sizeof odd) == 0, "norm %d: no mask at all", norm);
    // Wk <= 0: kept values that cancel, a negative kept sum, and nothing kept
    const int32_t c2[3] = {2, 0, 1};
    const double cancel[3] = {0.5, 0.25, -0.25}, neg[3] = {0.5, -0.5, 0.25}, any[3] = {0.5, 0.25, 0.25};
    uint8_t all[3] = {1, 1, 1};
    ff = 9.0;
    CHECK(hm_entry_row(c2, cancel, 3, mask, norm, 0.5, occ, oo, &ff) == 0 && ff == 0.0 && !std::signbit(ff), "norm %d: Wk == 0 empties the row, frac' = +0.0", norm);
    ff = 9.0;
    CHECK(hm_entry_row(c2, neg, 3, mask, norm, 0.5, occ, oo, &ff) == 0 && ff == 0.0 && !std::signbit(ff), "norm %d: Wk < 0 empties the row", norm);
    ff = 9.0;
    CHECK(hm_entry_row(c2, any, 3, all, norm, 0.5, occ, oo, &ff) == 0 && ff == 0.0 && !std::signbit(ff), "norm %d: nothing kept empties the row", norm);
    ff = 9.0;
    CHECK(hm_entry_row(c2, any, 0, mask, norm, 0.5, occ, oo, &ff) == 0 && ff == 0.5, "norm %d: an empty row stays as it is", norm);
  }
  std::printf("row rule: checked\n");
}

int main() {
  for (int n : {1, 5, 8, 9, 64, 65, 600}) test_bvh(n);
  const int grids[4][2] = {{5, 3}, {4, 4}, {9, 7}, {33, 17}};
  for (const auto &g : grids) test_pyramid(g[0], g[1]);
  test_tie();
  test_row_rule();
  std::printf("leaf calls %lld, of them on leaves without an unmasked item %lld\n", leaf_calls, dead_leaf_calls);
  CHECK(dead_leaf_calls == 0, "the leaf body ran %lld times on a leaf without an unmasked item", dead_leaf_calls);
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
