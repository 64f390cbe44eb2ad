// The search every Store shares: two box trees, two walks, one stack bound.
//
// The trees.  `PyramidView`: the 2 x 2 AABB pyramid over a structured point set (k_setup.hip; level 0 = blocks of MPG_PYR_B0 x MPG_PYR_B0
// points, cells or quads).  `BvhView`: the Morton-sorted 8-ary BVH over a mesh's sites, dual triangles or cell polygons (bvh_build,
// k_store_nearest.hip; leaf = MPG_BVH_LEAF consecutive sorted items).  box[level] is [nodes][6] = lo.xyz, hi.xyz in both.
// The adaptors `PyrTree` / `BvhTree` give the walks what they need of either: the top level, the box of (level, node), the fan-out, the
// k-th child of a node (-1: outside the level), the width of the node number in a stack entry and BATCH, the number of children whose
// boxes walk_filter fetches in one round trip (the pyramid's four; one at a time for the BVH's eight, whose 48 bounds are not worth the
// registers).
// The walks.  `walk_filter`: depth-first over every node whose box passes a test, for "which leaves can hold / meet this figure".
// `walk_nearest`: branch and bound on a lower bound per box, for "which item is nearest".  A kernel keeps its own leaf body.
// The stack.  An entry is level << SHIFT | node.  Both walks go down one level per step, from the top level (<= MAXLEV - 1) to 0:
//   filter      the node to visit next stays in a register and only its passing siblings are stored, <= FAN - 1 per level left behind
//               and MAXLEV - 1 levels to leave: (FAN - 1) (MAXLEV - 1) entries at most;
//   best-first  all passing children are stored and the nearest is popped at once: the same FAN - 1 per level left behind, and one
//               more while the children of the last node are on top: (FAN - 1) (MAXLEV - 1) + 1.
// The arrays below have exactly these sizes, so no walk checks its stack at run time and none can drop a node.
// Plain C++ without HIP intrinsics: tests/c/tree_walk_test.cpp runs the same text on the host.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define TW_FN __host__ __device__ __forceinline__
#else
#define TW_FN inline
#endif

#define MPG_PYR_B0 4
#define MPG_PYR_MAXLEV 16
struct PyramidView {  // passed by value to kernels
  int nlev;
  int nx[MPG_PYR_MAXLEV], ny[MPG_PYR_MAXLEV];
  int64_t off[MPG_PYR_MAXLEV + 1];  // node offset of each level inside `box` (in nodes)
  const double *box;
};

#define MPG_BVH_LEAF 8
#define MPG_BVH_FAN 8
#define MPG_BVH_MAXLEV 12
struct BvhView {  // passed by value to kernels
  int64_t n;           // items sorted
  const int32_t *sid;  // original id of each sorted item
  int nlev;
  int64_t nnodes[MPG_BVH_MAXLEV];
  int64_t off[MPG_BVH_MAXLEV + 1];
  const double *box;
};

struct PyrTree {
  static constexpr int FAN = 4, MAXLEV = MPG_PYR_MAXLEV, SHIFT = 26, BATCH = 4;
  const PyramidView &v;
  TW_FN int top() const { return v.nlev - 1; }
  TW_FN const double *box(int lev, int node) const { return v.box + 6 * (v.off[lev] + node); }
  TW_FN int child(int lev, int node, int k) const {
    const int nxl = v.nx[lev], cnx = v.nx[lev - 1], cny = v.ny[lev - 1];
    const int ci = 2 * (node % nxl) + (k & 1), cj = 2 * (node / nxl) + (k >> 1);
    return ((ci < cnx) & (cj < cny)) ? cj * cnx + ci : -1;   // (& for &&: the level's sizes are fetched together, ahead of the division)
  }
};
struct BvhTree {
  static constexpr int FAN = MPG_BVH_FAN, MAXLEV = MPG_BVH_MAXLEV, SHIFT = 27, BATCH = 1;
  const BvhView &v;
  TW_FN int top() const { return v.nlev - 1; }
  TW_FN const double *box(int lev, int64_t node) const { return v.box + 6 * (v.off[lev] + node); }
  TW_FN int child(int lev, int node, int k) const {
    const int64_t c = (int64_t)node * FAN + k;
    return c < v.nnodes[lev - 1] ? (int)c : -1;
  }
};
// a level of `leaves` nodes fits a stack entry (the host checks it once per Store: mpg_walk_check, mpg_internal.h)
template <class Tree>
TW_FN bool walk_fits(int64_t leaves) { return leaves < ((int64_t)1 << Tree::SHIFT); }
template <class Tree>
TW_FN int walk_enc(int lev, int node) { return (lev << Tree::SHIFT) | node; }

template <class Tree>
struct WalkCap {
  static constexpr int FILTER = (Tree::FAN - 1) * (Tree::MAXLEV - 1), NEAREST = FILTER + 1;
  static_assert(Tree::MAXLEV <= (1 << (31 - Tree::SHIFT)), "the level does not fit above the node number");
};
static_assert(WalkCap<PyrTree>::FILTER == 45 && WalkCap<PyrTree>::NEAREST == 46 && WalkCap<BvhTree>::FILTER == 77 && WalkCap<BvhTree>::NEAREST == 78,
              "stack sizes follow from the fan-out and the levels (see the head of this file)");

// Depth-first over the nodes whose box `accept(box)` passes, from the entry `start` (tested first if test_start); leaf(node) is called for
// every level-0 node reached and ends the walk by returning true.  Children are taken in the order k = 0 .. FAN - 1, BATCH at a time: all
// of a batch are tested BEFORE any is kept, so that their bounds are fetched together and the walk makes one iteration per node that
// passes, not one dependent pop + box load per child.  deepest: the most entries the stack held (the host test reads it).
template <class Tree, class Accept, class Leaf>
TW_FN void walk_filter(const Tree &t, int start, bool test_start, Accept accept, Leaf leaf, int *deepest = nullptr) {
  constexpr int MASK = (1 << Tree::SHIFT) - 1;
  int stack[WalkCap<Tree>::FILTER];
  int sp = 0;
  int cur = (!test_start || accept(t.box(start >> Tree::SHIFT, start & MASK))) ? start : -1;
  for (;;) {
    if (cur < 0) {
      if (sp == 0) break;
      cur = stack[--sp];
    }
    const int e = cur;
    cur = -1;
    const int lev = e >> Tree::SHIFT, node = e & MASK;
    if (lev == 0) {
      if (leaf(node)) return;
      continue;
    }
#pragma unroll 1
    for (int k0 = 0; k0 < Tree::FAN; k0 += Tree::BATCH) {
      int c[Tree::BATCH];
      bool go[Tree::BATCH];
#pragma unroll
      for (int k = 0; k < Tree::BATCH; ++k) {
        c[k] = t.child(lev, node, k0 + k);
        go[k] = c[k] >= 0 && accept(t.box(lev - 1, c[k]));
      }
#pragma unroll
      for (int k = 0; k < Tree::BATCH; ++k)
        if (go[k]) {
          if (cur < 0) cur = walk_enc<Tree>(lev - 1, c[k]);
          else stack[sp++] = walk_enc<Tree>(lev - 1, c[k]);
        }
    }
    if (deepest && sp > *deepest) *deepest = sp;
  }
}

// Branch and bound: bound(box) is a lower bound of what leaf(node) can bring `best` down to.  A node is opened unless its bound is
// strictly above `best` -- equal bounds are explored: a tie with a lower id may hide inside -- and its children are stored by descending
// bound, so that the nearest is popped first.  leaf(node) updates `best` and ends the walk by returning true.
template <class Tree, class Bound, class Leaf>
TW_FN void walk_nearest(const Tree &t, Bound bound, double &best, Leaf leaf, int *deepest = nullptr) {
  constexpr int MASK = (1 << Tree::SHIFT) - 1;
  int stack[WalkCap<Tree>::NEAREST];
  int sp = 0;
  stack[sp++] = walk_enc<Tree>(t.top(), 0);
  while (sp > 0) {
    const int e = stack[--sp];
    const int lev = e >> Tree::SHIFT, node = e & MASK;
    if (bound(t.box(lev, node)) > best) continue;
    if (lev == 0) {
      if (leaf(node)) return;
      continue;
    }
    double cd[Tree::FAN];
    int cc[Tree::FAN];
    int nc = 0;
    for (int k = 0; k < Tree::FAN; ++k) {
      const int c = t.child(lev, node, k);
      if (c < 0) continue;
      const double d = bound(t.box(lev - 1, c));
      if (d > best) continue;
      int i = nc++;
      while (i > 0 && cd[i - 1] < d) {
        cd[i] = cd[i - 1];
        cc[i] = cc[i - 1];
        --i;
      }
      cd[i] = d;
      cc[i] = c;
    }
    for (int i = 0; i < nc; ++i) stack[sp++] = walk_enc<Tree>(lev - 1, cc[i]);
    if (deepest && sp > *deepest) *deepest = sp;
  }
}
