// A box tree seen through a mask over its items (mpg_handle_extrapolate_masked, k_extrapolate.hip): the walks of tree_walk.h never enter a
// subtree that holds no unmasked item.
//
// Why.  walk_nearest prunes on bound > best, and knn_search keeps best at INFINITY until its K-list is full.  A leaf body that merely
// skips masked items therefore opens EVERY node while fewer than K unmasked items have been met: with few unmasked items, or unmasked
// items far from the query, each query walks the whole tree.  The cure is structural, not a tighter bound: one byte per tree node,
//   alive[off[0] + leaf]  = the leaf holds at least one unmasked item        (alive_leaves: the caller's leaf test)
//   alive[off[l] + node]  = any child of the node is alive, l > 0            (alive_parent, one level after the other, bottom-up)
// and `AliveTree`, an adaptor whose child() answers -1 for a dead node, which both walks already read as "no such child".  The root is
// dead exactly when every item is masked: the caller skips the search then (alive_root).  The boxes stay those of ALL items -- valid lower
// bounds for any subset -- so the result is exact; the topology, the stack entries and the stack bounds (WalkCap) are those of the tree
// underneath.  Leaf bodies test mask[id] before they compute a distance.
// Plain C++ without HIP intrinsics, as tree_walk.h: the kernels and tests/c/knn_mask_test.cpp compile this same text.
#pragma once
#include <stdint.h>

#include "knn.h"
#include "tree_walk.h"

TW_FN int64_t alive_level_nodes(const PyrTree &t, int lev) { return (int64_t)t.v.nx[lev] * t.v.ny[lev]; }
TW_FN int64_t alive_level_nodes(const BvhTree &t, int lev) { return t.v.nnodes[lev]; }
template <class Tree>
TW_FN int64_t alive_total_nodes(const Tree &t) { return t.v.off[t.top()] + alive_level_nodes(t, t.top()); }

// one node of level lev > 0 from the level below
template <class Tree>
TW_FN uint8_t alive_parent(const Tree &t, int lev, int node, const uint8_t *alive) {
  uint8_t a = 0;
  for (int k = 0; k < Tree::FAN; ++k) {
    const int c = t.child(lev, node, k);
    if (c >= 0) a |= alive[t.v.off[lev - 1] + c];
  }
  return a != 0;
}

template <class Tree>
TW_FN bool alive_root(const Tree &t, const uint8_t *alive) { return alive[t.v.off[t.top()]] != 0; }

// the host form of the pass: leaf_alive(leaf) = "leaf holds an unmasked item"; alive has alive_total_nodes(t) bytes
template <class Tree, class LeafAlive>
inline void alive_build_host(const Tree &t, LeafAlive leaf_alive, uint8_t *alive) {
  const int64_t leaves = alive_level_nodes(t, 0);
  for (int64_t n = 0; n < leaves; ++n) alive[t.v.off[0] + n] = leaf_alive((int)n) ? 1 : 0;
  for (int lev = 1; lev <= t.top(); ++lev) {
    const int64_t nn = alive_level_nodes(t, lev);
    for (int64_t n = 0; n < nn; ++n) alive[t.v.off[lev] + n] = alive_parent(t, lev, (int)n, alive);
  }
}

template <class Tree>
struct AliveTree {
  static constexpr int FAN = Tree::FAN, MAXLEV = Tree::MAXLEV, SHIFT = Tree::SHIFT, BATCH = Tree::BATCH;
  const Tree t;
  const uint8_t *alive;
  TW_FN int top() const { return t.top(); }
  TW_FN const double *box(int lev, int node) const { return t.box(lev, node); }
  TW_FN int child(int lev, int node, int k) const {
    const int c = t.child(lev, node, k);
    return (c >= 0 && alive[t.v.off[lev - 1] + c]) ? c : -1;
  }
};
// knn_search (knn.h) over the unmasked items: `items` hands over the unmasked items of a leaf only.  A dead root -- every item masked -- is
// no search at all: the list comes back empty and no leaf body runs (the root of a one-leaf tree is that leaf).
template <class Tree, int K, class Bound, class Items>
TW_FN void knn_search_masked(const Tree &t, const uint8_t *alive, Bound bound, Items items, KBest<K> &list, int *deepest = nullptr) {
  list.clear();
  if (!alive_root(t, alive)) return;
  knn_search(AliveTree<Tree>{t, alive}, bound, items, list, deepest);
}

static_assert(WalkCap<AliveTree<PyrTree>>::NEAREST == WalkCap<PyrTree>::NEAREST && WalkCap<AliveTree<BvhTree>>::NEAREST == WalkCap<BvhTree>::NEAREST,
              "the adaptor changes neither the fan-out nor the levels: the stack bounds are those of the tree underneath");
