// Creep-fill extrapolation (mpg_handle_creep, k_creep.hip): the arithmetic of include/mpassit_amd.h's creep section, one text for device and host.
//
// A destination point p has neighbours Nb(p), ascending and without p: on a grid stagger of snx x sny points the points of
// [i - 1, i + 1] x [j - 1, j + 1] inside the grid (no shift, no wrap: cr_neighbours_grid), on a mesh's cells N1(p) of patch.h minus p
// (PtSrc::ring1 itself, not a copy).  cr_joins: the level predicate -- an unassigned point takes level L iff a neighbour holds level L - 1.
// cr_sum_div: the value of one column, acc = acc + v from 0.0 over its terms in candidate order, then acc / (double)m.  cr_merge_row: the
// ordered merge-and-divide of a whole row from its candidates in (contributor, stored) order -- pt_row_add's merge, then the division --
// which is what the device's sort-and-sum passes must equal bit for bit (tests/c/creep_test.cpp holds the two against each other).
// Every operation is rounded on its own: include it AFTER `#pragma clang fp contract(off)` (k_creep.hip), or build with -ffp-contract=off
// (tests/c/creep_test.cpp).  Only + and /.  Plain C++ without HIP intrinsics, as patch.h and knn.h.
#pragma once
#include "patch.h"

#define CR_MAX_NB PT_MAX_PNTS   // ids an Nb(p) buffer holds: 8 on a grid, at most 2 * maxEdges <= 24 on a mesh with maxEdges <= 12
#define CR_MAX_EDGES 12         // the widest verticesOnCell row whose ring fits: 1 + 2 * 12 = 25 <= PT_MAX_PNTS
enum { CR_UNASSIGNED = -1, CR_SKIPPED = -2 };   // level[p] of an unmapped row: still to be reached / dst_skip: never filled, never a neighbour

// Nb(p) on a grid stagger into ids [8] -> its size
PT_FN int cr_neighbours_grid(int snx, int sny, int32_t p, int32_t *ids) {
  const int i = p % snx, j = p / snx;
  int n = 0;
  for (int b = j - 1; b <= j + 1; ++b) {
    if (b < 0 || b >= sny) continue;
    for (int a = i - 1; a <= i + 1; ++a) {
      if (a < 0 || a >= snx || (a == i && b == j)) continue;
      ids[n++] = b * snx + a;
    }
  }
  return n;
}

// Nb(p) of the destination set d (a mesh's cells, or a grid stagger: only voc, tri, maxEdges, nV, snx, sny are read) into ids
// [CR_MAX_NB] -> its size.  A ring beyond PT_MAX_PNTS points has no neighbours here: the entry point refuses maxEdges > CR_MAX_EDGES,
// below which it cannot happen
PT_FN int cr_neighbours(const PtSrc &d, int32_t p, int32_t *ids) {
  if (!d.mesh()) return cr_neighbours_grid(d.snx, d.sny, p, ids);
  const int n1 = d.ring1(p, ids);
  if (n1 > PT_MAX_PNTS) return 0;
  int n = 0;
  for (int k = 0; k < n1; ++k)
    if (ids[k] != p) ids[n++] = ids[k];
  return n;
}

// the level predicate: does a point with neighbours nb [n] join level L?
PT_FN bool cr_joins(const int32_t *level, const int32_t *nb, int n, int L) {
  for (int k = 0; k < n; ++k)
    if (level[nb[k]] == L - 1) return true;
  return false;
}

// the value of one column: its n terms term(0), term(1), ... in candidate order, summed from 0.0, divided by the m contributors
template <class Term>
PT_FN double cr_sum_div(int64_t n, Term term, int m) {
  double acc = 0.0;
  for (int64_t k = 0; k < n; ++k) acc = acc + term(k);
  return acc / (double)m;
}

// a whole row from its candidates (ccol, cval) [nc] in (contributor, stored) order: the ascending distinct columns into col / val [cap],
// every value summed in candidate order from 0.0 and divided by m -> the row's length, -1 when it would hold more than cap entries
PT_FN int cr_merge_row(const int32_t *ccol, const double *cval, int64_t nc, int m, int32_t *col, double *val, int cap) {
  int n = 0;
  for (int64_t k = 0; k < nc; ++k)
    if (!pt_row_add(col, val, n, cap, ccol[k], cval[k])) return -1;
  for (int k = 0; k < n; ++k) val[k] = val[k] / (double)m;
  return n;
}
