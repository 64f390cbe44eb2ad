// Patch regridding (mpg_handle_patch, k_patch.hip): the arithmetic of include/mpassit_amd.h's patch section, one text for device and host.
//
// A source node c has a ring-1 patch N1(c) -- on a mesh c and the cells of the valid dual triangles of its listed vertices, on a grid
// stagger the 3 x 3 window about it shifted into the grid -- and, on a mesh, a ring-2 patch N2(c) = the union of N1(d) over d in N1(c);
// both ascending, both used only when they hold at most PT_MAX_PNTS points (PtSrc::ring1 / ring2 return PT_MAX_PNTS + 1 beyond that).
// pt_frame: the orthographic frame about c.  pt_fit<M>: h, G = sum phi phi^T in patch order, and the thresholded Cholesky G = R^T R in
// place (M = 6: degree 2, M = 3: degree 1); every index is a compile-time constant, so G / R live in registers.  pt_attempt: the ladder
// A (degree 2 on N1), B (degree 2 on N2), C (degree 1 on N1), D (the node itself) -- a property of the node alone.  pt_slot: the shape
// values L_k of one (destination point, slot) pair under the node's attempt, handed to emit(id, L) in patch order.  pt_set_add /
// pt_row_add: the ordered merge of up to PT_MAX_SLOTS * PT_MAX_PNTS candidates into the ascending distinct columns of a row, the values
// summed in (slot, patch position) order from 0.0.
// Every operation is rounded on its own: include it AFTER `#pragma clang fp contract(off)` (k_patch.hip), or build with -ffp-contract=off
// (tests/c/patch_test.cpp).  Only + - * / sqrt.  Plain C++ without HIP intrinsics, as knn.h.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define PT_FN __host__ __device__ __forceinline__
#define PT_UNROLL _Pragma("unroll")
#else
#define PT_FN inline
#define PT_UNROLL
#endif

#define PT_MAX_PNTS 32    // MPG_PATCH_MAX_PNTS of include/mpassit_amd.h
#define PT_MAX_SLOTS 4    // slots per row of a fixed bilinear handle (3 or 4)
#define PT_PIVOT_TOL 0x1p-26   // a pivot passes when s_k > 2^-26 * G_kk: a definition, not a tuning constant
enum { PT_ATT_A = 0, PT_ATT_B = 1, PT_ATT_C = 2, PT_ATT_D = 3 };

PT_FN double pt_dot(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// ids[0 .. n) ascending and distinct: id joins it.  false: it would be entry cap + 1 (nothing is written)
PT_FN bool pt_set_add(int32_t *ids, int &n, int cap, int32_t id) {
  int k = n;
  while (k > 0 && ids[k - 1] > id) --k;
  if (k > 0 && ids[k - 1] == id) return true;
  if (n >= cap) return false;
  for (int j = n; j > k; --j) ids[j] = ids[j - 1];
  ids[k] = id;
  ++n;
  return true;
}

// the same with a value per column: a new column starts from 0.0 + term, a known one takes val = val + term
PT_FN bool pt_row_add(int32_t *col, double *val, int &n, int cap, int32_t id, double term) {
  int k = n;
  while (k > 0 && col[k - 1] > id) --k;
  if (k > 0 && col[k - 1] == id) {
    val[k - 1] = val[k - 1] + term;
    return true;
  }
  if (n >= cap) return false;
  for (int j = n; j > k; --j) {
    col[j] = col[j - 1];
    val[j] = val[j - 1];
  }
  col[k] = id;
  val[k] = 0.0 + term;
  ++n;
  return true;
}

// the source point set: the cells of a whole mesh (voc [nCells][maxEdges] 1-based and 0-padded, tri [3][nV] with -1 = none) or the
// snx x sny points of a grid stagger, and their stored unit vectors
struct PtSrc {
  const double *x, *y, *z;
  const int32_t *voc, *tri;   // nullptr: a grid stagger
  int maxEdges;
  int64_t nV;
  int snx, sny;
  PT_FN bool mesh() const { return voc != nullptr; }
  PT_FN void xyz(int32_t id, double *q) const { q[0] = x[id]; q[1] = y[id]; q[2] = z[id]; }
  // d and the cells of the valid dual triangles of d's listed vertices join ids
  PT_FN bool add_cell(int32_t d, int32_t *ids, int &n) const {
    if (!pt_set_add(ids, n, PT_MAX_PNTS, d)) return false;
    for (int e = 0; e < maxEdges; ++e) {
      const int64_t v = (int64_t)voc[(int64_t)d * maxEdges + e] - 1;
      if (v < 0 || v >= nV) continue;
      const int32_t a = tri[v], b = tri[nV + v], c = tri[2 * nV + v];
      if (a < 0 || b < 0 || c < 0) continue;
      if (!pt_set_add(ids, n, PT_MAX_PNTS, a) || !pt_set_add(ids, n, PT_MAX_PNTS, b) || !pt_set_add(ids, n, PT_MAX_PNTS, c)) return false;
    }
    return true;
  }
  // N1(c) into ids [PT_MAX_PNTS] -> its size, PT_MAX_PNTS + 1 when it holds more
  PT_FN int ring1(int32_t c, int32_t *ids) const {
    int n = 0;
    if (mesh()) return add_cell(c, ids, n) ? n : PT_MAX_PNTS + 1;
    const int i = c % snx, j = c / snx;
    const int ih = snx - 3 > 0 ? snx - 3 : 0, jh = sny - 3 > 0 ? sny - 3 : 0;
    const int i0 = i - 1 < 0 ? 0 : i - 1 > ih ? ih : i - 1, j0 = j - 1 < 0 ? 0 : j - 1 > jh ? jh : j - 1;
    const int i1 = i0 + 2 < snx - 1 ? i0 + 2 : snx - 1, j1 = j0 + 2 < sny - 1 ? j0 + 2 : sny - 1;
    for (int b = j0; b <= j1; ++b)
      for (int a = i0; a <= i1; ++a) ids[n++] = b * snx + a;
    return n;
  }
  // N2(c) from N1(c) = n1 [c1] (c1 <= PT_MAX_PNTS), meshes only -> its size, PT_MAX_PNTS + 1 when it holds more
  PT_FN int ring2(const int32_t *n1, int c1, int32_t *ids) const {
    int n = 0;
    for (int k = 0; k < c1; ++k)
      if (!add_cell(n1[k], ids, n)) return PT_MAX_PNTS + 1;
    return n;
  }
};

// e1, e2 of the frame about the unit vector X: a = the axis of X's smallest |component| (the lowest on ties), t = a - (a . X) X,
// e1 = t / sqrt(t . t), e2 = X x e1
PT_FN void pt_frame(const double *X, double *e1, double *e2) {
  int ax = 0;
  if (fabs(X[1]) < fabs(X[ax])) ax = 1;
  if (fabs(X[2]) < fabs(X[ax])) ax = 2;
  double a[3] = {0.0, 0.0, 0.0};
  if (ax == 0) a[0] = 1.0;
  if (ax == 1) a[1] = 1.0;
  if (ax == 2) a[2] = 1.0;
  const double s = pt_dot(a, X);
  double t[3];
  PT_UNROLL
  for (int k = 0; k < 3; ++k) t[k] = a[k] - s * X[k];
  const double r = sqrt(pt_dot(t, t));
  PT_UNROLL
  for (int k = 0; k < 3; ++k) e1[k] = t[k] / r;
  e2[0] = X[1] * e1[2] - X[2] * e1[1];
  e2[1] = X[2] * e1[0] - X[0] * e1[2];
  e2[2] = X[0] * e1[1] - X[1] * e1[0];
}

template <int M>
struct PtFit {
  double X[3], e1[3], e2[3], h;
  double R[M][M];   // the upper triangle: G while it is summed, R of G = R^T R after the factorisation
};

template <int M>
PT_FN void pt_phi(double u, double v, double *phi) {
  phi[0] = 1.0;
  phi[1] = u;
  phi[2] = v;
  if constexpr (M > 3) {
    phi[3] = u * u;
    phi[4] = u * v;
    phi[5] = v * v;
  }
}

template <int M>
PT_FN void pt_uv(const PtFit<M> &f, const double *q, double &u, double &v) {
  const double d[3] = {q[0] - f.X[0], q[1] - f.X[1], q[2] - f.X[2]};
  u = pt_dot(d, f.e1) / f.h;
  v = pt_dot(d, f.e2) / f.h;
}

// the fit of node c on the patch ids [n]: frame, h, G, Cholesky.  false: h is not > 0, or a pivot is not > 2^-26 G_kk
template <int M>
PT_FN bool pt_fit(const PtSrc &s, const int32_t *ids, int n, int32_t c, PtFit<M> &f) {
  s.xyz(c, f.X);
  pt_frame(f.X, f.e1, f.e2);
  double hm = 0.0;
  for (int k = 0; k < n; ++k) {
    double q[3];
    s.xyz(ids[k], q);
    const double d[3] = {q[0] - f.X[0], q[1] - f.X[1], q[2] - f.X[2]};
    const double dd = pt_dot(d, d);
    hm = dd > hm ? dd : hm;
  }
  f.h = sqrt(hm);
  if (!(f.h > 0.0)) return false;
  PT_UNROLL
  for (int a = 0; a < M; ++a) {
    PT_UNROLL
    for (int b = 0; b < M; ++b) f.R[a][b] = 0.0;
  }
  for (int k = 0; k < n; ++k) {
    double q[3], u, v, phi[M];
    s.xyz(ids[k], q);
    pt_uv(f, q, u, v);
    pt_phi<M>(u, v, phi);
    PT_UNROLL
    for (int a = 0; a < M; ++a) {
      PT_UNROLL
      for (int b = a; b < M; ++b) f.R[a][b] = f.R[a][b] + phi[a] * phi[b];
    }
  }
  bool pass = true;
  PT_UNROLL
  for (int k = 0; k < M; ++k) {
    const double g = f.R[k][k];
    double p = g;
    PT_UNROLL
    for (int i = 0; i < k; ++i) p = p - f.R[i][k] * f.R[i][k];
    if (!(p > PT_PIVOT_TOL * g)) pass = false;
    const double r = sqrt(p);
    f.R[k][k] = r;
    PT_UNROLL
    for (int j = k + 1; j < M; ++j) {
      double t = f.R[k][j];
      PT_UNROLL
      for (int i = 0; i < k; ++i) t = t - f.R[i][k] * f.R[i][j];
      f.R[k][j] = t / r;
    }
  }
  return pass;
}

// the shape values of the fit at the point P: R^T z = phi(P), R y = z, L_k = sum_a phi_a(q_k) y_a from 0.0 -> emit(ids[k], L_k)
template <int M, class Emit>
PT_FN void pt_shape(const PtSrc &s, const PtFit<M> &f, const int32_t *ids, int n, const double *P, Emit emit) {
  double u, v, y[M];
  pt_uv(f, P, u, v);
  pt_phi<M>(u, v, y);
  PT_UNROLL
  for (int k = 0; k < M; ++k) {   // z in place
    double t = y[k];
    PT_UNROLL
    for (int i = 0; i < k; ++i) t = t - f.R[i][k] * y[i];
    y[k] = t / f.R[k][k];
  }
  PT_UNROLL
  for (int k = M - 1; k >= 0; --k) {   // y in place
    double t = y[k];
    PT_UNROLL
    for (int j = k + 1; j < M; ++j) t = t - f.R[k][j] * y[j];
    y[k] = t / f.R[k][k];
  }
  for (int k = 0; k < n; ++k) {
    double q[3], phi[M];
    s.xyz(ids[k], q);
    pt_uv(f, q, u, v);
    pt_phi<M>(u, v, phi);
    double L = 0.0;
    PT_UNROLL
    for (int a = 0; a < M; ++a) L = L + phi[a] * y[a];
    emit(ids[k], L);
  }
}

// the attempt that serves node c: A, B, C or D.  ids, tmp: PT_MAX_PNTS ints each
PT_FN int pt_attempt(const PtSrc &s, int32_t c, int32_t *ids, int32_t *tmp) {
  const int n1 = s.ring1(c, tmp);
  if (n1 > PT_MAX_PNTS) return PT_ATT_D;
  if (n1 >= 6) {
    PtFit<6> f;
    if (pt_fit<6>(s, tmp, n1, c, f)) return PT_ATT_A;
  }
  if (s.mesh()) {
    const int n2 = s.ring2(tmp, n1, ids);
    if (n2 >= 6 && n2 <= PT_MAX_PNTS) {
      PtFit<6> f;
      if (pt_fit<6>(s, ids, n2, c, f)) return PT_ATT_B;
    }
  }
  if (n1 >= 3) {
    PtFit<3> f;
    if (pt_fit<3>(s, tmp, n1, c, f)) return PT_ATT_C;
  }
  return PT_ATT_D;
}

// the patch node c is served from under attempt att, into ids -> its size
PT_FN int pt_slot_ids(const PtSrc &s, int32_t c, int att, int32_t *ids, int32_t *tmp) {
  if (att == PT_ATT_D) {
    ids[0] = c;
    return 1;
  }
  int n;
  if (att == PT_ATT_B) {
    const int n1 = s.ring1(c, tmp);
    n = s.ring2(tmp, n1 < PT_MAX_PNTS ? n1 : PT_MAX_PNTS, ids);
  } else {
    n = s.ring1(c, ids);
  }
  return n < PT_MAX_PNTS ? n : PT_MAX_PNTS;   // (A, B and C are only ever recorded for patches that fit)
}

// the shape values of node c's patch at the point P under attempt att -> emit(id, L) in patch order
template <class Emit>
PT_FN void pt_slot(const PtSrc &s, int32_t c, int att, const double *P, int32_t *ids, int32_t *tmp, Emit emit) {
  const int n = pt_slot_ids(s, c, att, ids, tmp);
  if (att == PT_ATT_D) {
    emit(c, 1.0);
  } else if (att == PT_ATT_C) {
    PtFit<3> f;
    (void)pt_fit<3>(s, ids, n, c, f);
    pt_shape<3>(s, f, ids, n, P, emit);
  } else {
    PtFit<6> f;
    (void)pt_fit<6>(s, ids, n, c, f);
    pt_shape<6>(s, f, ids, n, P, emit);
  }
}
