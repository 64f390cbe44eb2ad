// The bilinear map of a quad of four unit vectors, solved for a point on the sphere: shared by the Grid -> Grid Store
// (k_store_gridbil.hip) and the Grid -> Mesh Store (k_store_to_mesh.hip), which must produce the same weights for the same quad.
// Include it only in translation units that switch floating-point contraction off (#pragma clang fp contract(off) in front of their
// includes): what it computes is then a function of this text, not of which products a compiler chooses to fuse.
#pragma once
#include "geom.h"

// X(xi, eta) = A + (B - A) xi + (D - A) eta + (A - B + C - D) xi eta = lam * P, Newton in 3-D from the quad's middle.
// -> true when the point lies on the quad's side of the origin (lam > 0); xi, eta are not range-checked here.
__device__ inline bool quad_solve(dv3 P, dv3 A, dv3 B, dv3 C, dv3 D, double *xi, double *eta) {
  double s = 0.5, t = 0.5, lam = 1.0;
  dv3 e1 = B - A, e2 = D - A, e3 = (A - B) + (C - D);
  for (int it = 0; it < 50; ++it) {
    dv3 X = (A + e1 * s) + (e2 * t + e3 * (s * t));
    dv3 F = X - P * lam;
    dv3 Js = e1 + e3 * t, Jt = e2 + e3 * s, Jl = P * -1.0;
    double det = dot3(Js, cross3(Jt, Jl));
    if (det == 0.0) return false;
    dv3 mF = F * -1.0;
    double ds = dot3(mF, cross3(Jt, Jl)) / det;
    double dt = dot3(Js, cross3(mF, Jl)) / det;
    double dl = dot3(Js, cross3(Jt, mF)) / det;
    s += ds;
    t += dt;
    lam += dl;
    // Newton converges quadratically: after a step below 1e-9 what is left is ~1e-18, far under the rounding noise of the
    // residual (1e-16 of a unit vector over a cell of 5e-4 rad = 2e-13 in xi / eta).  The former 1e-15 was below that
    // noise and never met: every point ran all 50 iterations (0.74 ms per stagger on configuration 4).
    if (fabs(ds) < 1e-9 && fabs(dt) < 1e-9) break;
  }
  *xi = s;
  *eta = t;
  return lam > 0.0;
}

// One quad of the Grid -> Mesh Stores (k_store_to_mesh.hip, k_store_periodic_to_mesh.hip: the same text, hence the same weights): is P
// inside the quad of corners A, B, C, D?  -> its four weights in corner order.  The quad is solved only when its box holds the point.
__device__ __forceinline__ bool quad_try(dv3 P, dv3 A, dv3 B, dv3 C, dv3 D, double tol, double *ww) {
  const double lox = fmin(fmin(A.x, B.x), fmin(C.x, D.x)), hix = fmax(fmax(A.x, B.x), fmax(C.x, D.x));
  const double loy = fmin(fmin(A.y, B.y), fmin(C.y, D.y)), hiy = fmax(fmax(A.y, B.y), fmax(C.y, D.y));
  const double loz = fmin(fmin(A.z, B.z), fmin(C.z, D.z)), hiz = fmax(fmax(A.z, B.z), fmax(C.z, D.z));
  // the patch lies in the hull of its corners; its image on the sphere bulges out of it by <= d^2 / 2, and a point within tol of the
  // parametric range by <= 2 tol d more (d: the box's diagonal)
  const double d2 = (hix - lox) * (hix - lox) + (hiy - loy) * (hiy - loy) + (hiz - loz) * (hiz - loz);
  const double pad = 0.5 * d2 + 2.0 * tol * sqrt(d2) + 1e-9;
  if (P.x < lox - pad || P.x > hix + pad || P.y < loy - pad || P.y > hiy + pad || P.z < loz - pad || P.z > hiz + pad) return false;
  double xi, eta;
  if (!quad_solve(P, A, B, C, D, &xi, &eta)) return false;
  if (xi < -tol || xi > 1.0 + tol || eta < -tol || eta > 1.0 + tol) return false;
  ww[0] = (1 - xi) * (1 - eta); ww[1] = xi * (1 - eta); ww[2] = xi * eta; ww[3] = (1 - xi) * eta;
  return true;
}
