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
