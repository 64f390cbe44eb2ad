// The four ways the wind kernels combine a point's two regridded components a, b with its two per-point numbers (c, s) -- k_wind_pair.hip
// on two fixed handles, k_wind_csr.hip on two CSR handles; the table of what each policy computes stands at the head of k_wind_pair.hip.
// Both translation units set `#pragma clang fp contract(off)` in front of this header: every product and sum below is rounded.
#pragma once

struct CellsRotated {
  static constexpr int NOUT = 2;
  static constexpr bool ANGLES = true;
  static __device__ __forceinline__ void combine(double ra, double rb, double c, double s, double &o0, double &o1) {
    const double t1 = ra * c, t2 = rb * s, t3 = ra * s, t4 = rb * c;
    o0 = t1 - t2;
    o1 = t3 + t4;
  }
};
struct CellsPlain {
  static constexpr int NOUT = 2;
  static constexpr bool ANGLES = false;
  static __device__ __forceinline__ void combine(double ra, double rb, double, double, double &o0, double &o1) {
    o0 = ra;
    o1 = rb;
  }
};
struct EdgesNormal {
  static constexpr int NOUT = 1;
  static constexpr bool ANGLES = true;
  static __device__ __forceinline__ void combine(double ra, double rb, double c, double s, double &o0, double &o1) {
    const double t1 = ra * c, t2 = rb * s;
    o0 = t1 + t2;
    o1 = 0.0;   // (not stored)
  }
};
struct EdgesBoth {
  static constexpr int NOUT = 2;
  static constexpr bool ANGLES = true;
  static __device__ __forceinline__ void combine(double ra, double rb, double c, double s, double &o0, double &o1) {
    const double t1 = ra * c, t2 = rb * s;
    o0 = t1 + t2;
    const double t3 = rb * c, t4 = ra * s;
    o1 = t3 - t4;
  }
};
