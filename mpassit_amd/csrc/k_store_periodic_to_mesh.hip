// Grid -> Mesh bilinear weight generation from a grid that is periodic in i and closed by pole caps (MPG_GRID_PERIODIC_I): a global
// lat-lon analysis taken onto MPAS cells.  ESMF_FieldRegridStore(srcField on a 1PeriDim / MONOPOLE Grid's CENTER stagger, dstField on
// a Mesh location, regridmethod=BILINEAR, polemethod=).
//
// Sources are the nx x ny CENTER points (source index j * nx + i), destinations the mesh's cell centres or vertices.
//   quads  b in [0, ny - 2], a in [0, nx - 1]: A = (b, a), B = (b, (a + 1) mod nx), C = (b + 1, (a + 1) mod nx), D = (b + 1, a), quad id
//          b * nx + a.  A point belongs to the LOWEST quad id for which quad_try (quad_solve.h: the per-quad code of k_store_to_mesh.hip)
//          passes; the weights of a quad with a < nx - 1 are therefore the bits mpg_regrid_store_to_mesh produces for the same coordinates.
//   caps   only for points no quad took, under MPG_POLEMETHOD_ALLAVG: one fan of nx triangles per end row, A = (row, a), B = (row, (a + 1)
//          mod nx) and the pole that row closes on -- (0, 0, sign of the row's mean z), so the pole node sits where the end row's own
//          points say, not where the row number says (ESMF's MONOPOLE cap): rows numbered south to north have the south pole at row 0,
//          rows numbered north to south (GRIB, the Gaussian grids) the north pole.  Counter-clockwise seen from outside: tri_weights(P, A,
//          B, (0, 0, 1)) at the north pole, tri_weights(P, B, A, (0, 0, -1)) at the south pole (the triangles of k_grid_bilinear,
//          k_store_gridbil.hip), MPG_TOL whatever the inside-tolerance knob says.  Cap ids 0 .. nx - 1 on row 0, nx .. 2 nx - 1 on row
//          ny - 1, the lowest passing id wins.  The two signs are found once per grid on the host (mpg_k_grid_end_poles); two live ends on the
//          same pole are refused.
//          The pole's value is the mean of its CENTER row: the row has nx entries, each wr = t_pole / nx, columns A and B t_A + wr, t_B + wr.
// The handle is an ordinary CSR one with no pole terms: quad rows of exactly 4 entries (zeros included) sorted by column, cap rows of
// exactly nx in column order, empty rows for points nothing mapped.
// Quad candidates come by one of two routes that test the same quads with the same code, so the handles are identical bit for bit:
//   index space  on a lat-lon grid with its projection attached the point's own (i, j) names the quads within mpg_box_pad, a taken
//                mod nx; a NaN index (the lat-lon inverse hands none out poleward of MPG_LATLON_BOX_LIMIT) sends the point to the walk
//   walk         a depth-first walk of an AABB pyramid over the nx x (ny - 1) quads, the seam column included (g->wrappyr)
// Cap candidates are found the same way on both routes: the points without a quad are compacted into a list (count, scan, fill) and a
// wavefront per listed point tests the nx triangles of each live end, lanes over a.  No O(nx) work is done for a point a quad mapped.
// No atomic decides a stored byte (the atomics below count for mpg_handle_store_stats only).
// No floating-point contraction in this translation unit (see k_store_conserve.hip).
#pragma clang fp contract(off)
#include <math.h>

#include <vector>

#include "geom.h"
#include "mpg_internal.h"
#include "quad_solve.h"

#define PTM_CAP_NONE 0x7fffffff

// quad (a, b) of the periodic CENTER stagger, column a + 1 wrapped
__device__ __forceinline__ bool ptm_try_quad(dv3 P, int a, int b, int nx, const double *__restrict__ sx, const double *__restrict__ sy,
                                             const double *__restrict__ sz, double tol, double *ww) {
  const int64_t r0 = (int64_t)b * nx, r1 = r0 + nx;
  const int a1 = a + 1 == nx ? 0 : a + 1;
  return quad_try(P, ld3(sx, sy, sz, r0 + a), ld3(sx, sy, sz, r0 + a1), ld3(sx, sy, sz, r1 + a1), ld3(sx, sy, sz, r1 + a), tol, ww);
}

// qid[p]: the point's quad id, -1 where no quad passed; wq [4][n]: its weights in corner order A, B, C, D (0 where none).
// ij: the points' (i, j) in the grid's 0-based CENTER index space or nullptr.  cnt[0] += points that had an index space and still took the walk.
__global__ __launch_bounds__(256) void k_ptm_quads(int64_t n, const double *__restrict__ px, const double *__restrict__ py,
                                                   const double *__restrict__ pz, int nx, int ny, const double *__restrict__ sx,
                                                   const double *__restrict__ sy, const double *__restrict__ sz, const float *__restrict__ ij,
                                                   float pad_coef, float pad_latlon, PyramidView pyr, double tol, int32_t *__restrict__ qid,
                                                   double *__restrict__ wq, unsigned long long *__restrict__ cnt) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p >= n) return;
  const dv3 P = dv3{px[p], py[p], pz[p]};
  const int qny = ny - 1;
  double ww[4] = {0, 0, 0, 0};
  int best = 0x7fffffff;
  bool placed = false;
  if (ij) {
    const float fi = ij[2 * p], fj = ij[2 * p + 1];
    if (fi == fi && fj == fj) {
      placed = true;
      const float pad = mpg_box_pad(1.f, pad_coef, pad_latlon, fabs(P.z));
      const float lim_i = 2.f * (float)nx + 2.f, lim_j = (float)ny + 2.f;
      const int i0 = (int)floorf(fminf(fmaxf(fi - pad, -lim_i), lim_i)), i1 = (int)floorf(fminf(fmaxf(fi + pad, -lim_i), lim_i));
      const int na = min(i1 - i0 + 1, nx);   // a box as wide as the circle names every column once
      const int a_first = ((i0 % nx) + nx) % nx;
      const int b0 = max((int)floorf(fminf(fmaxf(fj - pad, -2.f), lim_j)), 0), b1 = min((int)floorf(fminf(fmaxf(fj + pad, -2.f), lim_j)), qny - 1);
      for (int b = b0; b <= b1 && best == 0x7fffffff; ++b) {   // ascending rows; within a row the wrapped columns are compared by id
        int a = a_first;
        for (int k = 0; k < na; ++k) {
          const int q = b * nx + a;
          double tw[4];
          if (q < best && ptm_try_quad(P, a, b, nx, sx, sy, sz, tol, tw)) {
            best = q;
#pragma unroll
            for (int c = 0; c < 4; ++c) ww[c] = tw[c];
          }
          a = a + 1 == nx ? 0 : a + 1;
        }
      }
    } else {
      atomicAdd(cnt, 1ull);
    }
  }
  if (!placed) {
    // walk_filter (tree_walk.h) over the wrap-aware pyramid; the margin covers a point within tol outside a quad the node's pad was not
    // built for
    const double mg = 2.0 * tol;
    const PyrTree tree{pyr};
    walk_filter(
        tree, walk_enc<PyrTree>(tree.top(), 0), true,
        [&](const double *bx) {
          return !(P.x < bx[0] - mg || P.x > bx[3] + mg || P.y < bx[1] - mg || P.y > bx[4] + mg || P.z < bx[2] - mg || P.z > bx[5] + mg);
        },
        [&](int node) {
          const int bi = node % pyr.nx[0], bj = node / pyr.nx[0];
          const int a1 = min(bi * MPG_PYR_B0 + MPG_PYR_B0, nx), b1 = min(bj * MPG_PYR_B0 + MPG_PYR_B0, qny);
          for (int b = bj * MPG_PYR_B0; b < b1; ++b)
            for (int a = bi * MPG_PYR_B0; a < a1; ++a) {
              const int q = b * nx + a;
              if (q >= best) continue;
              double tw[4];
              if (ptm_try_quad(P, a, b, nx, sx, sy, sz, tol, tw)) {
                best = q;
#pragma unroll
                for (int c = 0; c < 4; ++c) ww[c] = tw[c];
              }
            }
          return false;
        });
  }
  qid[p] = best == 0x7fffffff ? -1 : best;
#pragma unroll
  for (int c = 0; c < 4; ++c) wq[c * n + p] = ww[c];
}

// miss[p] = 1 where no quad took the point (p < n), miss[n] = 0: the scan's last entry is the list's length
__global__ __launch_bounds__(256) void k_ptm_miss(int64_t n, const int32_t *__restrict__ qid, int32_t *__restrict__ miss) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p <= n) miss[p] = p < n && qid[p] < 0;
}
__global__ __launch_bounds__(256) void k_ptm_list(int64_t n, const int32_t *__restrict__ qid, const int32_t *__restrict__ moff,
                                                  int32_t *__restrict__ list) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p < n && qid[p] < 0) list[moff[p]] = (int32_t)p;
}

// One wavefront per listed point, lanes over the cap ids (row 0: 0 .. nx - 1, row ny - 1: nx .. 2 nx - 1) in steps of 64: every lane keeps
// the first -- its lowest -- passing id, the wavefront takes the minimum.  A point in a cap: qid = -2 - cap id, wq[0 .. 2] = t_A, t_B, t_pole.
// pole0 / pole1: the z (+1 or -1) of the pole row 0 / row ny - 1 closes on.
__global__ __launch_bounds__(256) void k_ptm_caps(int nlist, const int32_t *__restrict__ list, int64_t n, const double *__restrict__ px,
                                                  const double *__restrict__ py, const double *__restrict__ pz, int nx, int ny, int flags,
                                                  double pole0, double pole1, const double *__restrict__ sx, const double *__restrict__ sy,
                                                  const double *__restrict__ sz, int32_t *__restrict__ qid, double *__restrict__ wq) {
  const int lane = threadIdx.x & (MPG_WAVE - 1);
  const int k = (int)((blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / MPG_WAVE);
  if (k >= nlist) return;   // (the whole wavefront)
  const int64_t p = list[k];
  const dv3 P = dv3{px[p], py[p], pz[p]};
  const bool first = !(flags & MPG_GRID_NO_SOUTH_POLE), last = !(flags & MPG_GRID_NO_NORTH_POLE);   // the row-0 end, the row-(ny - 1) end
  int mine = PTM_CAP_NONE;
  double tA = 0.0, tB = 0.0, tP = 0.0;
  for (int id = (first ? 0 : nx) + lane; id < (last ? 2 * nx : nx); id += MPG_WAVE) {
    const bool is_last = id >= nx;
    const int a = is_last ? id - nx : id, a1 = a + 1 == nx ? 0 : a + 1;
    const int64_t row0 = is_last ? (int64_t)(ny - 1) * nx : 0;
    const double pole = is_last ? pole1 : pole0;
    const bool is_north = pole > 0.0;
    const dv3 A = ld3(sx, sy, sz, row0 + a), B = ld3(sx, sy, sz, row0 + a1);
    double t[3];
    // counter-clockwise seen from outside: (A, B, N) at the north pole, (B, A, S) at the south pole
    const bool in = is_north ? tri_weights(P, A, B, dv3{0.0, 0.0, pole}, MPG_TOL, t) : tri_weights(P, B, A, dv3{0.0, 0.0, pole}, MPG_TOL, t);
    if (in) {
      mine = id;
      tA = is_north ? t[0] : t[1];
      tB = is_north ? t[1] : t[0];
      tP = t[2];
      break;
    }
  }
  int lowest = mine;
  for (int o = MPG_WAVE / 2; o > 0; o >>= 1) lowest = min(lowest, __shfl_xor(lowest, o));
  if (lowest != PTM_CAP_NONE && mine == lowest) {   // ids are distinct across lanes: exactly one lane
    qid[p] = -2 - lowest;
    wq[p] = tA;
    wq[n + p] = tB;
    wq[2 * n + p] = tP;
  }
}

// len[p]: 4 for a quad row, nx for a cap row, 0 for an unmapped point (len[n] = 0: the scan's last entry is nnz).
// cnt[1] += cap rows, cnt[2] += seam-quad rows (a = nx - 1): mpg_handle_store_stats [3] and [4]
__global__ __launch_bounds__(256) void k_ptm_rowlen(int64_t n, int nx, const int32_t *__restrict__ qid, int32_t *__restrict__ len,
                                                    unsigned long long *__restrict__ cnt) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p > n) return;
  if (p == n) {
    len[p] = 0;
    return;
  }
  const int q = qid[p];
  len[p] = q >= 0 ? 4 : q <= -2 ? nx : 0;
  if (q <= -2) atomicAdd(cnt + 1, 1ull);
  else if (q >= 0 && q % nx == nx - 1) atomicAdd(cnt + 2, 1ull);
}

__device__ __forceinline__ void ptm_cswap(int32_t &ca, double &wa, int32_t &cb, double &wb) {
  if (cb < ca) {
    const int32_t c = ca; ca = cb; cb = c;
    const double w = wa; wa = wb; wb = w;
  }
}
// quad rows: the four entries in ascending column order (a fixed five-comparator network), their weights moved with them
__global__ __launch_bounds__(256) void k_ptm_fill_quads(int64_t n, int nx, const int32_t *__restrict__ qid, const double *__restrict__ wq,
                                                        const int32_t *__restrict__ rowptr, int32_t *__restrict__ col,
                                                        double *__restrict__ val) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int q = qid[p];
  if (q < 0) return;
  const int b = q / nx, a = q - b * nx, a1 = a + 1 == nx ? 0 : a + 1;
  int32_t c0 = b * nx + a, c1 = b * nx + a1, c2 = (b + 1) * nx + a1, c3 = (b + 1) * nx + a;
  double w0 = wq[p], w1 = wq[n + p], w2 = wq[2 * n + p], w3 = wq[3 * n + p];
  ptm_cswap(c0, w0, c1, w1);
  ptm_cswap(c2, w2, c3, w3);
  ptm_cswap(c0, w0, c2, w2);
  ptm_cswap(c1, w1, c3, w3);
  ptm_cswap(c1, w1, c2, w2);
  const int64_t o = rowptr[p];
  col[o] = c0; col[o + 1] = c1; col[o + 2] = c2; col[o + 3] = c3;
  val[o] = w0; val[o + 1] = w1; val[o + 2] = w2; val[o + 3] = w3;
}
// cap rows: one wavefront per listed point, lanes over the row's nx columns
__global__ __launch_bounds__(256) void k_ptm_fill_caps(int nlist, const int32_t *__restrict__ list, int64_t n, int nx, int ny,
                                                       const int32_t *__restrict__ qid, const double *__restrict__ wq,
                                                       const int32_t *__restrict__ rowptr, int32_t *__restrict__ col, double *__restrict__ val) {
  const int lane = threadIdx.x & (MPG_WAVE - 1);
  const int k = (int)((blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / MPG_WAVE);
  if (k >= nlist) return;
  const int64_t p = list[k];
  const int q = qid[p];
  if (q > -2) return;   // under MPG_POLEMETHOD_NONE, or in a missing cap: an empty row
  const int id = -2 - q;
  const bool is_north = id >= nx;
  const int a = is_north ? id - nx : id, a1 = a + 1 == nx ? 0 : a + 1;
  const int32_t row0 = is_north ? (ny - 1) * nx : 0;
  const double tA = wq[p], tB = wq[n + p], wr = wq[2 * n + p] / (double)nx;
  const int64_t o = rowptr[p];
  for (int i = lane; i < nx; i += MPG_WAVE) {
    col[o + i] = row0 + i;
    val[o + i] = i == a ? tA + wr : i == a1 ? tB + wr : wr;
  }
}

// The index route needs a lat-lon grid that closes the circle, with its projection attached and checked (CENTER points).  A mesh POINT
// needs less of the inverse than the figures of the other Stores (mpg_grid_has_inverse: cells of 2 degrees at most): the quads' sides
// along i are meridians, exact in index space whatever the cell size, and the sides along j are chords of parallels, which leave their
// row by (atan(tan(lat) / cos(dlon / 2)) - lat) / dlat index units -- the route is taken when that stays within 0.04 up to
// MPG_LATLON_BOX_LIMIT, inside the 0.05 every index box is padded by.
static bool ptm_index_route(const mpg_grid_s *g) {
  if (!mpg_store_boxes() || !g->has_inverse || !g->inverse_ok[MPG_STAGGERLOC_CENTER] || g->proj.code != MPG_PROJ_LATLON) return false;
  const double rad = M_PI / 180.0, dlon = fabs(g->proj.loninc), dlat = fabs(g->proj.latinc);
  if (!(dlon > 0.0) || !(dlat > 0.0) || fabs((double)g->nx * dlon - 360.0) > 1e-6) return false;
  double bulge = 0.0;
  for (int lat = 1; lat <= (int)MPG_LATLON_BOX_LIMIT; ++lat)
    bulge = fmax(bulge, (atan(tan(lat * rad) / cos(0.5 * dlon * rad)) / rad - (double)lat) / dlat);
  return bulge <= 0.04;
}

// The pole each end row closes on, once per grid: the sign of the mean z of CENTER row 0 and of row ny - 1, summed on the host in column
// order (one number per end decides every triangle of its fan; no lane, no atomic takes part).
int mpg_k_grid_end_poles(mpg_grid_s *g, hipStream_t s) {
  if (g->end_pole[0] && g->end_pole[1]) return MPG_SUCCESS;
  const int nx = g->nx;
  const double *z = g->pts[MPG_STAGGERLOC_CENTER].z.p;
  std::vector<double> row(2 * (size_t)nx);
  MPG_HIP(hipMemcpyAsync(row.data(), z, sizeof(double) * nx, hipMemcpyDeviceToHost, s));
  MPG_HIP(hipMemcpyAsync(row.data() + nx, z + (int64_t)(g->ny - 1) * nx, sizeof(double) * nx, hipMemcpyDeviceToHost, s));
  MPG_HIP(hipStreamSynchronize(s));
  for (int e = 0; e < 2; ++e) {
    double sum = 0.0;
    for (int i = 0; i < nx; ++i) sum += row[(size_t)e * nx + i];
    g->end_pole[e] = sum < 0.0 ? -1 : 1;
  }
  return MPG_SUCCESS;
}

// The Store onto any list of points: `dst` holds n = nx_dst * ny_dst of them (a mesh location: ny_dst = 1; a stagger of another grid: its
// snx x sny).  `who` names the entry point in the messages.
int mpg_k_store_periodic_to_points(mpg_grid_s *g, const PointSet &dst, int64_t n, int nx_dst, int ny_dst, int pole_method, const char *who,
                                   mpg_handle_s *h, hipStream_t s) {
  int rc;
  const PointSet &src = g->pts[MPG_STAGGERLOC_CENTER];
  const int nx = g->nx, ny = g->ny;
  h->kind = MPG_KIND_CSR;
  h->nnz_per_row = 0;
  h->n_src = (int64_t)nx * ny;
  h->n_dst = n;
  h->nx_dst = nx_dst;
  h->ny_dst = ny_dst;
  h->nnz = 0;
  if ((rc = h->rowptr.alloc((size_t)n + 1))) return rc;
  if (n == 0) {
    MPG_HIP(hipMemsetAsync(h->rowptr.p, 0, sizeof(int32_t), s));
    MPG_HIP(hipStreamSynchronize(s));
    return MPG_SUCCESS;
  }
  const int no_pole = g->periodic & (MPG_GRID_NO_SOUTH_POLE | MPG_GRID_NO_NORTH_POLE);
  const bool caps = pole_method == MPG_POLEMETHOD_ALLAVG && no_pole != (MPG_GRID_NO_SOUTH_POLE | MPG_GRID_NO_NORTH_POLE);
  if (caps) {
    if ((rc = mpg_k_grid_end_poles(g, s))) return rc;
    if (!no_pole && g->end_pole[0] == g->end_pole[1]) {
      mpg_set_error("%s: CENTER rows 0 and %d both lie in the %s hemisphere, so at most one of them closes on a "
                    "pole; a row block passes MPG_GRID_NO_SOUTH_POLE (row 0) / MPG_GRID_NO_NORTH_POLE (row ny - 1) for the end that does not",
                    who, g->ny - 1, g->end_pole[0] > 0 ? "northern" : "southern");
      return MPG_ERR_INVALID_ARG;
    }
  }
  Pyramid &pyr = g->wrappyr;
  if (!pyr.built && (rc = mpg_k_build_wrap_pyramid(src, nx, ny, pyr, s))) return rc;
  if ((rc = mpg_walk_check<PyrTree>((int64_t)pyr.nx[0] * pyr.ny[0], who))) return rc;
  TmpBuf<float> ij;
  const bool use_ij = ptm_index_route(g);
  if (use_ij) {
    if ((rc = ij.alloc(2 * (size_t)n, s))) return rc;
    if ((rc = mpg_k_points_ij(g, n, dst.x.p, dst.y.p, dst.z.p, ij.p, s, MPG_LATLON_BOX_LIMIT, false))) return rc;
  }
  TmpBuf<unsigned long long> cnt;   // [0] index points that took the walk, [1] cap rows, [2] seam-quad rows
  TmpBuf<int32_t> qid, len, list;
  TmpBuf<double> wq;
  TmpBuf<long long> tot;
  if ((rc = cnt.alloc(3, s)) || (rc = qid.alloc((size_t)n, s)) || (rc = len.alloc((size_t)n + 1, s)) || (rc = wq.alloc(4 * (size_t)n, s)) ||
      (rc = tot.alloc(1, s)))
    return rc;
  MPG_HIP(hipMemsetAsync(cnt.p, 0, 3 * sizeof(unsigned long long), s));
  const unsigned nb = (unsigned)((n + 255) / 256), nb1 = (unsigned)((n + 256) / 256);
  const double tol = mpg_grid_inside_tol_exp() == 10 ? MPG_TOL : pow(10.0, -(double)mpg_grid_inside_tol_exp());
  k_ptm_quads<<<nb, 256, 0, s>>>(n, dst.x.p, dst.y.p, dst.z.p, nx, ny, src.x.p, src.y.p, src.z.p, use_ij ? ij.p : nullptr,
                                 (float)mpg_grid_box_pad_coef(g), (float)mpg_grid_box_pad_latlon(g), mpg_pyr_view(pyr), tol, qid.p, wq.p, cnt.p);
  MPG_HIP(hipGetLastError());
  // the points no quad took, as a list of exact size: count, scan, fill (len serves as the flags and then as the offsets)
  int32_t nlist = 0;
  if (caps) {
    k_ptm_miss<<<nb1, 256, 0, s>>>(n, qid.p, len.p);
    MPG_HIP(hipGetLastError());
    if ((rc = mpg_scan_excl_i32(len.p, len.p, n + 1, s))) return rc;
    MPG_HIP(hipMemcpyAsync(&nlist, len.p + n, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MPG_HIP(hipStreamSynchronize(s));   // (at most n < 2^31 flags: the int32 scan cannot wrap)
    if (nlist > 0) {
      if ((rc = list.alloc((size_t)nlist, s))) return rc;
      k_ptm_list<<<nb, 256, 0, s>>>(n, qid.p, len.p, list.p);
      k_ptm_caps<<<(unsigned)(((int64_t)nlist * MPG_WAVE + 255) / 256), 256, 0, s>>>(nlist, list.p, n, dst.x.p, dst.y.p, dst.z.p, nx, ny, g->periodic,
                                                                                    (double)g->end_pole[0], (double)g->end_pole[1], src.x.p, src.y.p, src.z.p, qid.p, wq.p);
      MPG_HIP(hipGetLastError());
    }
  }
  // CSR assembly: row lengths, offsets (the int32 scan beside a 64-bit total: the scan could wrap), fill
  k_ptm_rowlen<<<nb1, 256, 0, s>>>(n, nx, qid.p, len.p, cnt.p);
  MPG_HIP(hipGetLastError());
  if ((rc = mpg_scan_excl_i32(len.p, h->rowptr.p, n + 1, s)) || (rc = mpg_sum_i32_i64(len.p, n, tot.p, s))) return rc;
  int32_t nnz = 0;
  long long total = 0;
  unsigned long long hc[3] = {0, 0, 0};
  MPG_HIP(hipMemcpyAsync(&nnz, h->rowptr.p + n, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipMemcpyAsync(&total, tot.p, sizeof(total), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipMemcpyAsync(hc, cnt.p, sizeof(hc), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipStreamSynchronize(s));
  if (nnz < 0 || total != (long long)nnz) {
    mpg_set_error("%s: %lld entries (%lld cap rows of %d) exceed 2^31; MPG_POLEMETHOD_NONE stores no cap rows, "
                  "and a destination split into parts stores fewer each",
                  who, total, (long long)hc[1], nx);
    return MPG_ERR_OVERFLOW;
  }
  h->nnz = nnz;
  if ((rc = h->col.alloc((size_t)nnz)) || (rc = h->val.alloc((size_t)nnz))) return rc;
  if (nnz > 0) {
    k_ptm_fill_quads<<<nb, 256, 0, s>>>(n, nx, qid.p, wq.p, h->rowptr.p, h->col.p, h->val.p);
    if (hc[1] > 0)
      k_ptm_fill_caps<<<(unsigned)(((int64_t)nlist * MPG_WAVE + 255) / 256), 256, 0, s>>>(nlist, list.p, n, nx, ny, qid.p, wq.p, h->rowptr.p,
                                                                                         h->col.p, h->val.p);
    MPG_HIP(hipGetLastError());
  }
  MPG_HIP(hipStreamSynchronize(s));   // the temporaries go back to the pool behind the fill
  // mpg_handle_store_stats: [1] points that had an index and still took the walk, [2] points in all, [3] cap rows, [4] seam-quad rows
  h->store_path = use_ij ? 1 : 0;
  h->store_stats[1] = (int64_t)hc[0];
  h->store_stats[2] = n;
  h->store_stats[3] = (int64_t)hc[1];
  h->store_stats[4] = (int64_t)hc[2];
  return MPG_SUCCESS;
}

int mpg_k_store_periodic_to_mesh(mpg_grid_s *g, mpg_mesh_s *m, int meshloc, int pole_method, mpg_handle_s *h, hipStream_t s) {
  const PointSet &dst = meshloc == MPG_MESHLOC_EDGE ? m->edge : meshloc == MPG_MESHLOC_ELEMENT ? m->cell : m->vert;
  const int64_t n = meshloc == MPG_MESHLOC_EDGE ? m->edge.n : meshloc == MPG_MESHLOC_ELEMENT ? m->nCells : m->nVertices;
  return mpg_k_store_periodic_to_points(g, dst, n, (int)n, 1, pole_method, "mpg_regrid_store_periodic_to_mesh", h, s);
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_store_periodic_to_mesh() { return (const void *)k_ptm_quads; }
