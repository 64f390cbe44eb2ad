// Creep-fill extrapolation (mpg_handle_creep): the unmapped rows of a route handle filled level by level, every new row the average of
// its already filled neighbours' rows, as a NEW CSR handle (include/mpassit_amd.h states the contract, creep.h is its arithmetic).  No
// source geometry and no search: only the destination's connectivity.  A Store-time family of passes:
//
//   set-up      k_cr_init      level[p] = 0 for a mapped row, CR_UNASSIGNED / CR_SKIPPED for an unmapped one; rlen[p] = the entries a mapped
//                              row has under the CSR-output rule.  A CSR input's rows are read in place (rpos = its rowptr); a fixed input
//               k_cr_fixed_csr is written out once as level 0's rows (slots in slot order, -1 slots dropped, a nearest handle's 1.0).
//                              The unmapped rows and the level-0 entries are counted and read back: nothing unmapped ends here.
//   per level L k_cr_front     one thread per unassigned point: Nb(p) (cr_neighbours), flag = a neighbour holds level L - 1 (cr_joins), cnt =
//                              the candidates of its row, the contributors' lengths summed.  Levels are only READ here.
//               mpg_scan_excl_i32 over the flags, mpg_sum_i32_i64 over the counts -> the front's size and the level's candidates, read back
//               k_cr_compact   the front in ascending id (list), level[p] = L, the rows' candidate counts -> scanned into offsets
//               k_cr_expand    one wave per front row: its contributors in ascending id, each one's entries in stored order, written as
//                              64-bit keys (front row << 32 | column) with their values, in candidate order
//               mpg_sort_pairs_u64_i32 (stable): every (row, column) run lies together, its terms still in candidate order
//               k_cr_heads     1 at the first term of every run -> scanned: the run's place in the level's rows; the count is read back
//               k_cr_values    one lane per run: cr_sum_div over its terms, the column and the value into the level's rows
//               k_cr_rows      rpos / rlen of the front's points
//   assembly    the row lengths summed in 64 bits (read back, checked), mpg_scan_excl_i32 -> rowptr; k_cr_gather0 copies the level-0 rows
//               (one thread per row) and records the longest row (an integer maximum); k_cr_gather, once per level, copies that level's
//               rows (one wave per row).
// The rows of a level are a block of their own, kept until the assembly: a level reads only the level below it.  There is no per-row
// buffer in registers or LDS: rows of any length take the same path, and there is no blocking knob.  Two host round trips per level.
// No floating-point atomics, and the sort is stable: the same bytes from run to run.
#pragma clang fp contract(off)
#include <memory>
#include <vector>

#include "mpg_internal.h"
#include "creep.h"

struct CrIn {
  const int32_t *rowptr;   // CSR row pointers; nullptr: fixed slots
  const int32_t *col;      // CSR columns, or idx [nz][n] (-1 = none)
  const double *val;       // CSR values, or w [nz][n]; nullptr: every value 1.0 (nearest)
  int nz;                  // slots of a fixed handle
  int64_t n;               // rows
};

// the rows of one level: `col` / `val` hold them back to back; list = its points in ascending id (level 0: none, every mapped row)
struct CrLevel {
  TmpBuf<int32_t> col, list;
  TmpBuf<double> val;
  int64_t nf = 0;
};

static inline unsigned cr_grid(int64_t n) { return (unsigned)((n + 255) / 256); }
static inline unsigned cr_wgrid(int64_t rows) { return (unsigned)((rows + 3) / 4); }   // one wave per row, four to a workgroup

// level, rlen [n + 1] (rlen[n] = 0), unm [n + 1] = 1 at an unmapped row (unm[n] = 0)
__global__ __launch_bounds__(256) void k_cr_init(CrIn in, const uint8_t *__restrict__ skip, int32_t *__restrict__ level,
                                                 int32_t *__restrict__ rlen, int32_t *__restrict__ unm) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > in.n) return;
  int len = 0, u = 0;
  if (i < in.n) {
    if (in.rowptr) len = in.rowptr[i + 1] - in.rowptr[i];
    else if (in.col[i] >= 0)
      for (int s = 0; s < in.nz; ++s) len += in.col[(int64_t)s * in.n + i] >= 0;
    u = len == 0;
    level[i] = !u ? 0 : (skip && skip[i]) ? CR_SKIPPED : CR_UNASSIGNED;
  }
  rlen[i] = len;
  unm[i] = u;
}

// a fixed input's mapped rows as CSR rows at rpos
__global__ __launch_bounds__(256) void k_cr_fixed_csr(CrIn in, const int32_t *__restrict__ rpos, const int32_t *__restrict__ rlen,
                                                      int32_t *__restrict__ col, double *__restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= in.n || rlen[i] == 0) return;
  int64_t at = rpos[i];
  for (int s = 0; s < in.nz; ++s) {
    const int32_t c = in.col[(int64_t)s * in.n + i];
    if (c < 0) continue;
    col[at] = c;
    val[at] = in.val ? in.val[(int64_t)s * in.n + i] : 1.0;
    ++at;
  }
}

// flag, cnt [n + 1] (both 0 at n and at every point that does not join level L)
__global__ __launch_bounds__(256) void k_cr_front(PtSrc dst, int64_t n, const int32_t *__restrict__ level, const int32_t *__restrict__ rlen, int L,
                                                  int32_t *__restrict__ flag, int32_t *__restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  int f = 0;
  int64_t c = 0;
  if (i < n && level[i] == CR_UNASSIGNED) {
    int32_t nb[CR_MAX_NB];
    const int m = cr_neighbours(dst, (int32_t)i, nb);
    f = cr_joins(level, nb, m, L);
    if (f)
      for (int k = 0; k < m; ++k)
        if (level[nb[k]] == L - 1) c += rlen[nb[k]];
  }
  flag[i] = f;
  cnt[i] = (int32_t)(c < 0x7fffffffLL ? c : 0x7fffffffLL);   // (a clamped count takes the level's 64-bit sum past the limit: refused)
}

// list [nf] ascending, level[p] = L, ccnt [nf + 1] (ccnt[nf] = 0)
__global__ __launch_bounds__(256) void k_cr_compact(int64_t n, const int32_t *__restrict__ flag, const int32_t *__restrict__ fpos,
                                                    const int32_t *__restrict__ cnt, int L, int32_t *__restrict__ list,
                                                    int32_t *__restrict__ level, int32_t *__restrict__ ccnt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  if (i == n) {
    ccnt[fpos[n]] = 0;
  } else if (flag[i]) {
    const int32_t u = fpos[i];
    list[u] = (int32_t)i;
    level[i] = L;
    ccnt[u] = cnt[i];
  }
}

// one wave per front row u: keys / cval / cidx at [coff[u], coff[u + 1]) in (contributor, stored) order, mcnt[u] = the contributors
__global__ __launch_bounds__(256) void k_cr_expand(PtSrc dst, int64_t nf, const int32_t *__restrict__ list, const int32_t *__restrict__ level, int L,
                                                   const int32_t *__restrict__ rpos, const int32_t *__restrict__ rlen,
                                                   const int32_t *__restrict__ pcol, const double *__restrict__ pval,
                                                   const int32_t *__restrict__ coff, unsigned long long *__restrict__ keys,
                                                   double *__restrict__ cval, int32_t *__restrict__ cidx, int32_t *__restrict__ mcnt) {
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (u >= nf) return;
  int32_t nb[CR_MAX_NB];
  const int nn = cr_neighbours(dst, list[u], nb);
  int64_t at = coff[u];
  const int64_t end = coff[u + 1];
  int m = 0;
  for (int k = 0; k < nn; ++k) {
    const int32_t q = nb[k];
    if (level[q] != L - 1) continue;
    const int64_t b = rpos[q];
    const int32_t len = rlen[q];
    for (int32_t e = lane; e < len && at + e < end; e += 64) {   // (at + len <= end by k_cr_front's count: the test keeps a store inside whatever happens)
      keys[at + e] = ((unsigned long long)u << 32) | (unsigned long long)(uint32_t)pcol[b + e];
      cval[at + e] = pval[b + e];
      cidx[at + e] = (int32_t)(at + e);
    }
    at += len;
    ++m;
  }
  if (lane == 0) mcnt[u] = m;
}

// head [nc + 1]: 1 at the first term of a (row, column) run, head[nc] = 0
__global__ __launch_bounds__(256) void k_cr_heads(int64_t nc, const unsigned long long *__restrict__ keys, int32_t *__restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > nc) return;
  head[i] = i < nc && (i == 0 || keys[i] != keys[i - 1]);
}

// one lane per run: the column and cr_sum_div of its terms, which the stable sort left in candidate order
__global__ __launch_bounds__(256) void k_cr_values(int64_t nc, const unsigned long long *__restrict__ keys, const int32_t *__restrict__ sidx,
                                                   const int32_t *__restrict__ head, const int32_t *__restrict__ hpos,
                                                   const double *__restrict__ cval, const int32_t *__restrict__ mcnt,
                                                   int32_t *__restrict__ col, double *__restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nc || !head[i]) return;
  const unsigned long long key = keys[i];
  int64_t len = 1;
  while (i + len < nc && keys[i + len] == key) ++len;
  const int64_t j = hpos[i];
  col[j] = (int32_t)(uint32_t)(key & 0xffffffffull);
  val[j] = cr_sum_div(len, [&](int64_t k) { return cval[sidx[i + k]]; }, mcnt[key >> 32]);
}

// where the rows of the front's points lie in the level's block
__global__ __launch_bounds__(256) void k_cr_rows(int64_t nf, const int32_t *__restrict__ list, const int32_t *__restrict__ coff,
                                                 const int32_t *__restrict__ hpos, int32_t *__restrict__ rpos, int32_t *__restrict__ rlen) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= nf) return;
  const int32_t a = hpos[coff[u]], b = hpos[coff[u + 1]];
  rpos[list[u]] = a;
  rlen[list[u]] = b - a;
}

// the level-0 rows into the output, one thread per row; the longest row of ALL rows (an integer maximum: the order does not matter)
__global__ __launch_bounds__(256) void k_cr_gather0(int64_t n, const int32_t *__restrict__ level, const int32_t *__restrict__ rpos,
                                                    const int32_t *__restrict__ pcol, const double *__restrict__ pval,
                                                    const int32_t *__restrict__ rowptr, int32_t *__restrict__ col, double *__restrict__ val,
                                                    int32_t *__restrict__ longest) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int32_t len = 0;
  if (i < n) {
    const int64_t at = rowptr[i];
    len = rowptr[i + 1] - (int32_t)at;
    if (level[i] == 0) {
      const int64_t b = rpos[i];
      for (int q = 0; q < len; ++q) {
        col[at + q] = pcol[b + q];
        val[at + q] = pval[b + q];
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) len = max(len, __shfl_down(len, o));
  if ((threadIdx.x & 63) == 0 && len > 0) atomicMax(longest, len);
}

// the rows of one level into the output, one wave per row
__global__ __launch_bounds__(256) void k_cr_gather(int64_t nf, const int32_t *__restrict__ list, const int32_t *__restrict__ rpos,
                                                   const int32_t *__restrict__ pcol, const double *__restrict__ pval,
                                                   const int32_t *__restrict__ rowptr, int32_t *__restrict__ col, double *__restrict__ val) {
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= nf) return;
  const int64_t p = list[u], at = rowptr[p], b = rpos[p];
  const int32_t len = rowptr[p + 1] - (int32_t)at;
  for (int32_t e = threadIdx.x & 63; e < len; e += 64) {
    col[at + e] = pcol[b + e];
    val[at + e] = pval[b + e];
  }
}

static int cr_too_many(long long n, const char *what) {
  mpg_set_error("mpg_handle_creep: %s would be %lld, more than 2^31 - 2 (rowptr and the passes' offsets are int32): lower num_levels, or "
                "creep the parts of the destination separately", what, n);
  return MPG_ERR_OVERFLOW;
}

// in: the handle to fill; dst: the connectivity of its in->n_dst destination points (creep.h: a mesh's voc / tri, or a stagger's snx, sny;
// no coordinates are read).  out: shape and method set by the caller, arrays empty.  Arguments checked by the API entry point; blocking.
int mpg_k_creep(mpg_handle_s *in, const PtSrc &dst, int num_levels, const uint8_t *dst_skip, mpg_handle_s *out, hipStream_t s) {
  int rc;
  const int64_t n = in->n_dst;
  CrIn I;
  if (in->kind == MPG_KIND_CSR) {
    I.rowptr = in->rowptr.p; I.col = in->col.p; I.val = in->val.p; I.nz = 0;
  } else {
    I.rowptr = nullptr; I.col = in->idx.p; I.val = in->w.p; I.nz = in->nnz_per_row;
  }
  I.n = n;
  out->kind = MPG_KIND_CSR;
  out->nnz_per_row = 0;
  // set-up
  TmpBuf<int32_t> level, rlen, rpos, flag, fpos, cnt;
  TmpBuf<long long> sums;   // [0] unmapped rows / a level's candidates / the output's entries, [1] level 0's entries
  if ((rc = level.alloc((size_t)n + 1, s)) || (rc = rlen.alloc((size_t)n + 1, s)) || (rc = rpos.alloc((size_t)n + 1, s)) ||
      (rc = flag.alloc((size_t)n + 1, s)) || (rc = fpos.alloc((size_t)n + 1, s)) || (rc = cnt.alloc((size_t)n + 1, s)) || (rc = sums.alloc(2, s)))
    return rc;
  k_cr_init<<<cr_grid(n + 1), 256, 0, s>>>(I, dst_skip, level.p, rlen.p, flag.p);
  MPG_HIP(hipGetLastError());
  if ((rc = mpg_sum_i32_i64(flag.p, n + 1, sums.p, s)) || (rc = mpg_sum_i32_i64(rlen.p, n + 1, sums.p + 1, s))) return rc;
  long long host[2] = {0, 0};
  MPG_HIP(hipMemcpyAsync(host, sums.p, sizeof(host), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipStreamSynchronize(s));
  const long long unmapped0 = host[0], nnz0 = host[1];
  if (nnz0 > 0x7ffffffeLL) return cr_too_many(nnz0, "the entries of the mapped rows alone");
  std::vector<std::unique_ptr<CrLevel>> levels;
  levels.emplace_back(new CrLevel());
  const int32_t *col0 = I.col;
  const double *val0 = I.val;
  if (I.rowptr) {
    MPG_HIP(hipMemcpyAsync(rpos.p, I.rowptr, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyDeviceToDevice, s));
  } else {
    CrLevel &l0 = *levels[0];
    if ((rc = mpg_scan_excl_i32(rlen.p, rpos.p, n + 1, s))) return rc;
    if ((rc = l0.col.alloc((size_t)nnz0 + 1, s)) || (rc = l0.val.alloc((size_t)nnz0 + 1, s))) return rc;
    if (n > 0) k_cr_fixed_csr<<<cr_grid(n), 256, 0, s>>>(I, rpos.p, rlen.p, l0.col.p, l0.val.p);
    MPG_HIP(hipGetLastError());
    col0 = l0.col.p;
    val0 = l0.val.p;
  }
  // the levels
  long long filled = 0;
  int last = 0;
  for (int L = 1; unmapped0 - filled > 0 && L <= num_levels; ++L) {
    k_cr_front<<<cr_grid(n + 1), 256, 0, s>>>(dst, n, level.p, rlen.p, L, flag.p, cnt.p);
    MPG_HIP(hipGetLastError());
    if ((rc = mpg_scan_excl_i32(flag.p, fpos.p, n + 1, s)) || (rc = mpg_sum_i32_i64(cnt.p, n + 1, sums.p, s))) return rc;
    int32_t nf32 = 0;
    long long nc = 0;
    MPG_HIP(hipMemcpyAsync(&nf32, fpos.p + n, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MPG_HIP(hipMemcpyAsync(&nc, sums.p, sizeof(long long), hipMemcpyDeviceToHost, s));
    MPG_HIP(hipStreamSynchronize(s));
    const int64_t nf = nf32;
    if (nf == 0) break;   // the first level that assigns nothing ends the loop
    if (nc > 0x7ffffffeLL) return cr_too_many(nc, "the candidate entries of one level");
    levels.emplace_back(new CrLevel());
    CrLevel &lv = *levels.back();
    const CrLevel &below = *levels[L - 1];
    const int32_t *pcol = L == 1 ? col0 : below.col.p;
    const double *pval = L == 1 ? val0 : below.val.p;
    lv.nf = nf;
    TmpBuf<int32_t> ccnt, coff, mcnt, cidx, sidx, head, hpos;
    TmpBuf<unsigned long long> keys, skeys;
    TmpBuf<double> cval;
    if ((rc = lv.list.alloc((size_t)nf, s)) || (rc = ccnt.alloc((size_t)nf + 1, s)) || (rc = coff.alloc((size_t)nf + 1, s)) ||
        (rc = mcnt.alloc((size_t)nf, s)) || (rc = cidx.alloc((size_t)nc + 1, s)) || (rc = sidx.alloc((size_t)nc + 1, s)) ||
        (rc = head.alloc((size_t)nc + 1, s)) || (rc = hpos.alloc((size_t)nc + 1, s)) || (rc = keys.alloc((size_t)nc + 1, s)) ||
        (rc = skeys.alloc((size_t)nc + 1, s)) || (rc = cval.alloc((size_t)nc + 1, s)))
      return rc;
    k_cr_compact<<<cr_grid(n + 1), 256, 0, s>>>(n, flag.p, fpos.p, cnt.p, L, lv.list.p, level.p, ccnt.p);
    MPG_HIP(hipGetLastError());
    if ((rc = mpg_scan_excl_i32(ccnt.p, coff.p, nf + 1, s))) return rc;
    k_cr_expand<<<cr_wgrid(nf), 256, 0, s>>>(dst, nf, lv.list.p, level.p, L, rpos.p, rlen.p, pcol, pval, coff.p, keys.p, cval.p, cidx.p, mcnt.p);
    MPG_HIP(hipGetLastError());
    if ((rc = mpg_sort_pairs_u64_i32(keys.p, skeys.p, cidx.p, sidx.p, nc, s))) return rc;
    k_cr_heads<<<cr_grid(nc + 1), 256, 0, s>>>(nc, skeys.p, head.p);
    MPG_HIP(hipGetLastError());
    if ((rc = mpg_scan_excl_i32(head.p, hpos.p, nc + 1, s))) return rc;
    int32_t nd = 0;
    MPG_HIP(hipMemcpyAsync(&nd, hpos.p + nc, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MPG_HIP(hipStreamSynchronize(s));
    if ((rc = lv.col.alloc((size_t)nd + 1, s)) || (rc = lv.val.alloc((size_t)nd + 1, s))) return rc;
    if (nc > 0) k_cr_values<<<cr_grid(nc), 256, 0, s>>>(nc, skeys.p, sidx.p, head.p, hpos.p, cval.p, mcnt.p, lv.col.p, lv.val.p);
    k_cr_rows<<<cr_grid(nf), 256, 0, s>>>(nf, lv.list.p, coff.p, hpos.p, rpos.p, rlen.p);
    MPG_HIP(hipGetLastError());
    filled += nf;
    last = L;
  }
  out->store_stats[1] = filled;
  out->store_stats[2] = last;
  out->store_stats[3] = unmapped0 - filled;
  // assembly
  if ((rc = out->rowptr.alloc((size_t)n + 1))) return rc;
  TmpBuf<int32_t> longest;
  if ((rc = longest.alloc(1, s))) return rc;
  MPG_HIP(hipMemsetAsync(longest.p, 0, sizeof(int32_t), s));
  if ((rc = mpg_sum_i32_i64(rlen.p, n + 1, sums.p, s))) return rc;
  long long nnz = 0;
  MPG_HIP(hipMemcpyAsync(&nnz, sums.p, sizeof(long long), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipStreamSynchronize(s));
  if (nnz > 0x7ffffffeLL) return cr_too_many(nnz, "the entries of the CSR output");
  if ((rc = mpg_scan_excl_i32(rlen.p, out->rowptr.p, n + 1, s))) return rc;
  if ((rc = out->col.alloc((size_t)nnz + 1)) || (rc = out->val.alloc((size_t)nnz + 1))) return rc;
  out->nnz = nnz;
  if (n > 0) {
    k_cr_gather0<<<cr_grid(n), 256, 0, s>>>(n, level.p, rpos.p, col0, val0, out->rowptr.p, out->col.p, out->val.p, longest.p);
    for (size_t L = 1; L < levels.size(); ++L) {
      const CrLevel &lv = *levels[L];
      k_cr_gather<<<cr_wgrid(lv.nf), 256, 0, s>>>(lv.nf, lv.list.p, rpos.p, lv.col.p, lv.val.p, out->rowptr.p, out->col.p, out->val.p);
    }
    MPG_HIP(hipGetLastError());
  }
  int32_t max_row = 0;
  MPG_HIP(hipMemcpyAsync(&max_row, longest.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipStreamSynchronize(s));   // (the temporaries may go)
  out->max_row = max_row;
  out->store_stats[6] = max_row;
  return MPG_SUCCESS;
}

// mpg_init loads this translation unit's code object ahead of its first launch (mpg_api.hip: warm_modules)
const void *mpg_anchor_k_creep() { return (const void *)&k_cr_front; }
