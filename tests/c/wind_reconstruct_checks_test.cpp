// The argument checks of the three wind-reconstruction calls (mpassit_amd/csrc/wind_reconstruct_checks.h, the text mpg_api.hip compiles)
// run on the host: every refusal by code and by a word of its message, the accepted forms, the arithmetic at the edges of the 64-bit
// range, and the LDS bytes in front of the kernel's tiles.  Only the Store's check reads its (host) arrays; the others never dereference
// an array: host buffers stand in for device memory.  Built by tests/test_wind_reconstruct_checks.py with -fsanitize=address,undefined.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../mpassit_amd/csrc/wind_reconstruct_checks.h"

static int failures = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

static bool refused(int rc, int want, const WvErr &e, const char *who, const char *word) {
  const bool ok = rc == want && strstr(e.msg, who) && (!word || strstr(e.msg, word));
  if (!ok) printf("  rc %d (want %d), message: %s\n", rc, want, e.msg);
  return ok;
}

static WrHandle handle(bool csr, int64_t n_pole, int64_t ns, int64_t nd, int64_t nnz, int64_t max_row) {
  WrHandle h;
  h.csr = csr;
  h.n_pole = n_pole;
  h.n_src = ns;
  h.n_dst = nd;
  h.nnz = nnz;
  h.max_row = max_row;
  return h;
}

int main() {
  WvErr e;
  memset(&e, 0, sizeof e);
  // ---- the Store
  {
    const char *who = "mpg_reconstruct_store";
    const int me = 4;
    const int64_t nc = 5, ne = 9;
    std::vector<int32_t> n = {3, 0, 4, 2, 1};
    std::vector<int32_t> eoc = {1, 2, 3, 0, /**/ 0, 0, 0, 0, /**/ 9, 9, 1, 5, /**/ 4, 6, -7, 99, /**/ 8, 0, 0, 0};   // slots past the count are not read
    void *out = &e;
    int64_t nnz = -1, longest = -1;
    EXPECT(wr_check_store(nc, ne, me, n.data(), eoc.data(), out, &nnz, &longest, e) == MPG_SUCCESS && nnz == 10 && longest == 4);
    std::vector<int32_t> zero(nc, 0);
    EXPECT(wr_check_store(nc, ne, me, zero.data(), eoc.data(), out, &nnz, &longest, e) == MPG_SUCCESS && nnz == 0 && longest == 0);
    EXPECT(wr_check_store(nc, ne, 0, zero.data(), eoc.data(), out, &nnz, &longest, e) == MPG_SUCCESS && nnz == 0);
    EXPECT(refused(wr_check_store(nc, ne, me, nullptr, eoc.data(), out, &nnz, &longest, e), MPG_ERR_INVALID_ARG, e, who, "NULL"));
    EXPECT(refused(wr_check_store(nc, ne, me, n.data(), nullptr, out, &nnz, &longest, e), MPG_ERR_INVALID_ARG, e, who, "NULL"));
    EXPECT(refused(wr_check_store(nc, ne, me, n.data(), eoc.data(), nullptr, &nnz, &longest, e), MPG_ERR_INVALID_ARG, e, who, "NULL"));
    EXPECT(refused(wr_check_store(0, ne, me, n.data(), eoc.data(), out, &nnz, &longest, e), MPG_ERR_INVALID_ARG, e, who, "sizes"));
    EXPECT(refused(wr_check_store(nc, 0, me, n.data(), eoc.data(), out, &nnz, &longest, e), MPG_ERR_INVALID_ARG, e, who, "sizes"));
    EXPECT(refused(wr_check_store(nc, ne, -1, n.data(), eoc.data(), out, &nnz, &longest, e), MPG_ERR_INVALID_ARG, e, who, "sizes"));
    EXPECT(refused(wr_check_store(0x7fffffffll, ne, me, n.data(), eoc.data(), out, &nnz, &longest, e), MPG_ERR_OVERFLOW, e, who, "int32"));
    EXPECT(refused(wr_check_store(nc, 0x7fffffffll, me, n.data(), eoc.data(), out, &nnz, &longest, e), MPG_ERR_OVERFLOW, e, who, "int32"));
    std::vector<int32_t> bad = n;
    bad[2] = 5;                                                                      // a count above maxEdges, with its cell
    EXPECT(refused(wr_check_store(nc, ne, me, bad.data(), eoc.data(), out, &nnz, &longest, e), MPG_ERR_INVALID_ARG, e, who, "cell 2"));
    bad[2] = -1;
    EXPECT(refused(wr_check_store(nc, ne, me, bad.data(), eoc.data(), out, &nnz, &longest, e), MPG_ERR_INVALID_ARG, e, who, "cell 2"));
    bad = n;
    bad[3] = 3;                                                                      // counts the slot that holds -7
    EXPECT(refused(wr_check_store(nc, ne, me, bad.data(), eoc.data(), out, &nnz, &longest, e), MPG_ERR_INVALID_ARG, e, who, "cell 3"));
    EXPECT(strstr(e.msg, "-7") != nullptr);
    EXPECT(refused(wr_check_store(nc, 8, me, n.data(), eoc.data(), out, &nnz, &longest, e), MPG_ERR_INVALID_ARG, e, who, "cell 2"));   // id 9 > nEdges 8
    bad = n;
    bad[1] = 1;                                                                      // id 0: ids are 1-based
    EXPECT(refused(wr_check_store(nc, ne, me, bad.data(), eoc.data(), out, &nnz, &longest, e), MPG_ERR_INVALID_ARG, e, who, "1-based"));
  }
  const int64_t ns = 288, nd = 100, nnz = 600;
  const int me = 8;
  const WrHandle csr = handle(true, 0, ns, nd, nnz, 8), fixed = handle(false, 0, ns, nd, 0, -1), pole = handle(false, 7, ns, nd, 0, -1),
                 csr_pole = handle(true, 7, ns, nd, nnz, 8), none = handle(true, 0, ns, nd, 0, 0), unknown = handle(true, 0, ns, nd, nnz, -1);
  // ---- the values
  {
    const char *who = "mpg_reconstruct_weights";
    std::vector<double> co(nd * me * 3), df(6 * nd), m(3 * nnz);
    bool nothing = true;
    EXPECT(wr_check_weights(&csr, me, co.data(), df.data(), m.data(), &nothing, e) == MPG_SUCCESS && !nothing);
    EXPECT(wr_check_weights(&csr, me, co.data(), nullptr, m.data(), &nothing, e) == MPG_SUCCESS && !nothing);          // NULL frames: X, Y, Z
    EXPECT(wr_check_weights(&csr, me + 4, co.data(), nullptr, m.data(), &nothing, e) == MPG_SUCCESS);
    EXPECT(wr_check_weights(&none, me, nullptr, nullptr, nullptr, &nothing, e) == MPG_SUCCESS && nothing);             // no entries: writes nothing
    EXPECT(refused(wr_check_weights(nullptr, me, co.data(), df.data(), m.data(), &nothing, e), MPG_ERR_INVALID_ARG, e, who, "NULL handle"));
    EXPECT(refused(wr_check_weights(&fixed, me, co.data(), df.data(), m.data(), &nothing, e), MPG_ERR_UNSUPPORTED, e, who, "fixed"));
    EXPECT(refused(wr_check_weights(&pole, me, co.data(), df.data(), m.data(), &nothing, e), MPG_ERR_UNSUPPORTED, e, who, "pole"));
    EXPECT(refused(wr_check_weights(&csr_pole, me, co.data(), df.data(), m.data(), &nothing, e), MPG_ERR_UNSUPPORTED, e, who, "pole"));
    EXPECT(refused(wr_check_weights(&csr, me - 1, co.data(), df.data(), m.data(), &nothing, e), MPG_ERR_INVALID_ARG, e, who, "exceeds maxEdges"));
    EXPECT(refused(wr_check_weights(&csr, -1, co.data(), df.data(), m.data(), &nothing, e), MPG_ERR_INVALID_ARG, e, who, "maxEdges"));
    EXPECT(refused(wr_check_weights(&unknown, me, co.data(), df.data(), m.data(), &nothing, e), MPG_ERR_INVALID_ARG, e, who, "longest row"));
    EXPECT(refused(wr_check_weights(&csr, me, nullptr, df.data(), m.data(), &nothing, e), MPG_ERR_INVALID_ARG, e, who, "NULL array"));
    EXPECT(refused(wr_check_weights(&csr, me, co.data(), df.data(), nullptr, &nothing, e), MPG_ERR_INVALID_ARG, e, who, "NULL array"));
    EXPECT(refused(wr_check_weights(&csr, me, co.data(), df.data(), co.data() + nd * me * 3 - 1, &nothing, e), MPG_ERR_INVALID_ARG, e, who, "alias"));
    EXPECT(refused(wr_check_weights(&csr, me, co.data(), m.data() + 2 * nnz - 1, m.data(), &nothing, e), MPG_ERR_INVALID_ARG, e, who, "alias"));
    // with frames the values are two planes: what lies behind them is an array of its own; without, three
    EXPECT(wr_check_weights(&csr, 2, m.data() + 2 * nnz, df.data(), m.data(), &nothing, e) == MPG_ERR_INVALID_ARG);    // (longest row 8 > 2)
    const WrHandle two = handle(true, 0, ns, nd, nnz, 2);
    EXPECT(wr_check_weights(&two, 2, m.data() + 2 * nnz, df.data(), m.data(), &nothing, e) == MPG_SUCCESS);
    EXPECT(refused(wr_check_weights(&two, 2, m.data() + 2 * nnz, nullptr, m.data(), &nothing, e), MPG_ERR_INVALID_ARG, e, who, "alias"));
    const WrHandle wide = handle(true, 0, 1, INT64_MAX / 64, 4, 8);
    EXPECT(refused(wr_check_weights(&wide, 8, co.data(), nullptr, m.data(), &nothing, e), MPG_ERR_INVALID_ARG, e, who, "addressed"));
  }
  // ---- the apply
  {
    const char *who = "mpg_wind_reconstruct";
    const int nlev = 3, CF = MPG_LAYOUT_CELL_FAST, LF = MPG_LAYOUT_LEV_FAST;
    std::vector<double> m(3 * nnz), u(nlev * (ns + 5)), r0(nlev * nd), r1(nlev * nd), r2(nlev * nd), big(3 * nnz + 3 * nlev * nd);
    int64_t ld = -1;
    auto call = [&](const WrHandle *h, const double *mm, int nout, const void *uu, int st, int sl, int64_t lu, int nl, const void *a, const void *b,
                    const void *c, int dt, int dl) { return wr_check_apply(h, mm, nout, uu, st, sl, lu, nl, a, b, c, dt, dl, &ld, e); };
    EXPECT(call(&csr, m.data(), 2, u.data(), 0, LF, 0, nlev, r0.data(), r1.data(), nullptr, 0, CF) == MPG_SUCCESS && ld == ns);
    EXPECT(call(&csr, m.data(), 3, u.data(), 1, LF, 0, nlev, r0.data(), r1.data(), r2.data(), 1, LF) == MPG_SUCCESS && ld == ns);
    EXPECT(call(&csr, m.data(), 3, u.data(), 0, CF, 0, nlev, r0.data(), r1.data(), r2.data(), 1, LF) == MPG_SUCCESS && ld == ns);
    EXPECT(call(&csr, m.data(), 2, u.data(), 1, CF, ns + 5, nlev, r0.data(), r1.data(), nullptr, 0, CF) == MPG_SUCCESS && ld == ns + 5);
    EXPECT(call(&csr, m.data(), 2, u.data(), 1, CF, ns, nlev, r0.data(), r1.data(), nullptr, 0, CF) == MPG_SUCCESS && ld == ns);
    EXPECT(call(&unknown, m.data(), 2, u.data(), 0, LF, 0, nlev, r0.data(), r1.data(), nullptr, 0, CF) == MPG_SUCCESS);     // any CSR handle
    EXPECT(call(&none, nullptr, 2, u.data(), 0, LF, 0, nlev, r0.data(), r1.data(), nullptr, 0, CF) == MPG_SUCCESS);         // no entries: no values
    EXPECT(refused(call(nullptr, nullptr, 2, nullptr, 0, 0, 0, 0, nullptr, nullptr, nullptr, 0, 0), MPG_ERR_INVALID_ARG, e, who, "NULL handle"));
    EXPECT(refused(call(&csr, m.data(), 1, u.data(), 0, LF, 0, nlev, r0.data(), nullptr, nullptr, 0, CF), MPG_ERR_INVALID_ARG, e, who, "mpg_regrid_csr_to_mesh_dev"));
    EXPECT(strstr(e.msg, "mpg_regrid_csr_rows_dev") != nullptr);
    EXPECT(refused(call(&csr, m.data(), 0, u.data(), 0, LF, 0, nlev, r0.data(), r1.data(), nullptr, 0, CF), MPG_ERR_INVALID_ARG, e, who, "nout"));
    EXPECT(refused(call(&csr, m.data(), 4, u.data(), 0, LF, 0, nlev, r0.data(), r1.data(), r2.data(), 0, CF), MPG_ERR_INVALID_ARG, e, who, "nout"));
    EXPECT(refused(call(&csr, m.data(), 2, u.data(), 0, LF, 0, nlev, r0.data(), r1.data(), r2.data(), 0, CF), MPG_ERR_INVALID_ARG, e, who, "r2_dev"));
    EXPECT(refused(call(&csr, m.data(), 3, u.data(), 0, LF, 0, nlev, r0.data(), r1.data(), nullptr, 0, CF), MPG_ERR_INVALID_ARG, e, who, "r2_dev"));
    EXPECT(refused(call(&fixed, m.data(), 2, u.data(), 0, LF, 0, nlev, r0.data(), r1.data(), nullptr, 0, CF), MPG_ERR_UNSUPPORTED, e, who, "fixed"));
    EXPECT(refused(call(&pole, m.data(), 2, u.data(), 0, LF, 0, nlev, r0.data(), r1.data(), nullptr, 0, CF), MPG_ERR_UNSUPPORTED, e, who, "pole"));
    EXPECT(refused(call(&csr, m.data(), 2, u.data(), 2, LF, 0, nlev, r0.data(), r1.data(), nullptr, 0, CF), MPG_ERR_UNSUPPORTED, e, who, "mpg_bswap_dev"));
    EXPECT(refused(call(&csr, m.data(), 2, u.data(), 0, LF, 0, nlev, r0.data(), r1.data(), nullptr, 3, CF), MPG_ERR_UNSUPPORTED, e, who, "mpg_bswap_dev"));
    EXPECT(refused(call(&csr, nullptr, 2, u.data(), 0, LF, 0, nlev, r0.data(), r1.data(), nullptr, 0, CF), MPG_ERR_INVALID_ARG, e, who, "NULL array"));
    EXPECT(refused(call(&csr, m.data(), 2, nullptr, 0, LF, 0, nlev, r0.data(), r1.data(), nullptr, 0, CF), MPG_ERR_INVALID_ARG, e, who, "NULL array"));
    EXPECT(refused(call(&csr, m.data(), 2, u.data(), 0, LF, 0, nlev, nullptr, r1.data(), nullptr, 0, CF), MPG_ERR_INVALID_ARG, e, who, "NULL array"));
    EXPECT(refused(call(&csr, m.data(), 2, u.data(), 0, LF, 0, nlev, r0.data(), nullptr, nullptr, 0, CF), MPG_ERR_INVALID_ARG, e, who, "NULL array"));
    EXPECT(refused(call(&csr, m.data(), 2, u.data(), 0, LF, 0, 0, r0.data(), r1.data(), nullptr, 0, CF), MPG_ERR_INVALID_ARG, e, who, "nlev"));
    EXPECT(refused(call(&csr, m.data(), 2, u.data(), 0, LF, 0, -4, r0.data(), r1.data(), nullptr, 0, CF), MPG_ERR_INVALID_ARG, e, who, "nlev"));
    EXPECT(refused(call(&csr, m.data(), 2, u.data(), 0, LF, 0, nlev, r0.data(), r1.data(), nullptr, 0, 2), MPG_ERR_INVALID_ARG, e, who, "dst_layout"));
    EXPECT(refused(call(&csr, m.data(), 2, u.data(), 0, -1, 0, nlev, r0.data(), r1.data(), nullptr, 0, CF), MPG_ERR_INVALID_ARG, e, who, "src_layout"));
    EXPECT(refused(call(&csr, m.data(), 2, u.data(), 4, LF, 0, nlev, r0.data(), r1.data(), nullptr, 0, CF), MPG_ERR_INVALID_ARG, e, who, "src_type"));
    EXPECT(refused(call(&csr, m.data(), 2, u.data(), 0, LF, 0, nlev, r0.data(), r1.data(), nullptr, -1, CF), MPG_ERR_INVALID_ARG, e, who, "dst_type"));
    EXPECT(refused(call(&csr, m.data(), 2, u.data(), 0, LF, ns, nlev, r0.data(), r1.data(), nullptr, 0, CF), MPG_ERR_INVALID_ARG, e, who, "must be 0"));
    EXPECT(refused(call(&csr, m.data(), 2, u.data(), 0, CF, ns - 1, nlev, r0.data(), r1.data(), nullptr, 0, CF), MPG_ERR_INVALID_ARG, e, who, "u_level_stride"));
    EXPECT(refused(call(&csr, m.data(), 2, u.data(), 0, CF, -1, nlev, r0.data(), r1.data(), nullptr, 0, CF), MPG_ERR_INVALID_ARG, e, who, "u_level_stride"));
    EXPECT(refused(call(&csr, m.data(), 2, u.data(), 0, CF, INT64_MAX / 8, nlev, r0.data(), r1.data(), nullptr, 0, CF), MPG_ERR_INVALID_ARG, e, who, "addressed"));
    EXPECT(refused(call(&csr, m.data(), 2, u.data(), 0, LF, 0, nlev, r0.data(), r0.data(), nullptr, 0, CF), MPG_ERR_INVALID_ARG, e, who, "alias each other"));
    EXPECT(refused(call(&csr, m.data(), 3, u.data(), 0, LF, 0, nlev, r0.data(), r1.data(), r0.data() + nlev * nd - 1, 0, CF), MPG_ERR_INVALID_ARG, e, who, "alias each other"));
    EXPECT(refused(call(&csr, m.data(), 3, u.data(), 0, LF, 0, nlev, r0.data(), r1.data(), r1.data() + 1, 0, CF), MPG_ERR_INVALID_ARG, e, who, "alias each other"));
    EXPECT(refused(call(&csr, m.data(), 2, u.data(), 0, LF, 0, nlev, r0.data(), u.data() + nlev * ns - 1, nullptr, 0, CF), MPG_ERR_INVALID_ARG, e, who, "source"));
    EXPECT(refused(call(&csr, m.data(), 3, u.data(), 0, CF, ns + 5, nlev, r0.data(), r1.data(), u.data() + nlev * (ns + 5) - 1, 0, CF), MPG_ERR_INVALID_ARG, e, who, "source"));
    EXPECT(refused(call(&csr, big.data(), 2, u.data(), 0, LF, 0, nlev, big.data() + 2 * nnz - 1, r1.data(), nullptr, 0, CF), MPG_ERR_INVALID_ARG, e, who, "m_dev"));
    EXPECT(refused(call(&csr, big.data(), 3, u.data(), 0, LF, 0, nlev, r0.data(), r1.data(), big.data() + 2 * nnz, 0, CF), MPG_ERR_INVALID_ARG, e, who, "m_dev"));
    // two results read two planes of the values: a result behind them is its own array
    EXPECT(call(&csr, big.data(), 2, u.data(), 0, LF, 0, nlev, big.data() + 2 * nnz, big.data() + 2 * nnz + nlev * nd, nullptr, 0, CF) == MPG_SUCCESS);
    // the edges of the 64-bit range: results that cannot be addressed, and more blocks than one launch holds
    const WrHandle wide = handle(true, 0, 1, INT64_MAX / 16, 4, 1), many = handle(true, 0, 1, (int64_t)64 * 0x7fffffffll + 1, 4, 1),
                   most = handle(true, 0, 1, (int64_t)64 * 0x7fffffffll, 4, 1);
    const void *far0 = (const void *)(uintptr_t)(1ull << 60), *far1 = (const void *)(uintptr_t)(1ull << 61);
    EXPECT(refused(call(&wide, m.data(), 2, u.data(), 0, LF, 0, 3, r0.data(), r1.data(), nullptr, 0, CF), MPG_ERR_INVALID_ARG, e, who, "addressed"));
    EXPECT(refused(call(&many, m.data(), 2, u.data(), 1, LF, 0, 1, far0, far1, nullptr, 1, CF), MPG_ERR_OVERFLOW, e, who, "one launch"));
    EXPECT(call(&most, m.data(), 2, u.data(), 1, LF, 0, 1, far0, far1, nullptr, 1, CF) == MPG_SUCCESS);
  }
  // ---- the LDS in front of the tiles: nout planes of doubles, col, the row pointers; the tiles behind stay 16-byte aligned
  EXPECT(wr_lds_head(2) == 512 * 20 + 68 * 4 && wr_lds_head(3) == 512 * 28 + 68 * 4);
  EXPECT(wr_lds_head(2) % 16 == 0 && wr_lds_head(3) % 16 == 0);
  EXPECT(wr_lds_head(3) + 64 * 1024 <= 80 * 1024);      // two workgroups per CU of 160 KB, whatever the tiles
  EXPECT(wr_lds_head(3) + 3 * 64 * 33 * 8 == 65296);     // 55 levels x 3 float64 results: level chunks of 32
  EXPECT(WR_RP > WR_ROWS && WR_ROWS == 64);
  if (failures) {
    printf("%d check(s) failed\n", failures);
    return 1;
  }
  printf("store: ok\nvalues: ok\napply: ok\nlds: ok\nok\n");
  return 0;
}
