// The argument checks of mpg_handle_compose and mpg_compose_weights_dev and the block plan of the composition's symbolic job
// (mpassit_amd/csrc/compose_checks.h, the text mpg_api.hip and k_compose.hip compile) run on the host: every refusal by code and by a
// word of its message, the accepted forms, and the arithmetic at the edges of the 64-bit and int32 ranges.  No check dereferences a
// device array: host buffers stand in for device memory.  Built by tests/test_compose_checks.py with -fsanitize=address,undefined.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../mpassit_amd/csrc/compose_checks.h"

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

static CoHandle handle(bool csr, int64_t n_pole, int64_t ns, int64_t nd, int64_t nnz) {
  CoHandle h;
  h.csr = csr;
  h.n_pole = n_pole;
  h.n_src = ns;
  h.n_dst = nd;
  h.nnz = nnz;
  return h;
}

int main() {
  WvErr e;
  memset(&e, 0, sizeof e);
  // ---- mpg_handle_compose
  {
    const char *who = "mpg_handle_compose";
    void *out = &e;
    const CoHandle a = handle(false, 0, 642, 851, 3 * 851), b = handle(true, 0, 1920, 642, 3840);
    EXPECT(co_check_compose(&a, &b, out, e) == MPG_SUCCESS);
    const CoHandle a2 = handle(true, 0, 642, 851, 0), b2 = handle(false, 0, 1920, 642, 0);   // either kind on either side, no entries
    EXPECT(co_check_compose(&a2, &b2, out, e) == MPG_SUCCESS);
    EXPECT(co_check_compose(&a2, &b, out, e) == MPG_SUCCESS && co_check_compose(&a, &b2, out, e) == MPG_SUCCESS);
    EXPECT(refused(co_check_compose(nullptr, &b, out, e), MPG_ERR_INVALID_ARG, e, who, "NULL"));
    EXPECT(refused(co_check_compose(&a, nullptr, out, e), MPG_ERR_INVALID_ARG, e, who, "NULL"));
    EXPECT(refused(co_check_compose(&a, &b, nullptr, e), MPG_ERR_INVALID_ARG, e, who, "NULL"));
    EXPECT(refused(co_check_compose(nullptr, nullptr, nullptr, e), MPG_ERR_INVALID_ARG, e, who, "NULL"));
    const CoHandle loc = handle(false, 0, 100, 851, 3 * 851);   // a localized outer: a packed source
    EXPECT(refused(co_check_compose(&loc, &b, out, e), MPG_ERR_INVALID_ARG, e, who, "n_dst = 642"));
    EXPECT(strstr(e.msg, "n_src = 100") && strstr(e.msg, "localized"));
    const CoHandle big = handle(true, 0, INT64_MAX, 5, 1), bigb = handle(true, 0, 7, INT64_MAX - 1, 1);
    EXPECT(refused(co_check_compose(&big, &bigb, out, e), MPG_ERR_INVALID_ARG, e, who, "9223372036854775806"));
    const CoHandle pa = handle(false, 4, 642, 851, 3 * 851), pb = handle(true, 1, 1920, 642, 3840);
    EXPECT(refused(co_check_compose(&pa, &b, out, e), MPG_ERR_UNSUPPORTED, e, who, "`outer`"));
    EXPECT(strstr(e.msg, "mpg_handle_pole_count > 0") && strstr(e.msg, "mpg_handle_from_weights"));
    EXPECT(refused(co_check_compose(&a, &pb, out, e), MPG_ERR_UNSUPPORTED, e, who, "`inner`"));
    EXPECT(refused(co_check_compose(&loc, &pb, out, e), MPG_ERR_INVALID_ARG, e, who, "chain"));   // the sizes come first
    printf("compose: ok\n");
  }
  // ---- the block plan and the entry count
  {
    const char *who = "mpg_handle_compose";
    int64_t r1 = -1, nc = -1;
    const std::vector<int64_t> cnt = {5, 0, 7, 100, 0, 0, 3, 2};
    const int64_t n = (int64_t)cnt.size();
    // by the budget: a block closes before the row that would pass the cap; a longer row stands alone
    EXPECT(co_next_block(cnt.data(), n, 0, 12, 0, &r1, &nc, e) == MPG_SUCCESS && r1 == 3 && nc == 12);
    EXPECT(co_next_block(cnt.data(), n, 0, 11, 0, &r1, &nc, e) == MPG_SUCCESS && r1 == 2 && nc == 5);
    EXPECT(co_next_block(cnt.data(), n, 3, 12, 0, &r1, &nc, e) == MPG_SUCCESS && r1 == 4 && nc == 100);
    EXPECT(co_next_block(cnt.data(), n, 4, 12, 0, &r1, &nc, e) == MPG_SUCCESS && r1 == 8 && nc == 5);
    EXPECT(co_next_block(cnt.data(), n, 0, 1, 0, &r1, &nc, e) == MPG_SUCCESS && r1 == 1 && nc == 5);
    EXPECT(co_next_block(cnt.data(), n, 0, 0, 0, &r1, &nc, e) == MPG_SUCCESS && r1 == 1 && nc == 5);   // always one row at least
    EXPECT(co_next_block(cnt.data(), n, 4, 0, 0, &r1, &nc, e) == MPG_SUCCESS && r1 == 5 && nc == 0);
    EXPECT(co_next_block(cnt.data(), n, 0, INT64_MAX, 0, &r1, &nc, e) == MPG_SUCCESS && r1 == n && nc == 117);
    // by rows
    EXPECT(co_next_block(cnt.data(), n, 0, 1000, 1, &r1, &nc, e) == MPG_SUCCESS && r1 == 1 && nc == 5);
    EXPECT(co_next_block(cnt.data(), n, 1, 1000, 7, &r1, &nc, e) == MPG_SUCCESS && r1 == 8 && nc == 112);
    EXPECT(co_next_block(cnt.data(), n, 0, 1000, 7, &r1, &nc, e) == MPG_SUCCESS && r1 == 7 && nc == 115);
    EXPECT(co_next_block(cnt.data(), n, 0, 1000, CO_BLOCK_ROWS_MAX, &r1, &nc, e) == MPG_SUCCESS && r1 == n && nc == 117);
    EXPECT(co_next_block(cnt.data(), n, n, 1000, 0, &r1, &nc, e) == MPG_SUCCESS && r1 == n && nc == 0);   // nothing left
    // every plan covers every row once, whatever the block size
    for (int64_t cap : {0ll, 1ll, 8ll, 12ll, 117ll, 1000ll})
      for (int64_t rows : {0ll, 1ll, 2ll, 7ll, 100ll}) {
        int64_t r0 = 0, total = 0, blocks = 0;
        while (r0 < n) {
          EXPECT(co_next_block(cnt.data(), n, r0, cap, rows, &r1, &nc, e) == MPG_SUCCESS && r1 > r0);
          if (r1 <= r0) break;
          EXPECT(rows == 0 || r1 - r0 <= rows);
          EXPECT(r1 - r0 == 1 || nc <= cap);
          total += nc;
          r0 = r1;
          ++blocks;
        }
        EXPECT(r0 == n && total == 117 && blocks <= n);
      }
    // the edges of int32 and of 64 bits: the candidates are a 64-bit quantity, a block's are not
    const std::vector<int64_t> edge = {CO_MAX_BLOCK_CAND, 1, CO_MAX_BLOCK_CAND - 1, 1, 1};
    EXPECT(co_next_block(edge.data(), 5, 0, INT64_MAX, 0, &r1, &nc, e) == MPG_SUCCESS && r1 == 1 && nc == CO_MAX_BLOCK_CAND);
    EXPECT(co_next_block(edge.data(), 5, 1, INT64_MAX, 0, &r1, &nc, e) == MPG_SUCCESS && r1 == 3 && nc == CO_MAX_BLOCK_CAND);
    EXPECT(co_next_block(edge.data(), 5, 3, INT64_MAX, 0, &r1, &nc, e) == MPG_SUCCESS && r1 == 5 && nc == 2);
    EXPECT(CO_MAX_BLOCK_CAND == 2147483646ll && CO_MAX_NNZ == 2147483646ll && CO_BLOCK_CAND * CO_BYTES_PER_CAND <= CO_BUDGET_BYTES);
    EXPECT(CO_BLOCK_CAND > 0 && CO_BLOCK_CAND <= CO_MAX_BLOCK_CAND && CO_LDS_ROW_ENTRIES >= 0);
    const std::vector<int64_t> over = {1, CO_MAX_BLOCK_CAND + 1};
    EXPECT(co_next_block(over.data(), 2, 0, 100, 1, &r1, &nc, e) == MPG_SUCCESS && r1 == 1 && nc == 1);
    EXPECT(refused(co_next_block(over.data(), 2, 0, 100, 0, &r1, &nc, e), MPG_ERR_OVERFLOW, e, who, "row 1"));   // as soon as the plan meets it
    EXPECT(refused(co_next_block(over.data(), 2, 1, 100, 0, &r1, &nc, e), MPG_ERR_OVERFLOW, e, who, "row 1"));
    EXPECT(strstr(e.msg, "2147483647") && strstr(e.msg, "split"));
    const std::vector<int64_t> huge = {INT64_MAX, INT64_MAX}, neg = {-1};
    EXPECT(refused(co_next_block(huge.data(), 2, 0, INT64_MAX, 0, &r1, &nc, e), MPG_ERR_OVERFLOW, e, who, "9223372036854775807"));
    EXPECT(refused(co_next_block(neg.data(), 1, 0, 100, 0, &r1, &nc, e), MPG_ERR_OVERFLOW, e, who, "row 0"));
    // a total far beyond int32 is planned without a wrap: 2^33 rows' worth in blocks of 2^31 - 2
    const std::vector<int64_t> many(8, 0x40000000ll);   // 8 x 2^30 = 2^33 candidates
    int64_t r0 = 0, total = 0, blocks = 0;
    while (r0 < 8) {
      EXPECT(co_next_block(many.data(), 8, r0, INT64_MAX, 0, &r1, &nc, e) == MPG_SUCCESS && nc <= CO_MAX_BLOCK_CAND && r1 > r0);
      if (r1 <= r0) break;
      total += nc;
      r0 = r1;
      ++blocks;
    }
    EXPECT(total == 0x200000000ll && blocks == 8);
    // the entries after de-duplication
    EXPECT(co_check_nnz(0, e) == MPG_SUCCESS && co_check_nnz(CO_MAX_NNZ, e) == MPG_SUCCESS);
    EXPECT(refused(co_check_nnz(CO_MAX_NNZ + 1, e), MPG_ERR_OVERFLOW, e, who, "2^31 - 2"));
    EXPECT(strstr(e.msg, "2147483647") && strstr(e.msg, "int32"));
    EXPECT(refused(co_check_nnz(INT64_MAX, e), MPG_ERR_OVERFLOW, e, who, "9223372036854775807"));
    EXPECT(refused(co_check_nnz(-1, e), MPG_ERR_OVERFLOW, e, who, nullptr));
    printf("blocks: ok\n");
  }
  // ---- mpg_compose_weights_dev
  {
    const char *who = "mpg_compose_weights";
    std::vector<double> buf(64);
    double *bm = buf.data(), *m = buf.data() + 32;
    bool nothing = true;
    const CoHandle c = handle(true, 0, 1920, 851, 4), a = handle(false, 0, 642, 851, 3 * 851), b = handle(true, 0, 1920, 642, 4);
    for (int k = 1; k <= CO_MAX_PLANES; ++k) EXPECT(co_check_weights(&c, &a, &b, k, bm, m, &nothing, e) == MPG_SUCCESS && !nothing);
    const CoHandle acsr = handle(true, 0, 642, 851, 9);
    EXPECT(co_check_weights(&c, &acsr, &b, 2, bm, m, &nothing, e) == MPG_SUCCESS && !nothing);
    const CoHandle c0 = handle(true, 0, 1920, 851, 0);   // no entries: nothing to write, no array needed
    EXPECT(co_check_weights(&c0, &a, &b, 1, nullptr, nullptr, &nothing, e) == MPG_SUCCESS && nothing);
    const CoHandle b0 = handle(true, 0, 1920, 642, 0);   // an inner without entries has no planes to give
    EXPECT(co_check_weights(&c, &a, &b0, 1, nullptr, m, &nothing, e) == MPG_SUCCESS && !nothing);
    EXPECT(refused(co_check_weights(nullptr, &a, &b, 1, bm, m, &nothing, e), MPG_ERR_INVALID_ARG, e, who, "NULL handle"));
    EXPECT(refused(co_check_weights(&c, nullptr, &b, 1, bm, m, &nothing, e), MPG_ERR_INVALID_ARG, e, who, "NULL handle"));
    EXPECT(refused(co_check_weights(&c, &a, nullptr, 1, bm, m, &nothing, e), MPG_ERR_INVALID_ARG, e, who, "NULL handle"));
    EXPECT(refused(co_check_weights(nullptr, nullptr, nullptr, 0, nullptr, nullptr, &nothing, e), MPG_ERR_INVALID_ARG, e, who, "NULL"));
    EXPECT(refused(co_check_weights(&c, &a, &b, 1, nullptr, m, &nothing, e), MPG_ERR_INVALID_ARG, e, who, "NULL array"));
    EXPECT(refused(co_check_weights(&c, &a, &b, 1, bm, nullptr, &nothing, e), MPG_ERR_INVALID_ARG, e, who, "NULL array"));
    for (int k : {0, -1, 5, INT32_MAX, INT32_MIN}) EXPECT(refused(co_check_weights(&c, &a, &b, k, bm, m, &nothing, e), MPG_ERR_INVALID_ARG, e, who, "1..4"));
    const CoHandle bfix = handle(false, 0, 1920, 642, 4 * 642), cfix = handle(false, 0, 1920, 851, 3 * 851);
    EXPECT(refused(co_check_weights(&c, &a, &bfix, 1, bm, m, &nothing, e), MPG_ERR_UNSUPPORTED, e, who, "`inner` is a fixed"));
    EXPECT(strstr(e.msg, "mpg_handle_get_weights") && strstr(e.msg, "mpg_handle_from_weights"));
    EXPECT(refused(co_check_weights(&cfix, &a, &b, 1, bm, m, &nothing, e), MPG_ERR_UNSUPPORTED, e, who, "`composed` is a fixed"));
    const CoHandle cp = handle(true, 2, 1920, 851, 4), ap = handle(false, 2, 642, 851, 3 * 851), bp = handle(true, 2, 1920, 642, 4);
    EXPECT(refused(co_check_weights(&cp, &a, &b, 1, bm, m, &nothing, e), MPG_ERR_UNSUPPORTED, e, who, "`composed` has pole-cap"));
    EXPECT(refused(co_check_weights(&c, &ap, &b, 1, bm, m, &nothing, e), MPG_ERR_UNSUPPORTED, e, who, "`outer` has pole-cap"));
    EXPECT(refused(co_check_weights(&c, &a, &bp, 1, bm, m, &nothing, e), MPG_ERR_UNSUPPORTED, e, who, "`inner` has pole-cap"));
    const CoHandle cd = handle(true, 0, 1920, 850, 4), cs = handle(true, 0, 1921, 851, 4), ab = handle(false, 0, 643, 851, 3 * 851);
    EXPECT(refused(co_check_weights(&cd, &a, &b, 1, bm, m, &nothing, e), MPG_ERR_INVALID_ARG, e, who, "composed is 850 x 1920"));
    EXPECT(refused(co_check_weights(&cs, &a, &b, 1, bm, m, &nothing, e), MPG_ERR_INVALID_ARG, e, who, "composed is 851 x 1921"));
    EXPECT(refused(co_check_weights(&c, &ab, &b, 1, bm, m, &nothing, e), MPG_ERR_INVALID_ARG, e, who, "outer 851 x 643"));
    // aliasing: 4 entries on either side, K planes of 32 bytes each
    EXPECT(refused(co_check_weights(&c, &a, &b, 1, bm, bm, &nothing, e), MPG_ERR_INVALID_ARG, e, who, "alias"));
    EXPECT(refused(co_check_weights(&c, &a, &b, 2, bm, bm + 7, &nothing, e), MPG_ERR_INVALID_ARG, e, who, "alias"));
    EXPECT(co_check_weights(&c, &a, &b, 2, bm, bm + 8, &nothing, e) == MPG_SUCCESS);
    EXPECT(refused(co_check_weights(&c, &a, &b, 2, bm + 7, bm, &nothing, e), MPG_ERR_INVALID_ARG, e, who, "alias"));
    EXPECT(co_check_weights(&c, &a, &b, 1, bm, bm + 4, &nothing, e) == MPG_SUCCESS);
    // the largest handles: the byte counts are formed in uintptr_t and never read
    const CoHandle cbig = handle(true, 0, CO_MAX_NNZ, CO_MAX_NNZ, CO_MAX_NNZ), abig = handle(true, 0, CO_MAX_NNZ, CO_MAX_NNZ, CO_MAX_NNZ);
    const uintptr_t lo = 0x10000, planes = 4 * (uintptr_t)CO_MAX_NNZ * sizeof(double);
    EXPECT(co_check_weights(&cbig, &abig, &abig, 4, (const double *)lo, (double *)(lo + planes), &nothing, e) == MPG_SUCCESS && !nothing);
    EXPECT(refused(co_check_weights(&cbig, &abig, &abig, 4, (const double *)lo, (double *)(lo + planes - 8), &nothing, e), MPG_ERR_INVALID_ARG, e, who, "alias"));
    EXPECT(refused(co_check_weights(&cbig, &abig, &abig, 4, (const double *)(lo + planes - 8), (double *)lo, &nothing, e), MPG_ERR_INVALID_ARG, e, who, "alias"));
    printf("planes: ok\n");
  }
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
