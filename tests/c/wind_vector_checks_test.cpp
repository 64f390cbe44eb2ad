// The argument checks of the three vector-wind calls (mpassit_amd/csrc/wind_vector_checks.h, the text mpg_api.hip compiles) run on the
// host: every refusal by code and by a word of its message, the accepted forms, the arithmetic at the edges of the 64-bit range, and
// the LDS bytes in front of the kernel's tiles.  The checks never dereference an array: host buffers stand in for device memory.
// Built by tests/test_wind_vector_checks.py with -fsanitize=address,undefined.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../mpassit_amd/csrc/wind_vector_checks.h"

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

int main() {
  WvErr e;
  memset(&e, 0, sizeof e);
  // ---- frames
  {
    const char *who = "mpg_sphere_frames";
    std::vector<double> lon(16), lat(16), c(16), s(16), fr(6 * 16);
    EXPECT(wv_check_frames(16, lon.data(), lat.data(), nullptr, nullptr, fr.data(), e) == MPG_SUCCESS);
    EXPECT(wv_check_frames(16, lon.data(), lat.data(), c.data(), s.data(), fr.data(), e) == MPG_SUCCESS);
    EXPECT(wv_check_frames(0, lon.data(), lat.data(), nullptr, nullptr, fr.data(), e) == MPG_SUCCESS);
    EXPECT(refused(wv_check_frames(0, nullptr, nullptr, nullptr, nullptr, nullptr, e), MPG_ERR_INVALID_ARG, e, who, "NULL"));   // before n == 0
    EXPECT(refused(wv_check_frames(16, nullptr, lat.data(), nullptr, nullptr, fr.data(), e), MPG_ERR_INVALID_ARG, e, who, "NULL"));
    EXPECT(refused(wv_check_frames(16, lon.data(), nullptr, nullptr, nullptr, fr.data(), e), MPG_ERR_INVALID_ARG, e, who, "NULL"));
    EXPECT(refused(wv_check_frames(16, lon.data(), lat.data(), nullptr, nullptr, nullptr, e), MPG_ERR_INVALID_ARG, e, who, "NULL"));
    EXPECT(refused(wv_check_frames(16, lon.data(), lat.data(), c.data(), nullptr, fr.data(), e), MPG_ERR_INVALID_ARG, e, who, "come together"));
    EXPECT(refused(wv_check_frames(16, lon.data(), lat.data(), nullptr, s.data(), fr.data(), e), MPG_ERR_INVALID_ARG, e, who, "come together"));
    EXPECT(refused(wv_check_frames(-1, lon.data(), lat.data(), nullptr, nullptr, fr.data(), e), MPG_ERR_INVALID_ARG, e, who, "n must be"));
    EXPECT(refused(wv_check_frames(INT64_MAX / 8, lon.data(), lat.data(), nullptr, nullptr, fr.data(), e), MPG_ERR_INVALID_ARG, e, who, "addressed"));
    EXPECT(refused(wv_check_frames(16, fr.data() + 1, lat.data(), nullptr, nullptr, fr.data(), e), MPG_ERR_INVALID_ARG, e, who, "alias"));
    EXPECT(refused(wv_check_frames(16, lon.data(), lat.data(), c.data(), fr.data() + 5 * 16 + 15, fr.data(), e), MPG_ERR_INVALID_ARG, e, who, "alias"));
    EXPECT(wv_check_frames(15, lon.data(), lat.data(), nullptr, nullptr, fr.data() + 6, e) == MPG_SUCCESS);
  }
  const int64_t ns = 288, nd = 1000, nnz = 4000;
  const WvHandle csr{true, 0, ns, nd, nnz}, fixed{false, 0, ns, nd, 0}, pole{false, 7, ns, nd, 0}, csr_pole{true, 7, ns, nd, nnz}, none{true, 0, ns, nd, 0};
  // ---- blocks
  {
    const char *who = "mpg_wind_vector_weights";
    std::vector<double> sf(6 * ns), df(6 * nd), m(4 * nnz);
    bool nothing = true;
    EXPECT(wv_check_weights(&csr, sf.data(), df.data(), m.data(), &nothing, e) == MPG_SUCCESS && !nothing);
    EXPECT(wv_check_weights(&none, nullptr, nullptr, nullptr, &nothing, e) == MPG_SUCCESS && nothing);      // no entries: writes nothing
    EXPECT(refused(wv_check_weights(nullptr, sf.data(), df.data(), m.data(), &nothing, e), MPG_ERR_INVALID_ARG, e, who, "NULL handle"));
    EXPECT(refused(wv_check_weights(&fixed, sf.data(), df.data(), m.data(), &nothing, e), MPG_ERR_UNSUPPORTED, e, who, "mpg_handle_from_weights"));
    EXPECT(refused(wv_check_weights(&pole, sf.data(), df.data(), m.data(), &nothing, e), MPG_ERR_UNSUPPORTED, e, who, "pole"));
    EXPECT(refused(wv_check_weights(&csr_pole, sf.data(), df.data(), m.data(), &nothing, e), MPG_ERR_UNSUPPORTED, e, who, "mpg_handle_pole_count"));
    EXPECT(refused(wv_check_weights(&csr, nullptr, df.data(), m.data(), &nothing, e), MPG_ERR_INVALID_ARG, e, who, "NULL array"));
    EXPECT(refused(wv_check_weights(&csr, sf.data(), nullptr, m.data(), &nothing, e), MPG_ERR_INVALID_ARG, e, who, "NULL array"));
    EXPECT(refused(wv_check_weights(&csr, sf.data(), df.data(), nullptr, &nothing, e), MPG_ERR_INVALID_ARG, e, who, "NULL array"));
    EXPECT(refused(wv_check_weights(&csr, sf.data(), df.data(), df.data() + 6 * nd - 1, &nothing, e), MPG_ERR_INVALID_ARG, e, who, "alias"));
    EXPECT(refused(wv_check_weights(&csr, m.data() + 4 * nnz - 1, df.data(), m.data(), &nothing, e), MPG_ERR_INVALID_ARG, e, who, "alias"));
  }
  // ---- the apply
  {
    const char *who = "mpg_wind_vector";
    const int nlev = 3;
    std::vector<double> m(4 * nnz), u(nlev * (ns + 5)), v(nlev * (ns + 5)), r0(nlev * nd), r1(nlev * nd), big(4 * nnz + 2 * nlev * nd);
    int64_t ldu = -1, ldv = -1;
    auto call = [&](const WvHandle *h, const double *mm, const void *uu, const void *vv, int st, int64_t lu, int64_t lv, int nl, const void *a, const void *b,
                    int dt, int lay) { return wv_check_apply(h, mm, uu, vv, st, lu, lv, nl, a, b, dt, lay, &ldu, &ldv, e); };
    EXPECT(call(&csr, m.data(), u.data(), v.data(), 0, 0, 0, nlev, r0.data(), r1.data(), 0, 1) == MPG_SUCCESS && ldu == ns && ldv == ns);
    EXPECT(call(&csr, m.data(), u.data(), v.data(), 0, ns, ns + 5, nlev, r0.data(), r1.data(), 1, 0) == MPG_SUCCESS && ldu == ns && ldv == ns + 5);
    EXPECT(call(&csr, m.data(), u.data(), v.data(), 1, 0, 0, nlev, r0.data(), nullptr, 1, 0) == MPG_SUCCESS);                  // r1 may be NULL
    EXPECT(call(&none, nullptr, u.data(), v.data(), 0, 0, 0, nlev, r0.data(), r1.data(), 0, 0) == MPG_SUCCESS);                // no entries: no blocks
    EXPECT(call(&csr, m.data(), u.data(), u.data(), 0, 0, 0, nlev, r0.data(), r1.data(), 0, 0) == MPG_SUCCESS);                // sources may coincide
    EXPECT(refused(call(nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, nullptr, nullptr, 0, 0), MPG_ERR_INVALID_ARG, e, who, "NULL handle"));
    EXPECT(refused(call(&fixed, m.data(), u.data(), v.data(), 0, 0, 0, nlev, r0.data(), r1.data(), 0, 0), MPG_ERR_UNSUPPORTED, e, who, "mpg_handle_get_weights"));
    EXPECT(refused(call(&pole, m.data(), u.data(), v.data(), 0, 0, 0, nlev, r0.data(), r1.data(), 0, 0), MPG_ERR_UNSUPPORTED, e, who, "pole"));
    EXPECT(refused(call(&csr, m.data(), u.data(), v.data(), 2, 0, 0, nlev, r0.data(), r1.data(), 0, 0), MPG_ERR_UNSUPPORTED, e, who, "big-endian"));
    EXPECT(refused(call(&csr, m.data(), u.data(), v.data(), 0, 0, 0, nlev, r0.data(), r1.data(), 3, 0), MPG_ERR_UNSUPPORTED, e, who, "big-endian"));
    EXPECT(refused(call(&csr, nullptr, u.data(), v.data(), 0, 0, 0, nlev, r0.data(), r1.data(), 0, 0), MPG_ERR_INVALID_ARG, e, who, "NULL array"));
    EXPECT(refused(call(&csr, m.data(), nullptr, v.data(), 0, 0, 0, nlev, r0.data(), r1.data(), 0, 0), MPG_ERR_INVALID_ARG, e, who, "NULL array"));
    EXPECT(refused(call(&csr, m.data(), u.data(), nullptr, 0, 0, 0, nlev, r0.data(), r1.data(), 0, 0), MPG_ERR_INVALID_ARG, e, who, "NULL array"));
    EXPECT(refused(call(&csr, m.data(), u.data(), v.data(), 0, 0, 0, nlev, nullptr, r1.data(), 0, 0), MPG_ERR_INVALID_ARG, e, who, "NULL array"));
    EXPECT(refused(call(&csr, m.data(), u.data(), v.data(), 0, 0, 0, 0, r0.data(), r1.data(), 0, 0), MPG_ERR_INVALID_ARG, e, who, "nlev"));
    EXPECT(refused(call(&csr, m.data(), u.data(), v.data(), 0, 0, 0, -4, r0.data(), r1.data(), 0, 0), MPG_ERR_INVALID_ARG, e, who, "nlev"));
    EXPECT(refused(call(&csr, m.data(), u.data(), v.data(), 0, 0, 0, nlev, r0.data(), r1.data(), 0, 2), MPG_ERR_INVALID_ARG, e, who, "dst_layout"));
    EXPECT(refused(call(&csr, m.data(), u.data(), v.data(), 4, 0, 0, nlev, r0.data(), r1.data(), 0, 0), MPG_ERR_INVALID_ARG, e, who, "src_type"));
    EXPECT(refused(call(&csr, m.data(), u.data(), v.data(), 0, 0, 0, nlev, r0.data(), r1.data(), -1, 0), MPG_ERR_INVALID_ARG, e, who, "dst_type"));
    EXPECT(refused(call(&csr, m.data(), u.data(), v.data(), 0, ns - 1, 0, nlev, r0.data(), r1.data(), 0, 0), MPG_ERR_INVALID_ARG, e, who, "u_level_stride"));
    EXPECT(refused(call(&csr, m.data(), u.data(), v.data(), 0, 0, ns - 1, nlev, r0.data(), r1.data(), 0, 0), MPG_ERR_INVALID_ARG, e, who, "v_level_stride"));
    EXPECT(refused(call(&csr, m.data(), u.data(), v.data(), 0, -1, 0, nlev, r0.data(), r1.data(), 0, 0), MPG_ERR_INVALID_ARG, e, who, "u_level_stride"));
    EXPECT(refused(call(&csr, m.data(), u.data(), v.data(), 0, INT64_MAX / 8, 0, nlev, r0.data(), r1.data(), 0, 0), MPG_ERR_INVALID_ARG, e, who, "addressed"));
    EXPECT(refused(call(&csr, m.data(), u.data(), v.data(), 0, 0, 0, nlev, r0.data(), r0.data(), 0, 0), MPG_ERR_INVALID_ARG, e, who, "r0_dev and r1_dev"));
    EXPECT(refused(call(&csr, m.data(), u.data(), v.data(), 0, 0, 0, nlev, r0.data(), r0.data() + nlev * nd - 1, 0, 0), MPG_ERR_INVALID_ARG, e, who, "alias"));
    EXPECT(refused(call(&csr, m.data(), u.data(), v.data(), 0, 0, 0, 1, u.data() + ns - 1, r1.data(), 0, 0), MPG_ERR_INVALID_ARG, e, who, "source"));
    EXPECT(refused(call(&csr, m.data(), u.data(), v.data(), 0, 0, 0, nlev, r0.data(), v.data(), 0, 0), MPG_ERR_INVALID_ARG, e, who, "source"));
    EXPECT(refused(call(&csr, big.data(), u.data(), v.data(), 0, 0, 0, nlev, big.data() + 4 * nnz - 1, r1.data(), 0, 0), MPG_ERR_INVALID_ARG, e, who, "m_dev"));
    EXPECT(refused(call(&csr, big.data(), u.data(), v.data(), 0, 0, 0, nlev, r0.data(), big.data() + 3 * nnz, 0, 0), MPG_ERR_INVALID_ARG, e, who, "m_dev"));
    // r0 alone reads two planes of the blocks: a result behind them is its own array
    EXPECT(call(&csr, big.data(), u.data(), v.data(), 0, 0, 0, nlev, big.data() + 2 * nnz, nullptr, 0, 0) == MPG_SUCCESS);
    EXPECT(call(&csr, big.data(), u.data(), v.data(), 0, 0, 0, nlev, big.data() + 4 * nnz, big.data() + 4 * nnz + nlev * nd, 0, 0) == MPG_SUCCESS);
    // the edges of the 64-bit range: results that cannot be addressed, and more blocks than one launch holds
    const WvHandle wide{true, 0, 1, INT64_MAX / 16, 4}, many{true, 0, 1, (int64_t)64 * 0x7fffffffll + 1, 4}, most{true, 0, 1, (int64_t)64 * 0x7fffffffll, 4};
    EXPECT(refused(call(&wide, m.data(), u.data(), v.data(), 0, 0, 0, 3, r0.data(), nullptr, 0, 0), MPG_ERR_INVALID_ARG, e, who, "addressed"));
    EXPECT(refused(call(&many, m.data(), u.data(), v.data(), 1, 0, 0, 1, r0.data(), nullptr, 1, 0), MPG_ERR_OVERFLOW, e, who, "one launch"));
    EXPECT(call(&most, m.data(), u.data(), v.data(), 1, 0, 0, 1, (const void *)(uintptr_t)(1ull << 60), nullptr, 1, 0) == MPG_SUCCESS);
  }
  // ---- the LDS in front of the tiles: 2 nout planes of doubles, col, the row pointers; the tiles behind stay 16-byte aligned
  EXPECT(wv_lds_head(1) == 384 * 20 + 68 * 4 && wv_lds_head(2) == 384 * 36 + 68 * 4);
  EXPECT(wv_lds_head(1) % 16 == 0 && wv_lds_head(2) % 16 == 0);
  EXPECT(wv_lds_head(2) + 64 * 1024 <= 80 * 1024);      // two workgroups per CU of 160 KB, whatever the tiles
  EXPECT(WV_RP > WV_ROWS && WV_CHUNK % 2 == 0);
  if (failures) {
    printf("%d check(s) failed\n", failures);
    return 1;
  }
  printf("frames: ok\nblocks: ok\napply: ok\nlds: ok\nok\n");
  return 0;
}
