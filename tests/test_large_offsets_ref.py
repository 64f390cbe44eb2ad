"""The reference of the large-offset tests (tests/_large_offsets_ref.py) held to the oracle on the CPU, at a few hundred points: fixed
handles of 1, 3 and 4 entries and a CSR one, both source layouts (a pitched cell-fast source included), both destination orders, with and
without an affine epilogue -- against oracle.apply_fixed / oracle.apply_csr, within the reference's own bar, and against the same sums in
np.longdouble.  compare() must pass on the reference's own values rounded to float32 / float64 and must fail on ONE element read from
a neighbouring source.  The column generator of case A1 is checked at its full sizes (integer arithmetic on 4197 rows)."""
import numpy as np
import pytest

import _large_offsets_ref as LR

N_SRC, N_DST, NLEV = 997, 333, 7


def _weights(kind, rng):
    import torch
    if kind == "csr":
        lens = rng.integers(0, 40, size=N_DST)
        lens[:4] = (0, 1, 39, 0)
        rowptr = np.concatenate([[0], np.cumsum(lens)])
        col = rng.integers(0, N_SRC, size=int(lens.sum())).astype(np.int32)
        val = rng.normal(size=col.size)
        return LR.Weights(torch, N_SRC, N_DST, rowptr=rowptr, col=col, val=val), (rowptr, col, val)
    nnz = int(kind)
    idx = rng.integers(0, N_SRC, size=(N_DST, nnz)).astype(np.int32)
    idx[rng.random(N_DST) < 0.1] = -1                                   # unmapped points
    w = np.ones((N_DST, nnz)) if nnz == 1 else rng.normal(size=(N_DST, nnz))
    return LR.Weights(torch, N_SRC, N_DST, idx=idx, w=w), (idx, w)


def _exact(W, raw, x2d):
    """[nlev][n_dst] in np.longdouble; x2d: [nlev][n_src] float64."""
    out = np.zeros((NLEV, N_DST), np.longdouble)
    if W.kind == "csr":
        rowptr, col, val = raw
        for p in range(N_DST):
            for q in range(rowptr[p], rowptr[p + 1]):
                out[:, p] += np.longdouble(val[q]) * x2d[:, col[q]].astype(np.longdouble)
    else:
        idx, w = raw
        for p in range(N_DST):
            if idx[p, 0] >= 0:
                for q in range(idx.shape[1]):
                    out[:, p] += np.longdouble(w[p, q]) * x2d[:, idx[p, q]].astype(np.longdouble)
    return out


@pytest.mark.parametrize("lev_fast", [False, True])
@pytest.mark.parametrize("kind", ["1", "3", "4", "csr"])
def test_reference_against_the_oracle(oracle, kind, lev_fast):
    import torch
    rng = np.random.default_rng(11 + 2 * len(kind) + int(lev_fast))
    W, raw = _weights(kind, rng)
    x2d = (rng.random((NLEV, N_SRC)) - 0.5) * LR.SPAN                   # [lev][cell]
    flat = np.ascontiguousarray(x2d.T if lev_fast else x2d).reshape(-1)
    want = oracle.apply_csr(*raw, flat, NLEV, lev_fast=lev_fast) if kind == "csr" else oracle.apply_fixed(raw[0], raw[1], flat, NLEV, lev_fast=lev_fast)
    exact = _exact(W, raw, x2d)
    src = torch.as_tensor(flat)
    bar = LR.apply_bar(W).numpy()
    for dst_rows in (False, True):
        ref = LR.apply_ref(W, src, NLEV, lev_fast, dst_rows=dst_rows).numpy()
        ref = ref.T if dst_rows else ref
        assert ref.shape == want.shape == (NLEV, N_DST)
        assert (np.abs(ref - want) <= bar[None, :]).all(), "the reference leaves the oracle's bar"
        assert (np.abs(ref - exact.astype(np.float64)) <= bar[None, :] / 2 + LR.EPS64 * np.abs(ref)).all(), "the reference alone leaves its own bar"
        assert np.array_equal(ref, want) or kind != "1", "a copy is exact"
        # in chunks, the same bits
        parts = [LR.apply_ref(W, src, NLEV, lev_fast, p0=a, p1=min(a + 100, N_DST), dst_rows=dst_rows).numpy() for a in range(0, N_DST, 100)]
        assert np.array_equal(np.concatenate(parts, axis=0 if dst_rows else 1), ref.T if dst_rows else ref)
    unm = np.diff(raw[0]) == 0 if kind == "csr" else raw[0][:, 0] < 0
    assert unm.any() and (want[:, unm] == 0.0).all() and (LR.apply_ref(W, src, NLEV, lev_fast).numpy()[:, unm] == 0.0).all()
    # an affine epilogue: the oracle's values through the same multiply and add
    scale, offset = 9.81, -300.0
    ref = LR.apply_ref(W, src, NLEV, lev_fast, scale=scale, offset=offset).numpy()
    bar = LR.apply_bar(W, scale=scale, offset=offset).numpy()
    assert (np.abs(ref - (want * scale + offset)) <= bar[None, :]).all()
    assert (ref[:, unm] == offset).all()


@pytest.mark.parametrize("kind", ["3", "csr"])
def test_pitched_source_and_compare(kind):
    """A cell-fast source whose planes lie `stride` > n_src apart, results in both orders and both types: compare() passes on the
    reference's own values and fails when ONE element was read one source off."""
    import torch
    rng = np.random.default_rng(5)
    W, raw = _weights(kind, rng)
    stride = N_SRC + 29
    buf = torch.full((NLEV * stride,), float("nan"), dtype=torch.float64)
    x2d = torch.as_tensor((rng.random((NLEV, N_SRC)) - 0.5) * LR.SPAN)
    buf.view(NLEV, stride)[:, :N_SRC] = x2d
    dense = LR.apply_ref(W, x2d.reshape(-1), NLEV, False)
    assert torch.equal(LR.apply_ref(W, buf, NLEV, False, stride=stride), dense)
    assert torch.equal(LR.apply_ref(W, x2d.t().contiguous().reshape(-1), NLEV, True), dense)
    for dt in (torch.float64, torch.float32):
        for dst_rows in (False, True):
            got = (dense.t() if dst_rows else dense).contiguous().to(dt).reshape(-1)
            worst = LR.compare(W, got, buf, NLEV, False, stride=stride, dst_rows=dst_rows, what="self")
            assert worst <= 1.0
            # a pitched result [lev][ld]
            if not dst_rows:
                ld = N_DST + 3
                pit = torch.zeros(NLEV * ld, dtype=dt)
                pit.view(NLEV, ld)[:, :N_DST] = dense.to(dt)
                assert LR.compare(W, pit, buf, NLEV, False, stride=stride, dst_stride=ld, what="pitched") <= 1.0
            # one element read one source off: an error of order 1, far beyond any bar
            p = int(np.flatnonzero(W.n.numpy() > 0)[3])
            wrong = x2d.clone()
            c = int(raw[1][raw[0][p]] if kind == "csr" else raw[0][p, 0])
            wrong[2, c] = x2d[2, (c + 1) % N_SRC]
            bad = LR.apply_ref(W, wrong.reshape(-1), NLEV, False)
            assert int((bad != dense).sum()) >= 1
            got = (bad.t() if dst_rows else bad).contiguous().to(dt).reshape(-1)
            with pytest.raises(AssertionError, match="beyond their bar"):
                LR.compare(W, got, buf, NLEV, False, stride=stride, dst_rows=dst_rows, what="wrong element")
            got = (dense.t() if dst_rows else dense).contiguous().to(dt).reshape(-1).clone()
            got[5] = float("nan")
            with pytest.raises(AssertionError, match="beyond their bar"):
                LR.compare(W, got, buf, NLEV, False, stride=stride, dst_rows=dst_rows, what="unwritten element")


def test_offsets_are_int64():
    import torch
    c = torch.tensor([0, (1 << 31) // 55, (1 << 32) // 55 + 1, 78_199_999], dtype=torch.int64)
    off = LR.src_offsets(torch, c, 55, True, 0, True)
    assert off.dtype == torch.int64 and int(off[-1, -1]) == 78_199_999 * 55 + 54 >= 1 << 32
    off = LR.src_offsets(torch, c, 55, False, 78_200_000, False)
    assert int(off[-1, -1]) == 54 * 78_200_000 + 78_199_999 and int(off[28, 0]) == 28 * 78_200_000 >= 1 << 31
    assert LR.chunk_points(55, 10 ** 9) * 55 * 8 * 6 <= LR.CHUNK_BYTES


def test_a1_column_generator_at_full_size():
    """Case A1's rows: 0 to 1100 entries, a 64-row run far beyond one 1024-entry LDS chunk, and in EVERY non-empty row at least one id
    of each band -- low ids, the rows that straddle element 2^31 and 2^32 of a 55-level file-order source, the last 8 ids."""
    row, col, S, lens = LR.a1_columns()
    n_dst = LR.A1_NX * LR.A1_NY
    assert n_dst == 65 * 64 + 37 and lens.size == n_dst and lens.min() == 0 and lens.max() == 1100
    assert row.dtype == col.dtype == np.int32 and row.size == col.size == S.size == lens.sum()
    assert np.array_equal(np.bincount(row - 1, minlength=n_dst), lens) and (np.diff(row) >= 0).all()
    assert col.min() >= 1 and col.max() == LR.A1_NSRC
    bands = LR.a1_bands()
    t31, t32 = (1 << 31) / LR.A1_NLEV, (1 << 32) / LR.A1_NLEV
    assert bands[1][0] < t31 < bands[1][1] - 1 and bands[2][0] < t32 < bands[2][1] - 1 and bands[3] == (LR.A1_NSRC - 8, LR.A1_NSRC)
    assert all(hi - lo <= 17 for lo, hi in bands[1:])
    c0 = col.astype(np.int64) - 1
    nonempty = np.flatnonzero(lens > 0)
    assert 0 < nonempty.size < n_dst and lens[nonempty].min() >= 4
    for lo, hi in bands:
        hit = np.bincount(row[(c0 >= lo) & (c0 < hi)] - 1, minlength=n_dst)
        assert (hit[nonempty] >= 1).all(), "a row without an id in [%d, %d)" % (lo, hi)
    # elements on both sides of each threshold are read: the band's rows straddle it
    e = c0 * LR.A1_NLEV
    for thr in (1 << 31, 1 << 32):
        assert ((e < thr) & (e + LR.A1_NLEV > thr)).any() and (e >= thr).any() and (e + LR.A1_NLEV <= thr).any()
    assert int(e.max()) + LR.A1_NLEV - 1 == LR.A1_NSRC * LR.A1_NLEV - 1 >= 1 << 32
    # a 64-row run crosses the 1024-entry chunks inside rows and (somewhere) exactly at a row's end
    rp = np.concatenate([[0], np.cumsum(lens)])
    assert (rp[64::64] - rp[:-64:64]).min() > 20 * 1024
    ends_on = [np.isin(np.arange(1024, rp[a + 64] - rp[a], 1024), rp[a + 1:a + 65] - rp[a]).any() for a in range(0, n_dst - 64, 64)]
    assert any(ends_on) and not all(ends_on)
    row2, col2, S2, _ = LR.a1_columns()
    assert np.array_equal(col, col2) and np.array_equal(S, S2)
