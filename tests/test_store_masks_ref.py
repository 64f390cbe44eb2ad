"""The numpy mirrors of the Store-time mask calls (target_grid.mask_rows, target_grid.extrapolate_rows_masked) on small synthetic patterns,
against plain per-row Python loops written from the sentences of include/mpassit_amd.h; zero masks reproduce the inputs and
target_grid.extrapolate_rows bit for bit."""
import numpy as np
import pytest

from mpassit_amd import target_grid as tg


def _pattern(seed, n=57, n_src=23):
    """A CSR pattern with empty rows, rows of one entry, duplicate columns, zero and negative values, and a dst_frac."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 7, n)
    lens[::9] = 0
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = rng.integers(0, n_src, rowptr[-1]).astype(np.int32)
    val = rng.integers(-2, 40, rowptr[-1]) / 64.0 + rng.random(rowptr[-1]) * (rng.random(rowptr[-1]) < 0.5)
    frac = rng.random(n)
    return rowptr, col, val, frac, n_src


def _loop(rowptr, col, val, frac, sm, dm, rule, norm):
    """The header's sentences, one row at a time."""
    n = rowptr.size - 1
    out_rows, fout, stats = [], [], [0, 0, 0]
    for i in range(n):
        ent = [(int(col[q]), float(val[q])) for q in range(rowptr[i], rowptr[i + 1])]
        f = None if frac is None else float(frac[i])
        if dm is not None and dm[i]:
            new, f2 = [], 0.0
            stats[1] += len(ent) > 0
        elif rule == tg.MASKRULE_ROW:
            hit = sm is not None and any(sm[c] for c, _ in ent)
            new, f2 = ([], 0.0) if hit else (ent, f)
            stats[0] += hit
        else:
            kept = [(c, v) for c, v in ent if sm is None or not sm[c]]
            if len(kept) == len(ent):
                new, f2 = ent, f
            else:
                Wk = np.float64(0.0)
                for _, v in kept:
                    Wk = Wk + np.float64(v)
                if not kept or not Wk > 0.0:
                    new, f2 = [], 0.0
                    stats[0] += 1
                elif norm == tg.NORM_DSTAREA:
                    new, f2 = kept, float(Wk)
                else:
                    new, f2 = [(c, float(np.float64(v) / Wk)) for c, v in kept], (0.0 if f is None else float(np.float64(f) * Wk))
        stats[2] += len(ent) - len(new)
        out_rows.append(new)
        fout.append(f2)
    rp = np.concatenate([[0], np.cumsum([len(r) for r in out_rows])]).astype(np.int64)
    c = np.array([c for r in out_rows for c, _ in r], np.int32)
    v = np.array([v for r in out_rows for _, v in r], np.float64)
    return rp, c, v, (None if frac is None else np.array(fout, np.float64)), stats


def _same(a, b):
    assert a[0].tolist() == b[0].tolist()
    assert a[1].tolist() == b[1].tolist()
    assert a[2].tobytes() == b[2].tobytes()
    assert (a[3] is None) == (b[3] is None)
    if a[3] is not None:
        assert a[3].tobytes() == b[3].tobytes()
    assert list(a[4]) == list(b[4])


@pytest.mark.parametrize("rule,norm", [(tg.MASKRULE_ROW, tg.NORM_DSTAREA), (tg.MASKRULE_ENTRY, tg.NORM_DSTAREA), (tg.MASKRULE_ENTRY, tg.NORM_FRACAREA)])
@pytest.mark.parametrize("with_frac", [True, False])
def test_mask_rows_against_the_row_loop(rule, norm, with_frac):
    seen = set()
    for seed in range(6):
        rowptr, col, val, frac, n_src = _pattern(seed)
        frac = frac if with_frac else None
        rng = np.random.default_rng(100 + seed)
        for sm, dm in ((rng.random(n_src) < 0.3, rng.random(rowptr.size - 1) < 0.2), (rng.random(n_src) < 0.8, None), (None, rng.random(rowptr.size - 1) < 0.5),
                       (np.ones(n_src, bool), None), (np.zeros(n_src, np.uint8), np.zeros(rowptr.size - 1, np.uint8))):
            got = tg.mask_rows(rowptr, col, val, frac, sm, dm, rule, norm)
            want = _loop(rowptr, col, val, frac, sm, dm, rule, norm)
            _same(got, want)
            had, now = np.diff(rowptr), np.diff(got[0])
            seen |= {"untouched"} if ((now == had) & (had > 0)).any() else set()
            seen |= {"emptied"} if ((now == 0) & (had > 0)).any() else set()
            seen |= {"partly"} if ((now > 0) & (now < had)).any() else set()
    assert {"untouched", "emptied"} <= seen and (("partly" in seen) == (rule == tg.MASKRULE_ENTRY))


def test_mask_rows_without_masks_returns_the_input():
    rowptr, col, val, frac, _ = _pattern(3)
    for rule in (tg.MASKRULE_ROW, tg.MASKRULE_ENTRY):
        for norm in (tg.NORM_DSTAREA, tg.NORM_FRACAREA):
            rp, c, v, f, stats = tg.mask_rows(rowptr, col, val, frac, None, None, rule, norm)
            assert rp.tolist() == rowptr.tolist() and c.tolist() == col.tolist() and v.tobytes() == val.tobytes() and f.tobytes() == frac.tobytes()
            assert stats == [0, 0, 0]
    with pytest.raises(ValueError):
        tg.mask_rows(rowptr, col, val, frac, None, None, 0)


def test_a_row_whose_kept_sum_is_not_positive_is_emptied():
    rowptr = np.array([0, 3, 6, 8])
    col = np.array([0, 1, 2, 0, 1, 2, 1, 2], np.int32)
    val = np.array([0.5, 0.25, -0.25, 0.5, 0.25, 0.25, 0.0, 1.0])
    sm = np.array([1, 0, 0], np.uint8)          # source 0 masked: row 0 keeps 0.25 - 0.25 = 0, row 1 keeps 0.5, row 2 is untouched
    for norm in (tg.NORM_DSTAREA, tg.NORM_FRACAREA):
        rp, c, v, f, stats = tg.mask_rows(rowptr, col, val, np.array([1.0, 0.5, 0.25]), sm, None, tg.MASKRULE_ENTRY, norm)
        assert rp.tolist() == [0, 0, 2, 4] and c.tolist() == [1, 2, 1, 2] and stats == [1, 0, 4]
        assert v.tolist() == ([0.25, 0.25, 0.0, 1.0] if norm == tg.NORM_DSTAREA else [0.5, 0.5, 0.0, 1.0])
        assert f.tolist() == ([0.0, 0.5, 0.25] if norm == tg.NORM_DSTAREA else [0.0, 0.25, 0.25]) and not np.signbit(f[0])


def _points(seed, n):
    rng = np.random.default_rng(seed)
    p = rng.integers(-4, 5, (3, n)) / 8.0 + 0.01 * rng.integers(0, 2, (3, n))     # a coarse lattice: equal distances, coincident points
    return p


@pytest.mark.parametrize("method,N,e", [(tg.EXTRAPMETHOD_NEAREST_STOD, 1, 2.0), (tg.EXTRAPMETHOD_NEAREST_IDAVG, 1, 2.0), (tg.EXTRAPMETHOD_NEAREST_IDAVG, 3, 2.0),
                                        (tg.EXTRAPMETHOD_NEAREST_IDAVG, 8, 2.0), (tg.EXTRAPMETHOD_NEAREST_IDAVG, 4, 3.5)])
def test_extrapolate_rows_masked_against_the_row_loop(method, N, e):
    src, dst = _points(1, 41), _points(2, 29)
    dst[:, :5] = src[:, :5]                                   # coincident with a source (masked or not)
    rows = np.arange(0, 29, 2)
    rng = np.random.default_rng(7)
    for mask in (rng.random(41) < 0.3, rng.random(41) < 0.9, np.arange(41) < 38, np.ones(41, bool), np.zeros(41, np.uint8)):
        rowlen, ids, w = tg.extrapolate_rows_masked(src, dst, rows, mask, method, N, e)
        live = [c for c in range(41) if not mask[c]]
        K = min(N if method == tg.EXTRAPMETHOD_NEAREST_IDAVG else 1, len(live))
        assert ids.shape == (rows.size, K) and w.shape == (rows.size, K)
        for u, p in enumerate(rows):
            d = dst[:, p][:, None] - src[:, live]
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            order = sorted(range(len(live)), key=lambda k: (d2[k], live[k]))[:K]
            if K == 0:
                assert rowlen[u] == 0
                continue
            one = method == tg.EXTRAPMETHOD_NEAREST_STOD or K == 1 or d2[order[0]] == 0.0
            k = 1 if one else K
            assert rowlen[u] == k and ids[u, :k].tolist() == [live[o] for o in order[:k]] and (ids[u, k:] == -1).all() and (w[u, k:] == 0.0).all()
            if one:
                assert w[u, 0] == 1.0
            else:
                t = [d2[order[0]] / d2[o] if e == 2.0 else np.power(d2[order[0]] / d2[o], 0.5 * e) for o in order]
                S = t[0]
                for x in t[1:]:
                    S = S + x
                assert w[u].tolist() == [x / S for x in t]
        assert not mask[ids[ids >= 0]].any()


def test_zero_masks_reproduce_extrapolate_rows():
    src, dst = _points(3, 37), _points(4, 31)
    rows = np.arange(31) % 3 == 0
    for method, N, e in ((tg.EXTRAPMETHOD_NEAREST_STOD, 8, 2.0), (tg.EXTRAPMETHOD_NEAREST_IDAVG, 4, 2.0), (tg.EXTRAPMETHOD_NEAREST_IDAVG, 8, 3.5)):
        want = tg.extrapolate_rows(src, dst, rows, method, N, e)
        for mask in (None, np.zeros(37, bool), np.zeros(37, np.uint8)):
            got = tg.extrapolate_rows_masked(src, dst, rows, mask, method, N, e)
            for a, b in zip(got, want):
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
