"""The numpy mirror of the nearest-destination-to-source Store (target_grid.nearest_dtos_rows) against an independent restatement: a plain
Python loop over sources and destinations that keeps the smallest (d2, id) pair and then bins.  No GPU.  Every result is discrete or one
rounded division, so every comparison is exact.  Sets of at most 200 x 60 points."""
from fractions import Fraction

import numpy as np
import pytest

from mpassit_amd import target_grid as tg


def _unit(lat, lon):
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    return np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)])


def _loop(src, dst, norm, src_mask=None, dst_mask=None):
    """the rule of include/mpassit_amd.h, one scalar at a time"""
    n_src, n_dst = src.shape[1], dst.shape[1]
    nearest = [-1] * n_src
    for s in range(n_src):
        if src_mask is not None and src_mask[s]:
            continue
        best = None
        for d in range(n_dst):
            if dst_mask is not None and dst_mask[d]:
                continue
            dx, dy, dz = float(src[0, s]) - float(dst[0, d]), float(src[1, s]) - float(dst[1, d]), float(src[2, s]) - float(dst[2, d])
            d2 = (dx * dx + dy * dy) + dz * dz
            if best is None or (d2, d) < best:
                best = (d2, d)
        if best is not None:
            nearest[s] = best[1]
    rows = [[] for _ in range(n_dst)]
    for s, d in enumerate(nearest):
        if d >= 0:
            rows[d].append(s)
    rowptr, col, val = [0], [], []
    for r in rows:
        col += r
        val += [1.0 / float(len(r)) if norm == tg.DTOS_MEAN else 1.0 for _ in r]
        rowptr.append(len(col))
    return np.array(rowptr, np.int64), np.array(col, np.int32), np.array(val, np.float64), np.array(nearest, np.int32)


def _same(got, want, what):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float64 and got[3].dtype == np.int32, what
    for a, b, name in zip(got, want, ("rowptr", "col", "val", "nearest")):
        assert a.shape == b.shape and np.array_equal(a, b), (what, name)
    assert np.array_equal(got[2].view(np.int64), want[2].view(np.int64)), (what, "val bits")


def _clouds(seed, n_src, n_dst):
    rng = np.random.default_rng(seed)
    return (_unit(rng.uniform(0.3, 0.9, n_src), rng.uniform(-2.0, -1.2, n_src)), _unit(rng.uniform(0.3, 0.9, n_dst), rng.uniform(-2.0, -1.2, n_dst)))


@pytest.mark.parametrize("n_src,n_dst", [(200, 60), (60, 200), (1, 7), (97, 1)])
@pytest.mark.parametrize("norm", (tg.DTOS_SUM, tg.DTOS_MEAN))
def test_mirror_equals_the_loop(n_src, n_dst, norm):
    src, dst = _clouds(n_src * 1000 + n_dst, n_src, n_dst)
    got = tg.nearest_dtos_rows(src, dst, norm)
    _same(got, _loop(src, dst, norm), (n_src, n_dst, norm))
    lens = np.diff(got[0])
    assert lens.sum() == n_src and (got[3] >= 0).all()
    for d in np.flatnonzero(lens):
        assert (np.diff(got[1][got[0][d]:got[0][d + 1]]) > 0).all(), "a row's sources ascend"


def test_exact_tie_goes_to_the_lower_id():
    """destination points at lat +-a on one meridian, the source on the equator of that meridian: only the sign of dz differs, so the
    two d2 are equal bit for bit"""
    a, L0 = 0.3, 0.5
    src = _unit([0.0], [L0])
    for order in ((a, -a), (-a, a)):
        dst = _unit([0.9, order[0], 0.8, order[1]], [L0 + 1.0, L0, L0 - 1.0, L0])
        d = src - dst[:, [1, 3]]
        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        assert d2[0] == d2[1], "the premise: an exact tie"
        got = tg.nearest_dtos_rows(src, dst)
        _same(got, _loop(src, dst, tg.DTOS_SUM), order)
        assert got[3][0] == 1 and np.array_equal(got[0], [0, 0, 1, 1, 1])
        got = tg.nearest_dtos_rows(src, dst, dst_mask=np.array([0, 1, 0, 0], np.uint8))
        assert got[3][0] == 3, "the lower id masked: the tie's other half"


def test_a_source_that_coincides_with_a_destination():
    src, dst = _clouds(5, 50, 30)
    src[:, 17] = dst[:, 11]
    src[:, 18] = dst[:, 11]
    dst[:, 23] = dst[:, 11]                      # and an exact duplicate among the destinations: the lower id
    for norm in (tg.DTOS_SUM, tg.DTOS_MEAN):
        got = tg.nearest_dtos_rows(src, dst, norm)
        _same(got, _loop(src, dst, norm), "coincide")
        assert got[3][17] == 11 and got[3][18] == 11 and got[0][24] == got[0][23]


@pytest.mark.parametrize("norm", (tg.DTOS_SUM, tg.DTOS_MEAN))
def test_masks(norm):
    src, dst = _clouds(9, 180, 40)
    rng = np.random.default_rng(10)
    sm, dm = rng.uniform(size=180) < 0.3, (rng.uniform(size=40) < 0.5).astype(np.uint8)
    free = tg.nearest_dtos_rows(src, dst, norm)
    for s_, d_, what in ((sm, None, "src"), (None, dm, "dst"), (sm, dm, "both")):
        got = tg.nearest_dtos_rows(src, dst, norm, s_, d_)
        _same(got, _loop(src, dst, norm, s_, d_), what)
        if s_ is not None:
            assert (got[3][sm] == -1).all()
        if d_ is not None:
            live = got[3][got[3] >= 0]
            assert not dm[live].any() and (np.diff(got[0])[dm != 0] == 0).all()
            assert dm[free[3]].any(), "some source had to move on to the next unmasked destination"
    # every destination masked; every source masked; an empty source set
    for s_, d_ in ((None, np.ones(40, bool)), (np.ones(180, bool), None), (np.ones(180, np.uint8), np.ones(40, np.uint8))):
        got = tg.nearest_dtos_rows(src, dst, norm, s_, d_)
        _same(got, _loop(src, dst, norm, s_, d_), "all masked")
        assert (got[3] == -1).all() and (got[0] == 0).all() and got[1].size == 0 and got[2].size == 0
    got = tg.nearest_dtos_rows(np.zeros((3, 0)), dst, norm)
    assert got[3].size == 0 and np.array_equal(got[0], np.zeros(41, np.int64)) and got[1].size == 0 and got[2].size == 0


def test_values():
    """MEAN row sums within len x 2^-53 of 1, every SUM value exactly 1.0"""
    src, dst = _clouds(3, 200, 12)
    rowptr, col, val, _ = tg.nearest_dtos_rows(src, dst, tg.DTOS_MEAN)
    lens = np.diff(rowptr)
    assert lens.max() > 8
    for d in np.flatnonzero(lens):
        row = val[rowptr[d]:rowptr[d + 1]]
        assert (row == 1.0 / float(lens[d])).all()
        exact = sum(Fraction(float(v)) for v in row)            # the row's sum without any rounding of its own
        assert abs(exact - 1) <= int(lens[d]) * Fraction(1, 2 ** 53), (d, lens[d])
    assert (tg.nearest_dtos_rows(src, dst, tg.DTOS_SUM)[2] == 1.0).all()
    with pytest.raises(ValueError):
        tg.nearest_dtos_rows(src, dst, 2)
