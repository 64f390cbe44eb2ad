"""The numpy mirror of mpg_handle_creep (target_grid.creep_rows with creep_neighbours_grid / _mesh) on hand-worked cases: a strip filled
from one end (every row a sorted copy), a 3 x 3 block from its centre, the exact half-sum between two mapped ends, the Chebyshev levels of
a corner seed, the level cap, dst_skip as a wall with and without a gap, the chain identity, nothing and everything unmapped, and the row
sums of a 61 x 41 grid with a 4-point rim and a hole.

The row-sum bound: a filled row's exact sum (math.fsum of its stored values) stays within (row length + level) * 2^-52 of 1 when the
mapped rows are Dirichlet rows of three entries.  Where it comes from: a mapped row's stored values sum to 1 within 3 * 2^-53; a column's
value is a sum of k positive terms and one division, relative error at most k * 2^-53 with k <= 8 (the contributors hold a column once
each), so a level adds at most 4 * 2^-52 in the worst case and 0 where m = 1, while the rows grow by far more than three entries a level
(the union of up to 8 rows of random columns): the row-length term covers the levels with a wide margin.  The test prints the worst
figure."""
import math

import numpy as np

from mpassit_amd import target_grid as tg

EPS = 2.0 ** -52
ALL = tg.CREEP_ALL_LEVELS


def _csr(n, rows):
    """rows: {p: [(col, val), ...]} -> (rowptr, col, val)"""
    lens = np.array([len(rows.get(p, ())) for p in range(n)], np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    col = np.array([c for p in range(n) for c, _ in rows.get(p, ())], np.int32)
    val = np.array([v for p in range(n) for _, v in rows.get(p, ())], np.float64)
    return rowptr, col, val


def _row(out, p):
    _, rowptr, col, val = out
    return col[rowptr[p]:rowptr[p + 1]].tolist(), val[rowptr[p]:rowptr[p + 1]].tolist()


def _same(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


def test_neighbour_tables():
    nbr, cnt = tg.creep_neighbours_grid(1, 1)
    assert cnt.tolist() == [0] and (nbr == -1).all()
    nbr, cnt = tg.creep_neighbours_grid(1, 5)
    assert cnt.tolist() == [1, 2, 2, 2, 1] and nbr[:, :2].tolist() == [[1, -1], [0, 2], [1, 3], [2, 4], [3, -1]]
    nbr, cnt = tg.creep_neighbours_grid(2, 2)
    assert cnt.tolist() == [3] * 4 and nbr[:, :3].tolist() == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]
    nbr, cnt = tg.creep_neighbours_grid(3, 3)
    assert cnt.tolist() == [3, 5, 3, 5, 8, 5, 3, 5, 3]
    assert nbr[0, :3].tolist() == [1, 3, 4] and nbr[1, :5].tolist() == [0, 2, 3, 4, 5] and nbr[4].tolist() == [0, 1, 2, 3, 5, 6, 7, 8]
    nbr, cnt = tg.creep_neighbours_grid(4, 3)          # no shifted window at a border, unlike patch_neighbours_grid
    assert nbr[3, :cnt[3]].tolist() == [2, 6, 7]
    voc = [[1, 2, 0], [1, 2, 3], [1, 0, 0], [2, 3, 0], [3, 0, 0], [0, 0, 0]]   # test_patch_abi's mesh and a bare cell
    tri = [[0, 1, 2], [0, 1, 3], [-1, 3, 4]]
    nbr, cnt = tg.creep_neighbours_mesh(voc, tri)
    assert cnt.tolist() == [3, 3, 2, 2, 0, 0]
    assert nbr.tolist() == [[1, 2, 3], [0, 2, 3], [0, 1, -1], [0, 1, -1], [-1, -1, -1], [-1, -1, -1]]
    n1, c1, _ = tg.patch_neighbours_mesh(voc, tri)
    assert all(sorted(set(n1[p, :c1[p]].tolist()) - {p}) == nbr[p, :cnt[p]].tolist() for p in range(6)), "N1 minus self"
    nbr, cnt = tg.creep_neighbours_mesh(np.zeros((4, 3), np.int32), np.zeros((3, 3), np.int32))
    assert cnt.tolist() == [0] * 4, "bare centres have no neighbours"


def test_strip_from_one_end():
    rowptr, col, val = _csr(5, {0: [(7, 0.5), (3, 0.25), (7, 0.125)]})
    out = tg.creep_rows(rowptr, col, val, tg.creep_neighbours_grid(1, 5))
    assert out[0].tolist() == [0, 1, 2, 3, 4]
    assert _row(out, 0) == ([7, 3, 7], [0.5, 0.25, 0.125]), "the mapped row verbatim, duplicate column and all"
    for p in range(1, 5):
        assert _row(out, p) == ([3, 7], [0.25, 0.625]), "m = 1: the neighbour's row sorted and merged"
    out = tg.creep_rows(rowptr, col, val, tg.creep_neighbours_grid(5, 1))
    assert out[0].tolist() == [0, 1, 2, 3, 4] and out[1].tolist() == [0, 3, 5, 7, 9, 11]
    # values that appear once are copied exactly, whatever they are
    rowptr, col, val = _csr(3, {2: [(5, 0.1), (1, 1.0 / 3.0)]})
    out = tg.creep_rows(rowptr, col, val, tg.creep_neighbours_grid(1, 3))
    assert out[0].tolist() == [2, 1, 0] and _row(out, 0) == ([1, 5], [1.0 / 3.0, 0.1]) == _row(out, 1)


def test_block_from_its_centre():
    rowptr, col, val = _csr(9, {4: [(2, 0.75), (0, 0.25)]})
    out = tg.creep_rows(rowptr, col, val, tg.creep_neighbours_grid(3, 3))
    assert out[0].tolist() == [1, 1, 1, 1, 0, 1, 1, 1, 1]
    for p in (0, 1, 2, 3, 5, 6, 7, 8):
        assert _row(out, p) == ([0, 2], [0.25, 0.75])


def test_half_sum_between_two_ends():
    rowptr, col, val = _csr(3, {0: [(4, 0.5), (9, 0.5)], 2: [(9, 0.25), (1, 0.75)]})
    out = tg.creep_rows(rowptr, col, val, tg.creep_neighbours_grid(3, 1))
    assert out[0].tolist() == [0, 1, 0]
    assert _row(out, 1) == ([1, 4, 9], [0.375, 0.25, 0.375]), "m = 2: (0.5 + 0.25) / 2 on the shared column, a half elsewhere"
    # zero values stay in the row: the pattern does not depend on the values
    rowptr, col, val = _csr(3, {0: [(4, 0.5)], 2: [(4, -0.5), (6, 0.0)]})
    assert _row(tg.creep_rows(rowptr, col, val, tg.creep_neighbours_grid(3, 1)), 1) == ([4, 6], [0.0, 0.0])


def _corner_seed(rng):
    return _csr(63, {0: [(int(c), float(v)) for c, v in zip(rng.integers(0, 50, 3), rng.dirichlet([1, 1, 1]))]})


def test_corner_seed_levels_are_chebyshev_distances():
    rowptr, col, val = _corner_seed(np.random.default_rng(1))
    nb = tg.creep_neighbours_grid(9, 7)
    level, optr, ocol, oval = tg.creep_rows(rowptr, col, val, nb, ALL)
    j, i = np.divmod(np.arange(63), 9)
    assert np.array_equal(level, np.maximum(i, j))
    assert ((level > 0).sum(), level.max(), (level < 0).sum()) == (62, 8, 0), "rows filled, last level, rows still unmapped"
    assert (np.diff(optr) > 0).all()
    # the level cap
    l3, p3, c3, v3 = tg.creep_rows(rowptr, col, val, nb, 3)
    want = np.where(np.maximum(i, j) <= 3, np.maximum(i, j), -1)
    assert np.array_equal(l3, want) and ((l3 > 0).sum(), l3.max(), (l3 < 0).sum()) == (15, 3, 47)
    assert np.array_equal(np.diff(p3) > 0, want >= 0)
    for p in np.flatnonzero(want >= 0):
        assert _row((l3, p3, c3, v3), p) == _row((level, optr, ocol, oval), p), "a capped fill is a prefix of the full one"
    # the chain identity
    two = tg.creep_rows(rowptr, col, val, nb, 2)
    five = tg.creep_rows(two[1], two[2], two[3], nb, 3)
    assert _same(five[1:], tg.creep_rows(rowptr, col, val, nb, 5)[1:]), "creep(creep(h, 2), 3) has the bytes of creep(h, 5)"


def test_dst_skip_is_a_wall():
    rng = np.random.default_rng(2)
    nx, ny = 7, 5
    rows = {j * nx: [(int(c), float(v)) for c, v in zip(rng.integers(0, 30, 2), (0.5, 0.5))] for j in range(ny)}   # column 0 mapped
    rowptr, col, val = _csr(nx * ny, rows)
    nb = tg.creep_neighbours_grid(nx, ny)
    j, i = np.divmod(np.arange(nx * ny), nx)
    wall = i == 3
    level = tg.creep_rows(rowptr, col, val, nb, ALL, dst_skip=wall)[0]
    assert np.array_equal(level, np.where(i < 3, i, -1)), "the front stops at the wall: its far side is never reached"
    gap = wall & (j != 2)
    level, optr = tg.creep_rows(rowptr, col, val, nb, ALL, dst_skip=gap)[:2]
    want = np.where(i <= 3, i, 3 + np.maximum(i - 3, np.abs(j - 2)))
    want[gap] = -1
    assert np.array_equal(level, want), "through the gap, and outward from it on the far side"
    assert np.array_equal(np.diff(optr) > 0, want >= 0)
    # a skipped row that is mapped keeps its row, is level 0 and is a neighbour; skipping nothing is no skip
    keep = np.zeros(nx * ny, bool)
    keep[0] = True
    a = tg.creep_rows(rowptr, col, val, nb, ALL, dst_skip=keep)
    assert _same(a, tg.creep_rows(rowptr, col, val, nb, ALL)) and _same(a, tg.creep_rows(rowptr, col, val, nb, ALL, dst_skip=np.zeros(nx * ny, np.uint8)))


def test_nothing_and_everything_unmapped():
    rng = np.random.default_rng(3)
    rows = {p: [(int(rng.integers(0, 9)), 0.5), (int(rng.integers(0, 9)), 0.5)] for p in range(12)}
    rowptr, col, val = _csr(12, rows)
    level, optr, ocol, oval = tg.creep_rows(rowptr, col, val, tg.creep_neighbours_grid(4, 3), 2)
    assert (level == 0).all() and _same((optr, ocol, oval), (rowptr, col, val)), "nothing unmapped: a copy of the pattern"
    rowptr, col, val = _csr(12, {})
    level, optr, ocol, oval = tg.creep_rows(rowptr, col, val, tg.creep_neighbours_grid(4, 3))
    assert (level == -1).all() and optr.tolist() == [0] * 13 and ocol.size == 0 and oval.size == 0
    # bare centres: nothing is filled
    rowptr, col, val = _csr(4, {1: [(0, 1.0)]})
    level = tg.creep_rows(rowptr, col, val, tg.creep_neighbours_mesh(np.zeros((4, 3), np.int32), np.zeros((3, 3), np.int32)))[0]
    assert level.tolist() == [-1, 0, -1, -1]


def rim_and_hole(nx=61, ny=41, rim=4, hole=(25, 16, 10, 9), n_src=5000, seed=5):
    """The row-sum case: Dirichlet rows of three entries everywhere but a `rim`-point rim and a hole (i0, j0, width, height)."""
    rng = np.random.default_rng(seed)
    j, i = np.divmod(np.arange(nx * ny), nx)
    un = (i < rim) | (i >= nx - rim) | (j < rim) | (j >= ny - rim)
    un |= (i >= hole[0]) & (i < hole[0] + hole[2]) & (j >= hole[1]) & (j < hole[1] + hole[3])
    rows = {}
    for p in np.flatnonzero(~un):
        c = rng.choice(n_src, 3, replace=False)
        rows[int(p)] = list(zip(c.tolist(), rng.dirichlet([1.0, 1.0, 1.0]).tolist()))
    return _csr(nx * ny, rows), un


def worst_row_sum(level, rowptr, val):
    """max over the filled rows of |fsum(row) - 1| / ((row length + level) eps) -> (the ratio, the worst error in eps)"""
    worst, err = 0.0, 0.0
    for p in np.flatnonzero(level > 0):
        n = int(rowptr[p + 1] - rowptr[p])
        e = abs(math.fsum(val[rowptr[p]:rowptr[p + 1]].tolist()) - 1.0)
        worst, err = max(worst, e / ((n + int(level[p])) * EPS)), max(err, e / EPS)
    return worst, err


def test_row_sums():
    (rowptr, col, val), un = rim_and_hole()
    level, optr, ocol, oval = tg.creep_rows(rowptr, col, val, tg.creep_neighbours_grid(61, 41), ALL)
    assert np.array_equal(level > 0, un) and level.max() == 5 and (level < 0).sum() == 0
    ratio, err = worst_row_sum(level, optr, oval)
    print("%d rows filled in %d levels, longest row %d, worst row-sum error %.3g eps, %.3g of the bound"
          % ((level > 0).sum(), level.max(), np.diff(optr).max(), err, ratio))
    assert ratio <= 1.0
    assert (oval[np.repeat(level > 0, np.diff(optr))] > 0.0).all(), "an average of positive weights"
