"""CPU checks of target_grid.compose_csr, the bit-exact numpy mirror of mpg_handle_compose / mpg_compose_weights_dev, against
scipy.sparse: the pattern holds every non-zero of A @ B, the values lie within (terms + 1) 2^-53 (|A| |B|) entrywise, columns ascend and
are distinct, the identity on either side returns the other operand's bits, bilinear row sums stay 1, and duplicates, empty rows, long
rows and nnz = 0 are handled.  The measured figures are printed before they are held to their bounds."""
import numpy as np
import pytest
import scipy.sparse as sp

EPS = 2.0 ** -53


def _random_csr(rng, n_dst, n_src, lens, dup=False, positive=False):
    """CSR with the given row lengths, columns in random (unsorted) order; dup: columns may repeat inside a row"""
    lens = np.asarray(lens, dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([rng.choice(n_src, size=int(l), replace=dup or l > n_src) for l in lens] + [np.empty(0, np.int64)]).astype(np.int64)
    val = rng.uniform(0.1, 1.0, col.size) if positive else rng.uniform(-1.0, 1.0, col.size)
    return rowptr, col, val


def _bilinear_csr(rng, n_dst, n_src, k, empty=()):
    """rows of k positive weights that sum to 1 (rounded), rows in `empty` without entries"""
    lens = np.full(n_dst, k)
    lens[list(empty)] = 0
    rowptr, col, val = _random_csr(rng, n_dst, n_src, lens, positive=True)
    row = np.repeat(np.arange(n_dst), lens)
    val = val / np.bincount(row, weights=val, minlength=n_dst)[row]
    return rowptr, col, val


def _sp(rowptr, col, val, n_src):
    return sp.csr_matrix((val, col, rowptr), shape=(rowptr.size - 1, n_src))      # duplicates are summed on conversion


def _terms(a, b, n_mid, n_src):
    """[n_dst x n_src] number of (p, q) pairs behind every entry of A @ B"""
    ones = lambda m: sp.csr_matrix((np.ones(m[1].size), m[1], m[0]), shape=(m[0].size - 1, m[3]))
    return (ones((a[0], a[1], a[2], n_mid)) @ ones((b[0], b[1], b[2], n_src))).toarray()


def _check(a, b, n_mid, n_src, label):
    from mpassit_amd import target_grid as tg
    rowptr, col, vals = tg.compose_csr(a[0], a[1], a[2], b[0], b[1], b[2])
    n = a[0].size - 1
    assert rowptr.dtype == np.int64 and col.dtype == np.int32 and vals.shape == (1, col.size) and vals.dtype == np.float64
    assert rowptr.size == n + 1 and rowptr[0] == 0 and rowptr[-1] == col.size and (np.diff(rowptr) >= 0).all()
    for i in range(n):                                           # ascending and distinct inside every row
        assert (np.diff(col[rowptr[i]:rowptr[i + 1]].astype(np.int64)) > 0).all()
    assert col.size == 0 or (col.min() >= 0 and col.max() < n_src)
    C = np.zeros((n, n_src))
    P = np.zeros((n, n_src), bool)
    row = np.repeat(np.arange(n), np.diff(rowptr))
    C[row, col] = vals[0]
    P[row, col] = True
    ref = (_sp(a[0], a[1], a[2], n_mid) @ _sp(b[0], b[1], b[2], n_src)).toarray()
    mag = (_sp(a[0], a[1], np.abs(a[2]), n_mid) @ _sp(b[0], b[1], np.abs(b[2]), n_src)).toarray()
    terms = _terms(a, b, n_mid, n_src)
    assert P[ref != 0.0].all(), "the pattern misses a non-zero of A @ B"
    assert np.array_equal(P, terms > 0), "the pattern is the set of reachable columns, structural zeros included"
    excess = np.abs(C - ref) - (terms + 1) * EPS * mag
    print("%s: nnz %d, most terms %d, max |C - A@B| %.3e, max excess over the bound %.3e" % (label, col.size, terms.max(initial=0),
                                                                                          np.abs(C - ref).max(initial=0.0), excess.max(initial=0.0)))
    assert (excess <= 0.0).all()
    return rowptr, col, vals


def test_against_scipy_random():
    rng = np.random.default_rng(24)
    n_dst, n_mid, n_src = 57, 41, 33
    a = _random_csr(rng, n_dst, n_mid, rng.integers(0, 9, n_dst))
    b = _random_csr(rng, n_mid, n_src, rng.integers(0, 7, n_mid))
    _check(a, b, n_mid, n_src, "random")


def test_duplicates_empty_rows_and_long_rows():
    from mpassit_amd import target_grid as tg
    rng = np.random.default_rng(7)
    n_dst, n_mid, n_src = 23, 19, 11
    la, lb = rng.integers(0, 6, n_dst), rng.integers(0, 5, n_mid)
    la[[0, 5, 22]] = 0
    lb[[2, 3, 18]] = 0
    la[9] = 400                                                  # far more terms per entry than the vectorised passes take
    a = _random_csr(rng, n_dst, n_mid, la, dup=True)
    b = _random_csr(rng, n_mid, n_src, lb, dup=True)
    assert any(np.unique(a[1][a[0][i]:a[0][i + 1]]).size < la[i] for i in range(n_dst))
    assert any(np.unique(b[1][b[0][i]:b[0][i + 1]]).size < lb[i] for i in range(n_mid))
    rowptr, col, vals = _check(a, b, n_mid, n_src, "duplicates")
    assert _terms(a, b, n_mid, n_src).max() > tg._COMPOSE_VECTOR_PASSES
    for i in (0, 5, 22):
        assert rowptr[i] == rowptr[i + 1]
    # a row of A that reaches only empty rows of B is empty
    a2 = (np.array([0, 2, 3]), np.array([2, 3, 0]), np.array([1.0, 2.0, 3.0]))
    r2, c2, v2 = tg.compose_csr(a2[0], a2[1], a2[2], b[0], b[1], b[2])
    assert r2[0] == r2[1] == 0 and r2[2] == np.unique(b[1][b[0][0]:b[0][1]]).size
    # the plain loop and the passes give the same bits: the same product with the loop taking everything behind the first term
    keep = tg._COMPOSE_VECTOR_PASSES
    try:
        tg._COMPOSE_VECTOR_PASSES = 1
        again = tg.compose_csr(a[0], a[1], a[2], b[0], b[1], b[2])
    finally:
        tg._COMPOSE_VECTOR_PASSES = keep
    assert np.array_equal(again[0], rowptr) and np.array_equal(again[1], col) and again[2].tobytes() == vals.tobytes()


def test_summation_order_is_the_stated_one():
    """an entry with three terms whose sum depends on the order: ((t0 + t1) + t2) from 0.0"""
    from mpassit_amd import target_grid as tg
    a = (np.array([0, 3]), np.array([2, 0, 1]), np.array([1.0, 1.0, 1.0]))
    b = (np.array([0, 1, 2, 3]), np.array([0, 0, 0]), np.array([-1e16, 1.0, 1e16]))      # A visits B's rows 2, 0, 1
    rowptr, col, vals = tg.compose_csr(a[0], a[1], a[2], b[0], b[1], b[2])
    assert rowptr.tolist() == [0, 1] and col.tolist() == [0]
    assert vals[0, 0] == ((0.0 + 1e16) + -1e16) + 1.0 == 1.0
    a = (np.array([0, 3]), np.array([0, 1, 2]), np.array([1.0, 1.0, 1.0]))               # ... rows 0, 1, 2: the 1.0 is absorbed
    assert tg.compose_csr(a[0], a[1], a[2], b[0], b[1], b[2])[2][0, 0] == ((0.0 + -1e16) + 1.0) + 1e16 == 0.0
    # a product that comes out -0.0 is added to +0.0: +0.0, and the entry stays
    a = (np.array([0, 1]), np.array([0]), np.array([-1.0]))
    b = (np.array([0, 1]), np.array([4]), np.array([0.0]))
    rowptr, col, vals = tg.compose_csr(a[0], a[1], a[2], b[0], b[1], b[2])
    assert col.tolist() == [4] and vals[0, 0] == 0.0 and not np.signbit(vals[0, 0])


def test_identity_on_either_side():
    from mpassit_amd import target_grid as tg
    rng = np.random.default_rng(3)
    n_dst, n_src = 31, 17
    lens = rng.integers(0, 6, n_dst)
    a = _random_csr(rng, n_dst, n_src, lens)
    order = np.concatenate([a[0][i] + np.argsort(a[1][a[0][i]:a[0][i + 1]], kind="stable") for i in range(n_dst)] + [np.empty(0, np.int64)]).astype(np.int64)
    eye = lambda n: (np.arange(n + 1), np.arange(n), np.ones(n))
    for got in (tg.compose_csr(a[0], a[1], a[2], *eye(n_src)), tg.compose_csr(*eye(n_dst), a[0], a[1], a[2])):
        assert np.array_equal(got[0], a[0]) and np.array_equal(got[1], a[1][order])
        assert got[2][0].tobytes() == a[2][order].tobytes()      # 0.0 + (a * 1.0): a's bits, columns sorted


def test_bilinear_row_sums():
    from mpassit_amd import target_grid as tg
    rng = np.random.default_rng(11)
    n_dst, n_mid, n_src = 64, 40, 50
    a = _bilinear_csr(rng, n_dst, n_mid, 3, empty=(4, 60))
    b = _bilinear_csr(rng, n_mid, n_src, 4, empty=(7,))
    rowptr, col, vals = _check(a, b, n_mid, n_src, "bilinear")
    row = np.repeat(np.arange(n_dst), np.diff(rowptr))
    sums = np.bincount(row, weights=vals[0], minlength=n_dst)
    full = np.array([rowptr_a1 > rowptr_a0 and not (a[1][rowptr_a0:rowptr_a1] == 7).any()
                     for rowptr_a0, rowptr_a1 in zip(a[0][:-1], a[0][1:])])
    assert full.sum() >= n_dst // 2 and not full[4] and not full[60]
    # the entries' own bound summed over a row, (12 terms + 1) eps of a magnitude sum of 1; the operands' row sums, each within 5 eps
    # of 1 (k <= 4 rounded quotients by a rounded sum of k); and the 12 additions of this test's own bincount
    bound = (12 + 1 + 2 * 5 + 12) * EPS * (1.0 + 16 * EPS)
    print("bilinear o bilinear: max |row sum - 1| %.3e (bound %.3e) over %d rows" % (np.abs(sums[full] - 1.0).max(), bound, full.sum()))
    assert (np.abs(sums[full] - 1.0) <= bound).all()
    assert (sums[[4, 60]] == 0.0).all() and rowptr[4] == rowptr[5]


def test_planes_and_nothing():
    from mpassit_amd import target_grid as tg
    rng = np.random.default_rng(5)
    a = _random_csr(rng, 9, 8, rng.integers(0, 4, 9))
    b = _random_csr(rng, 8, 6, rng.integers(1, 4, 8))
    planes = rng.uniform(-1.0, 1.0, (3, b[1].size))
    rowptr, col, vals = tg.compose_csr(a[0], a[1], a[2], b[0], b[1], planes)
    assert vals.shape == (3, col.size)
    for k in range(3):                                           # each plane is the product with that plane alone
        one = tg.compose_csr(a[0], a[1], a[2], b[0], b[1], planes[k])
        assert np.array_equal(one[0], rowptr) and np.array_equal(one[1], col) and one[2][0].tobytes() == vals[k].tobytes()
    # nnz = 0 on either side, and on both
    none_a = (np.zeros(10, np.int64), np.empty(0, np.int64), np.empty(0))
    none_b = (np.zeros(9, np.int64), np.empty(0, np.int64), np.empty(0))
    for x, y in ((none_a, b), (a, none_b), (none_a, none_b)):
        r, c, v = tg.compose_csr(x[0], x[1], x[2], y[0], y[1], y[2])
        assert r.tolist() == [0] * 10 and c.size == 0 and c.dtype == np.int32 and v.shape == (1, 0)
    with pytest.raises(ValueError):
        tg.compose_csr(a[0], a[1] + 8, a[2], b[0], b[1], b[2])


def test_fixed_to_csr():
    from mpassit_amd import target_grid as tg
    idx = np.array([[3, 1, 2], [-1, -1, -1], [0, -1, 5], [4, 4, 4]], np.int32)
    w = np.arange(12, dtype=np.float64).reshape(4, 3) / 8.0
    rowptr, col, val = tg.fixed_to_csr(idx, w)
    assert rowptr.tolist() == [0, 3, 3, 5, 8] and col.tolist() == [3, 1, 2, 0, 5, 4, 4, 4] and col.dtype == np.int32
    assert val.tolist() == [0.0, 0.125, 0.25, 0.75, 1.0, 1.125, 1.25, 1.375]
    rowptr, col, val = tg.fixed_to_csr(np.array([[2], [-1], [0]], np.int32))                # nearest: no weight array, every value 1.0
    assert rowptr.tolist() == [0, 1, 1, 2] and col.tolist() == [2, 0] and val.tolist() == [1.0, 1.0]
