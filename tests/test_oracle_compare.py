"""The comparison helpers of the full-size oracle tests (tests/_oracle_compare.py) are not vacuous: each kind of wrong result those tests
guard against fails them.  CPU only (torch tensors on the host), so it runs without a GPU.

A NaN makes `abs(a - b).max() < tol` False in numpy and torch alike, but nanmax, equal_nan=True or a mask applied before the NaN check
would hide one -- hence the NaN cases, including a NaN at a point the mask leaves out."""
import numpy as np
import pytest

from _oracle_compare import (CANARY, Banded, assert_close, assert_f32_ulp, assert_zero, compare_grid_weights, from_be32, ring_mask)

torch = pytest.importorskip("torch")

NLEV, P = 55, 1001


def _pair(seed=0):
    rng = np.random.default_rng(seed)
    want = torch.from_numpy(rng.uniform(-30.0, 30.0, size=(2, NLEV, P)))
    return want.clone(), want


def test_identical_results_pass():
    got, want = _pair()
    assert assert_close(got, want, 1e-14, 30.0) == 0.0
    assert assert_f32_ulp(want.to(torch.float32), want) == (0, 0.0)


def test_one_perturbed_point_in_the_last_level_fails():
    got, want = _pair()
    got[-1, -1, P // 2] += 1e-9                   # ~3e-11 of the scale: far below any visible error, far above the 1e-13 bar
    with pytest.raises(AssertionError, match="largest difference"):
        assert_close(got, want, 1e-13, 30.0)
    assert assert_close(got, want, 1e-10, 30.0) > 0.0
    bar = torch.full((P,), 1e-13, dtype=torch.float64)      # a bar per point (weights that differ explain a difference there)
    with pytest.raises(AssertionError, match="beyond their bar"):
        assert_close(got, want, bar, 30.0)
    bar[P // 2] = 1e-10
    assert assert_close(got, want, bar, 30.0) > 0.0


def test_a_single_nan_fails():
    got, want = _pair()
    got[0, 7, 3] = float("nan")
    with pytest.raises(AssertionError, match="NaN"):
        assert_close(got, want, 1.0, 30.0)       # whatever the tolerance
    mask = torch.ones(P, dtype=torch.bool)
    mask[3] = False                               # a point the comparison leaves out (the ring) must still have been written
    with pytest.raises(AssertionError, match="NaN"):
        assert_close(got, want, 1.0, 30.0, mask=mask)
    with pytest.raises(AssertionError, match="NaN"):
        assert_f32_ulp(got.to(torch.float32), want)
    with pytest.raises(AssertionError, match="NaN"):    # a NaN in the reference is no free pass either
        assert_close(want, got, 1.0, 30.0)


def test_an_unwritten_result_fails():
    _, want = _pair()
    b = Banded(torch, want.numel(), torch.float64, shift=1, device="cpu")
    b.res[:-1] = want.reshape(-1)[:-1]            # every point but the last
    with pytest.raises(AssertionError, match="NaN"):
        assert_close(b.res.view(want.shape), want, 1.0, 30.0)
    b.assert_canaries()


@pytest.mark.parametrize("dtype,shift", [(torch.float64, 0), (torch.float64, 1), (torch.float32, 1)])
@pytest.mark.parametrize("where", ["before", "after"])
def test_a_touched_canary_fails(dtype, shift, where):
    b = Banded(torch, 1000, dtype, shift=shift, device="cpu")
    es = b.raw.element_size()
    assert (b.res.data_ptr() % 128) == shift * es and b.o0 * es >= 256 and (b.raw.numel() - b.o0 - b.n) * es >= 256
    assert bool(b.res.isnan().all()) and bool((b.raw[:b.o0] == CANARY).all())
    b.res.fill_(1.0)
    b.assert_canaries()
    b.raw[b.o0 - 1 if where == "before" else b.o0 + b.n] = 0.0   # one element next to the result
    with pytest.raises(AssertionError, match="outside the result"):
        b.assert_canaries()


def test_a_two_ulp_float32_difference_fails():
    _, want = _pair()
    got = want.to(torch.float32)
    got[1, NLEV - 1, 10] = torch.nextafter(torch.nextafter(got[1, NLEV - 1, 10], torch.tensor(np.inf, dtype=torch.float32)),
                                           torch.tensor(np.inf, dtype=torch.float32))
    with pytest.raises(AssertionError, match="2 float32 ulp"):
        assert_f32_ulp(got, want)
    # one ulp at one point is the rounding-boundary case the bar allows ...
    one = want.to(torch.float32)
    one[0, 0, 0] = torch.nextafter(one[0, 0, 0], torch.tensor(-np.inf, dtype=torch.float32))
    assert assert_f32_ulp(one, want) == (1, 1.0 / want.numel())
    # ... but not on more than the allowed fraction of the points
    many = want.to(torch.float32)
    many[:, :, :5] = torch.nextafter(many[:, :, :5], torch.full_like(many[:, :, :5], np.inf))
    with pytest.raises(AssertionError, match="1 ulp off"):
        assert_f32_ulp(many, want)
    # next to 0.0 a float32 ulp is smaller than the float64 reference's own bar: 2 ulp there are the rounding of a value within it
    tiny = torch.tensor([3e-13], dtype=torch.float64)
    t2 = torch.nextafter(torch.nextafter(tiny.to(torch.float32), torch.tensor([1.0])), torch.tensor([1.0]))
    with pytest.raises(AssertionError, match="2 float32 ulp"):
        assert_f32_ulp(t2, tiny)
    assert assert_f32_ulp(t2, tiny, eps=1e-13, max_frac=1.0) == (2, 1.0)
    # across zero: the ulp distance counts -0 / +0 as one value
    z = torch.zeros(4, dtype=torch.float64)
    assert assert_f32_ulp(-torch.zeros(4, dtype=torch.float32), z) == (0, 0.0)


def test_an_unmapped_point_that_is_not_zero_fails():
    got, _ = _pair()
    unmapped = torch.zeros(P, dtype=torch.bool)
    unmapped[[0, P - 1]] = True
    got[:, :, unmapped] = 0.0
    assert_zero(got, unmapped)
    got[-1, -1, P - 1] = 1e-300
    with pytest.raises(AssertionError, match="not 0.0"):
        assert_zero(got, unmapped)


def test_big_endian_float32_round_trip():
    x = torch.tensor([1.0, -2.5, 3.0e-38, 12345.678], dtype=torch.float32)
    be = torch.from_numpy(x.numpy().astype(">f4").view(np.float32).copy())
    assert not torch.equal(be, x)
    assert torch.equal(from_be32(be), x)


def test_grid_weights_interior_strict_ring_counted():
    ny, nx = 5, 7
    rng = np.random.default_rng(3)
    idx = rng.integers(0, 100, size=(ny * nx, 4)).astype(np.int32)
    w = rng.random((ny * nx, 4))
    ring = ring_mask(ny, nx).reshape(-1)
    assert ring.sum() == 2 * nx + 2 * (ny - 2)
    idx_g, w_g = idx.copy(), w.copy()
    p_ring = int(np.nonzero(ring)[0][3])
    idx_g[p_ring] = -1                             # the ring: counted, not failed
    assert compare_grid_weights(idx, w, idx_g, w_g, (ny, nx)) == (0.0, 1)
    w_g[nx + 2, 1] += 1e-11                        # an interior weight beyond the bar
    with pytest.raises(AssertionError, match="interior weights"):
        compare_grid_weights(idx, w, idx_g, w_g, (ny, nx))
    w_g[nx + 2, 1] = w[nx + 2, 1]
    idx_g[2 * nx + 3, 2] += 1                      # an interior point with another source
    with pytest.raises(AssertionError, match="other sources"):
        compare_grid_weights(idx, w, idx_g, w_g, (ny, nx))
