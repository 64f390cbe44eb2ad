"""Comparison helpers of the full-size oracle tests (test_wind_oracle_gpu, test_odd_grid_oracle_gpu): result buffers that show an
unwritten point (NaN-filled) and a write outside the result (canary bands either side), and comparisons that cannot pass vacuously --
a NaN, an untouched point or a touched canary fails them, whatever the tolerance (tests/test_oracle_compare.py shows each).

Everything works on torch tensors of any device, so that the 100 M-value results of those tests are compared where they live."""
import numpy as np

CANARY = 12345.0      # the bands' value: a float no kernel stores by accident (NaN / 0.0 / a regridded value)
BAND_BYTES = 256      # each band, at least: more than one 128-byte line on either side
LINE = 128


class Banded:
    """n elements of `dtype` on `device`, NaN-filled, between two canary bands of >= 256 bytes; the result starts `shift` elements
    into a 128-byte line.  .res is the result (a view), .raw the whole allocation."""

    def __init__(self, torch, n, dtype, shift=0, device="cuda"):
        es = torch.empty((), dtype=dtype).element_size()
        pad = (BAND_BYTES + LINE) // es                          # whole lines before the result's line
        self.raw = torch.full((n + 2 * pad + 2 * LINE // es,), CANARY, dtype=dtype, device=device)
        lead = (-self.raw.data_ptr() % LINE) // es                # (host allocations are aligned to less than a line)
        assert (self.raw.data_ptr() + lead * es) % LINE == 0
        self.o0, self.n, self.es = lead + pad + shift, n, es
        self.res = self.raw[self.o0:self.o0 + n]
        self.res.fill_(float("nan"))
        assert self.res.data_ptr() % LINE == shift * es

    def ptr(self):
        return self.res.data_ptr()

    def assert_canaries(self, what=""):
        assert_canaries(self.raw, self.o0, self.n, what)


def _bits(t):
    import torch
    return t.view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


def assert_canaries(raw, o0, n, what=""):
    """Both bands still hold CANARY bit for bit (a NaN, a 0.0 or any regridded value written there fails)."""
    import torch
    c = _bits(torch.full((1,), CANARY, dtype=raw.dtype, device=raw.device))
    lo, hi = _bits(raw[:o0]), _bits(raw[o0 + n:])
    assert lo.numel() > 0 and hi.numel() > 0
    bad_lo, bad_hi = int((lo != c).sum()), int((hi != c).sum())
    assert bad_lo == 0 and bad_hi == 0, "%s: wrote outside the result (%d elements before it, %d after it)" % (what, bad_lo, bad_hi)


def assert_all_finite(got, what=""):
    import torch
    bad = ~torch.isfinite(got)
    nbad = int(bad.sum())
    if nbad:
        first = np.unravel_index(int(torch.nonzero(bad.reshape(-1))[0]), tuple(got.shape))
        raise AssertionError("%s: %d points are NaN / Inf (an unwritten point?), the first at %s" % (what, nbad, first))


def assert_close(got, want, tol, scale, what="", mask=None):
    """float64 result against a float64 reference: every point (or the points of `mask`, a bool tensor over the LAST dimension) within
    tol * scale -- tol a number, or a tensor over the last dimension (a bar per point); the result must be finite everywhere, whatever
    the mask.  Returns the largest difference / scale."""
    import torch
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    assert got.dtype == torch.float64 and want.dtype == torch.float64
    assert_all_finite(got, what)
    assert_all_finite(want, what + " (reference)")
    d = (got - want).abs()
    if mask is not None:
        d = d[..., mask]
    dmax = float(d.max()) if d.numel() else 0.0
    if isinstance(tol, torch.Tensor):
        t = tol[mask] if mask is not None else tol
        over = d > t * scale
        assert not bool(over.any()), "%s: %d points beyond their bar, largest difference %.3e x scale %.3e" % (
            what, int(over.sum()), dmax / scale, scale)
        return dmax / scale
    assert dmax <= tol * scale, "%s: largest difference %.3e = %.3e x scale %.3e, bar %.1e" % (what, dmax, dmax / scale, scale, tol)
    return dmax / scale


def assert_zero(got, mask, what=""):
    """The points of `mask` (unmapped; a bool tensor over the LAST dimension) are exactly 0.0."""
    v = got[..., mask]
    n = int((v != 0.0).sum())
    assert n == 0, "%s: %d unmapped points are not 0.0" % (what, n)


def _ordered(b32):
    """int32 bit patterns of float32 -> int64 keys ordered like the floats (+0 and -0 both 0): key distance = ulp distance."""
    import torch
    b = b32.to(torch.int64)
    return torch.where(b < 0, -(b & 0x7FFFFFFF), b)


def assert_f32_ulp(got32, want64, what="", max_frac=1e-4, eps=0.0):
    """float32 result against float32(reference): equal, or one float32 ulp apart where the two float64 values straddle a rounding
    boundary, on at most `max_frac` of the points.  eps: the absolute uncertainty of the float64 reference (its own float64 bar); a
    result within eps + 1 ulp of it is the rounding of a value within that bar -- which matters only next to 0.0, where a float32 ulp
    is smaller than eps (sums of signed values cancel there).  NaN / Inf fail.  Returns (largest ulp distance, fraction of points not
    equal)."""
    import torch
    assert got32.dtype == torch.float32 and got32.shape == want64.shape, (what, got32.dtype, tuple(got32.shape), tuple(want64.shape))
    assert_all_finite(got32, what)
    ref32 = want64.to(torch.float32)
    dist = (_ordered(_bits(got32.contiguous())) - _ordered(_bits(ref32.contiguous()))).abs()
    frac = float((dist != 0).sum()) / max(dist.numel(), 1)
    far = dist > 1
    if bool(far.any()):
        a = ref32[far].abs()
        ulp = (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).to(torch.float64)
        d = (got32[far].to(torch.float64) - want64[far]).abs()
        bad = d > ulp + eps
        assert not bool(bad.any()), "%s: %d float32 ulp apart from the reference (|difference| %.3e, bar 1 ulp + %.1e)" % (
            what, int(dist[far][bad].max()), float(d[bad].max()), eps)
    umax = int(dist.max()) if dist.numel() else 0
    assert frac <= max_frac, "%s: %.2e of the points 1 ulp off (bar %.0e)" % (what, frac, max_frac)
    return umax, frac


def from_be32(t):
    """A float32 tensor holding big-endian bytes -> host-order float32 (same device)."""
    import torch
    assert t.dtype == torch.float32
    return t.contiguous().view(torch.uint8).reshape(-1, 4).flip(1).contiguous().view(torch.float32).reshape(t.shape)


def ring_mask(ny, nx):
    """[ny][nx] bool: the outermost row and column on every side (the implementation-defined ring)."""
    r = np.zeros((ny, nx), bool)
    r[0, :] = r[-1, :] = True
    r[:, 0] = r[:, -1] = True
    return r


def compare_grid_weights(idx_o, w_o, idx_g, w_g, shape, tol=1e-12):
    """Grid -> Grid weights [P][4] of the oracle and of a handle on a [ny][nx] destination.  Interior points: identical index rows,
    weights within tol.  Ring: the mapped sets are only counted.  Returns (largest interior weight difference, number of ring points
    mapped on one side only)."""
    ring = ring_mask(*shape).reshape(-1)
    inner = ~ring
    assert idx_o.shape == idx_g.shape == w_o.shape == w_g.shape
    same = (idx_o[inner] == idx_g[inner]).all(axis=1)
    if not same.all():
        p = np.nonzero(inner)[0][np.nonzero(~same)[0][0]]
        raise AssertionError("%d interior points have other sources, the first %d (j %d, i %d): oracle %s, handle %s" % (
            int((~same).sum()), p, p // shape[1], p % shape[1], idx_o[p], idx_g[p]))
    dw = float(np.abs(w_o[inner] - w_g[inner]).max())
    assert dw <= tol, "interior weights %.3e apart (bar %.0e)" % (dw, tol)
    ring_diff = int(((idx_o[ring, 0] >= 0) != (idx_g[ring, 0] >= 0)).sum())
    return dw, ring_diff
