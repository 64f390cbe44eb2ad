"""Reference of the Regrid apply for the large-offset tests (test_large_offsets_ref.py, test_large_offsets_gpu.py): plain torch, float64
values, int64 index arithmetic throughout, from the handle's own exported weights (RouteHandle.weights / RouteHandle.csr), so that only
the apply kernels are under test.

    ref[p][k] = sum_q  w[p][q] * (double) src[ off(idx[p][q], k) ]        separate multiplies and adds, stored order, from 0.0
    off(c, k) = c * nlev + k          level-fast source ([cell][lev], MPAS file order)
              = k * stride + c        cell-fast source  ([lev][cell], planes `stride` >= n_src elements apart)
    unmapped points (idx[p][0] < 0) and empty rows give 0.0;  then  ref * scale + offset  (a multiply and an add)

The bar is the one tests/test_csr_rows_apply_gpu.py derives, row by row: the kernel's row is an fma chain, the reference's separate
multiplies and adds -- two evaluations of a dot product of n terms, each within (n + 1) / 2 * eps * sum |w| |x| of the exact value to first
order, so they lie within
    bar[p] = (n[p] + 1) * eps64 * sum_q |w[p][q]| * max |x|
of each other; a float32 result is the one rounding of such a value: 2^-24 * |ref| more.  With an epilogue the row's bar scales by |scale|
and both sides round the product and the sum once more: 2 * eps64 * (|scale| * sum |w| * max |x| + |offset|) on top (apply_bar).

Everything works on chunks of destination points (chunk_points): no tensor of the reference holds more than CHUNK_BYTES / 6 bytes and a
chunk's temporaries stay below about 2 GB, whatever the size of the source or of the result.

a1_columns() is the column generator of the CSR case A1 (integer arithmetic only), here so that the CPU test can check it at full size."""
import numpy as np

EPS64 = float(np.finfo(np.float64).eps)
F32_ROUND = 2.0 ** -24
CHUNK_BYTES = 2 << 30
SPAN = 80.0                       # sources are i.i.d. uniform in [-SPAN / 2, SPAN / 2): a read of any wrong element is an error of order 1
XMAX = SPAN / 2


class Weights:
    """A handle's weights as torch tensors on `device`.  kind 'fixed': idx [P][nnz] int32 as the handle holds it (-1 in slot 0 = unmapped;
    widened to int64 before any arithmetic), w [P][nnz] float64
    (nearest, nnz = 1: ones -- the kernels copy).  kind 'csr': rowptr [P + 1] int64, col [nnz] int64, val [nnz] float64.  n [P] and sumw [P]
    are the row's entry count and sum |w| (0 for an unmapped point)."""

    def __init__(self, torch, n_src, n_dst, idx=None, w=None, rowptr=None, col=None, val=None, device="cpu"):
        self.torch, self.n_src, self.n_dst, self.device = torch, int(n_src), int(n_dst), device
        if idx is not None:
            self.kind = "fixed"
            idx = np.asarray(idx).reshape(n_dst, -1)
            self.nnz = idx.shape[1]
            w = np.ones(idx.shape) if self.nnz == 1 else np.asarray(w, np.float64).reshape(idx.shape)
            mapped = idx[:, 0] >= 0
            self.idx = torch.as_tensor(np.ascontiguousarray(idx, dtype=np.int32), device=device)
            self.w = torch.as_tensor(np.ascontiguousarray(w), device=device)
            self.n = torch.as_tensor(np.where(mapped, self.nnz, 0).astype(np.float64), device=device)
            self.sumw = torch.as_tensor(np.where(mapped, np.abs(w).sum(axis=1), 0.0), device=device)
            self.max_id = int(idx.max()) if idx.size else -1
        else:
            self.kind = "csr"
            rowptr = np.asarray(rowptr, np.int64)
            lens = np.diff(rowptr)
            self.maxlen = int(lens.max()) if lens.size else 0
            self.rowptr = torch.as_tensor(rowptr, device=device)
            self.col = torch.as_tensor(np.asarray(col).astype(np.int64), device=device)
            self.val = torch.as_tensor(np.asarray(val, np.float64), device=device)
            self.n = torch.as_tensor(lens.astype(np.float64), device=device)
            sumw = np.bincount(np.repeat(np.arange(n_dst), lens), weights=np.abs(val), minlength=n_dst) if n_dst else np.zeros(0)
            self.sumw = torch.as_tensor(sumw, device=device)
            self.max_id = int(np.asarray(col).max()) if len(col) else -1

    @classmethod
    def from_handle(cls, torch, rh, device="cuda"):
        if rh.nnz_per_row == 0:
            rowptr, col, val = rh.csr()
            return cls(torch, rh.n_src, rh.n_dst, rowptr=rowptr, col=col, val=val, device=device)
        idx, w = rh.weights()
        return cls(torch, rh.n_src, rh.n_dst, idx=idx, w=w, device=device)


def src_offsets(torch, c, nlev, lev_fast, stride, dst_rows):
    """int64 element offsets of sources c [m] at every level: [m][nlev] (dst_rows) or [nlev][m]."""
    assert c.dtype == torch.int64
    k = torch.arange(nlev, dtype=torch.int64, device=c.device)
    cc, kk = (c[:, None], k[None, :]) if dst_rows else (c[None, :], k[:, None])
    return cc * nlev + kk if lev_fast else kk * int(stride) + cc


def chunk_points(nlev, n_dst):
    """Destination points per chunk: six float64 temporaries of a chunk stay below CHUNK_BYTES."""
    return max(1, min(int(n_dst), CHUNK_BYTES // (6 * 8 * int(nlev))))


def apply_ref(W, src, nlev, lev_fast, stride=None, p0=0, p1=None, dst_rows=False, scale=1.0, offset=0.0):
    """The reference for destination points [p0, p1): [p1 - p0][nlev] (dst_rows) or [nlev][p1 - p0], float64.  src: a flat tensor of any
    float dtype on W's device; stride: the level stride of a cell-fast source (default n_src)."""
    torch = W.torch
    p1 = W.n_dst if p1 is None else p1
    stride = W.n_src if stride is None else int(stride)
    src = src.reshape(-1)
    if W.kind == "fixed":
        idx, w = W.idx[p0:p1], W.w[p0:p1]
        mapped = idx[:, 0] >= 0
        acc = None
        for q in range(W.nnz):
            c = torch.where(mapped, idx[:, q], torch.zeros_like(idx[:, q])).clamp_min(0).to(torch.int64)
            x = src[src_offsets(torch, c, nlev, lev_fast, stride, dst_rows)].to(torch.float64)
            wq = w[:, q][:, None] if dst_rows else w[:, q][None, :]
            term = wq * x
            acc = 0.0 + term if acc is None else acc + term
        m = mapped[:, None] if dst_rows else mapped[None, :]
        acc = torch.where(m, acc, torch.zeros_like(acc))
    else:
        b, e = W.rowptr[p0:p1], W.rowptr[p0 + 1:p1 + 1]
        lens = e - b
        shape = (p1 - p0, nlev) if dst_rows else (nlev, p1 - p0)
        acc = torch.zeros(shape, dtype=torch.float64, device=src.device)
        for q in range(int(lens.max()) if lens.numel() else 0):   # entry q of every row that has one: sequential per row, stored order
            has = lens > q
            pos = torch.where(has, b + q, torch.zeros_like(b))
            c = torch.where(has, W.col[pos], torch.zeros_like(pos))
            wq = torch.where(has, W.val[pos], torch.zeros_like(W.val[pos]))
            x = src[src_offsets(torch, c, nlev, lev_fast, stride, dst_rows)].to(torch.float64)
            hh, ww = (has[:, None], wq[:, None]) if dst_rows else (has[None, :], wq[None, :])
            acc = torch.where(hh, acc + ww * x, acc)
    if (scale, offset) != (1.0, 0.0):
        acc = acc * scale + offset
    return acc


def apply_bar(W, p0=0, p1=None, xmax=XMAX, scale=1.0, offset=0.0):
    """[p1 - p0] float64: the bar of every destination point of the chunk (module docstring)."""
    p1 = W.n_dst if p1 is None else p1
    row = (W.n[p0:p1] + 1.0) * EPS64 * W.sumw[p0:p1] * xmax
    if (scale, offset) == (1.0, 0.0):
        return row
    return abs(scale) * row + 2.0 * EPS64 * (abs(scale) * W.sumw[p0:p1] * xmax + abs(offset))


def result_view(got, n_dst, nlev, dst_rows, dst_stride=None):
    """The flat result `got` as [n_dst][nlev] (dst_rows: element p * nlev + k) or [nlev][n_dst] (element k * dst_stride + p)."""
    if dst_rows:
        return got.as_strided((n_dst, nlev), (nlev, 1))
    return got.as_strided((nlev, n_dst), (n_dst if dst_stride is None else int(dst_stride), 1))


def compare(W, got, src, nlev, lev_fast, stride=None, dst_rows=False, dst_stride=None, scale=1.0, offset=0.0, xmax=XMAX, what="", skip=None):
    """Every element of the flat result `got` (float32 or float64) against the reference, chunk by chunk.  Returns the largest difference
    in units of its bar (0.0 where both are exact); raises AssertionError with the first offender.  skip: a bool tensor [n_dst] of points
    this reference does not describe (pole caps: the caller checks them itself)."""
    torch = W.torch
    view = result_view(got, W.n_dst, nlev, dst_rows, dst_stride)
    f32 = got.dtype == torch.float32
    step, worst = chunk_points(nlev, W.n_dst), 0.0
    for p0 in range(0, W.n_dst, step):
        p1 = min(p0 + step, W.n_dst)
        ref = apply_ref(W, src, nlev, lev_fast, stride, p0, p1, dst_rows, scale, offset)
        bar = apply_bar(W, p0, p1, xmax, scale, offset)
        tol = (bar[:, None] if dst_rows else bar[None, :]).expand(ref.shape)
        if f32:
            tol = tol + F32_ROUND * ref.abs()
        g = (view[p0:p1] if dst_rows else view[:, p0:p1]).to(torch.float64)
        d = (g - ref).abs()
        bad = ~(d <= tol)                                        # (a NaN in the result is beyond any bar)
        if skip is not None:
            keep = ~skip[p0:p1]
            bad = bad & (keep[:, None] if dst_rows else keep[None, :])
            d = torch.where((keep[:, None] if dst_rows else keep[None, :]).expand(d.shape), d, torch.zeros_like(d))
        if bool(bad.any()):
            first = torch.nonzero(bad)[0].tolist()
            a, b = (first[0] + p0, first[1]) if dst_rows else (first[1] + p0, first[0])
            raise AssertionError("%s: %d elements of points [%d, %d) beyond their bar; the first at point %d, level %d: got %r, reference %r, bar %.3e" % (
                what, int(bad.sum()), p0, p1, a, b, float(g[tuple(first)]), float(ref[tuple(first)]), float(tol[tuple(first)])))
        worst = max(worst, float((d / tol.clamp_min(1e-300)).max()))
    return worst


# ---- case A1: the column generator ------------------------------------------------------------------------------------------------
A1_NSRC, A1_NX, A1_NY, A1_NLEV = 78_200_000, 65 * 64 + 37, 1, 55
A1_LENGTHS = [1100, 4, 0, 1023, 1024, 7, 1025, 300, 55, 0, 5, 640]    # row lengths, repeated: a 64-row run holds about 28 000 entries
A1_POOL = 20_000                                                       # besides the bands: this many ids spread evenly over all sources


def a1_bands(n_src=A1_NSRC, nlev=A1_NLEV):
    """The four id bands [lo, hi) every non-empty row of A1 draws from: low ids; within 8 of 2^31 / nlev; within 8 of 2^32 / nlev; the
    last 8 ids.  With nlev = 55 the rows of the second band straddle element 2^31 of the file-order source, those of the third 2^32."""
    t31, t32 = (1 << 31) // nlev, (1 << 32) // nlev
    bands = [(0, 4096), (t31 - 8, t31 + 9), (t32 - 8, t32 + 9), (n_src - 8, n_src)]
    assert all(0 <= lo < hi <= n_src for lo, hi in bands) and bands[2][1] <= bands[3][0]
    return bands


def a1_columns(n_src=A1_NSRC, n_dst=A1_NX * A1_NY, nlev=A1_NLEV, seed=41):
    """(row, col, S) in mpg_handle_from_weights' 1-based form.  Row p holds A1_LENGTHS[p % 12] entries; the first four of a non-empty
    row are one id of each band, the rest come from the bands and from A1_POOL ids spread over [0, n_src); the entries of a row are
    then shuffled.  Weights are uniform in [0.2, 1) / row length: positive, so that a masked Regrid without gaps defines every non-empty
    row (valid weight = total weight > 0) and can be held to the typed Regrid bit for bit."""
    rng = np.random.default_rng(seed)
    bands = a1_bands(n_src, nlev)
    lens = np.array([A1_LENGTHS[p % len(A1_LENGTHS)] for p in range(n_dst)], np.int64)
    total = int(lens.sum())
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    within = np.arange(total, dtype=np.int64) - np.repeat(rowptr[:-1], lens)          # position inside the row
    which = np.where(within < 4, within, rng.integers(0, 5, size=total))              # 0..3: that band, 4: the pool
    lo = np.array([b[0] for b in bands] + [0], np.int64)[which]
    width = np.array([b[1] - b[0] for b in bands] + [A1_POOL], np.int64)[which]
    pick = rng.integers(0, 1 << 62, size=total, dtype=np.int64) % width
    col = np.where(which < 4, lo + pick, pick * (n_src // A1_POOL))
    key = rng.random(total) + np.repeat(np.arange(n_dst, dtype=np.float64), lens)     # shuffle inside each row
    order = np.argsort(key, kind="stable")
    col = col[order]
    row = np.repeat(np.arange(1, n_dst + 1, dtype=np.int64), lens)
    S = (0.2 + 0.8 * rng.random(total)) / np.repeat(lens, lens).astype(np.float64)
    assert col.min() >= 0 and col.max() < n_src
    return row.astype(np.int32), (col + 1).astype(np.int32), S, lens


def fill_uniform(torch, t, seed, piece=1 << 30):
    """t (flat, any float dtype) <- i.i.d. uniform in [-SPAN / 2, SPAN / 2), generated in pieces of 2^30 elements."""
    gen = torch.Generator(device=t.device)
    gen.manual_seed(seed)
    for a in range(0, t.numel(), piece):
        t[a:a + piece].uniform_(-SPAN / 2, SPAN / 2, generator=gen)
    return t
