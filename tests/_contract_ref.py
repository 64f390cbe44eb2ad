"""The exact host restatement of include/mpassit_amd.h's "contract by identity" arithmetic (tests/c/contract_ref.c), bound with ctypes,
and what the two test modules that hang from it share: the source arrays, the from_weights pattern and the comparison by bits.

The C file is written from the header's text -- explicit fma() where the header says fma, separate products, sums and quotients
elsewhere -- and built at first use with  gcc -O2 -fPIC -shared -ffp-contract=off  into a temporary directory.  It takes a handle's
own exported pattern (RouteHandle.weights(), .csr(), .pole()) and host arrays; nothing here touches a GPU.

`variant` (REVERSED, MULADD, EPI_MULADD, EPI_SKIP, COLSORT) selects a deliberately wrong recipe; 0 is the contract."""
import atexit
import ctypes as C
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "contract_ref.c")
REVERSED, MULADD, EPI_MULADD, EPI_SKIP, COLSORT = 1, 2, 4, 8, 16

_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="contract_ref_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "contract_ref.so")
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", SRC, "-o", so, "-lm"], check=True)
        L = C.CDLL(so)
        L.cr_fma.restype = C.c_double
        L.cr_fma.argtypes = [C.c_double] * 3
        L.cr_fma_vec.argtypes = [C.c_void_p] * 4 + [C.c_int64]
        L.cr_apply_fixed.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int]
        L.cr_apply_csr.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int]
        L.cr_apply_masked.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int,
                                      C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_double, C.c_double,
                                      C.c_double, C.c_double]
        L.cr_wind_pair.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_int]
        _lib = L
    return _lib


def fma(a, b, c):
    return lib().cr_fma(float(a), float(b), float(c))


def fma_vec(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    a, b, c = (np.ascontiguousarray(x) for x in (a, b, c))
    out = np.empty(a.shape)
    lib().cr_fma_vec(a.ctypes.data, b.ctypes.data, c.ctypes.data, out.ctypes.data, a.size)
    return out


# ---- a handle's pattern -------------------------------------------------------------------------------------------------------
class Pattern:
    """What a handle exports, on the host: fixed (nnz 1 / 3 / 4: idx, w [n_dst][nnz], idx -1 = unmapped) or CSR (nnz 0: rowptr, col, val
    in stored order), and the pole caps of a periodic Grid -> Grid handle."""

    def __init__(self, n_src, n_dst, nnz, idx=None, w=None, rowptr=None, col=None, val=None, pole=None):
        self.n_src, self.n_dst, self.nnz = int(n_src), int(n_dst), int(nnz)
        if nnz:
            self.idx, self.w = np.ascontiguousarray(idx, np.int32).reshape(n_dst, nnz), np.ascontiguousarray(w, np.float64).reshape(n_dst, nnz)
            self.unmapped = self.idx[:, 0] < 0
            self.used = np.unique(self.idx[~self.unmapped])
        else:
            self.rowptr, self.col, self.val = (np.ascontiguousarray(rowptr, np.int64), np.ascontiguousarray(col, np.int32),
                                               np.ascontiguousarray(val, np.float64))
            self.unmapped = np.diff(self.rowptr) == 0
            self.used = np.unique(self.col)
        self.pole = pole

    # the getters of a RouteHandle, for the references that read a handle (tests/_masked_ref.py)
    nnz_per_row = property(lambda self: self.nnz)

    def weights(self):
        return self.idx, self.w

    def csr(self):
        return self.rowptr, self.col, self.val

    @classmethod
    def of(cls, rh):
        if rh.nnz_per_row == 0:
            rowptr, col, val = rh.csr()
            return cls(rh.n_src, rh.n_dst, 0, rowptr=rowptr, col=col, val=val)
        idx, w = rh.weights()
        dst, src0, wp, row_len = rh.pole()
        return cls(rh.n_src, rh.n_dst, rh.nnz_per_row, idx=idx, w=w, pole=(dst, src0, wp, row_len) if len(dst) else None)


def _dst(n_dst, nlev, nfields, dtype, lev_fast):
    return np.empty((nfields, n_dst, nlev) if lev_fast else (nfields, nlev, n_dst), dtype)


def _src(src, pat, nlev, nfields):
    src = np.ascontiguousarray(src)
    assert src.dtype in (np.float32, np.float64) and src.size == nfields * nlev * pat.n_src, (src.dtype, src.size, nfields, nlev, pat.n_src)
    return src


def _offsets(offset, nfields):
    off = np.ascontiguousarray(np.broadcast_to(np.asarray(offset, np.float64), (nfields,)))
    return off


def apply(pat, src, nlev=1, nfields=1, src_lev_fast=False, dst_dtype=np.float64, dst_lev_fast=False, epilogue=True, scale=1.0, offset=0.0,
          variant=0):
    """The unmasked Regrid of a pattern without its pole caps.  src: float32 / float64, nfields slabs of [lev][src] (or [src][lev]);
    returns (nfields, nlev, n_dst) or, dst_lev_fast, (nfields, n_dst, nlev) of dst_dtype.  epilogue=False is mpg_regrid_dev (the sum as it
    stands); otherwise (dst type) fma(acc, scale, offset) with `offset` a scalar or one value per field."""
    src = _src(src, pat, nlev, nfields)
    dst = _dst(pat.n_dst, nlev, nfields, dst_dtype, dst_lev_fast)
    off = _offsets(offset, nfields)
    tail = (src.ctypes.data, int(src.dtype == np.float32), int(src_lev_fast), nlev, nfields, dst.ctypes.data, int(dst.dtype == np.float32),
            int(dst_lev_fast), int(epilogue), float(scale), off.ctypes.data, int(variant))
    if pat.nnz:
        rc = lib().cr_apply_fixed(pat.idx.ctypes.data, pat.w.ctypes.data, pat.nnz, pat.n_src, pat.n_dst, *tail)
    else:
        rc = lib().cr_apply_csr(pat.rowptr.ctypes.data, pat.col.ctypes.data, pat.val.ctypes.data, pat.n_src, pat.n_dst, *tail)
    assert rc == 0, "contract_ref: rc %d" % rc
    return dst


def apply_masked(pat, src, nlev=1, nfields=1, src_lev_fast=False, dst_dtype=np.float64, flags=1, missing_value=0.0, src_mask=None,
                 min_valid_frac=0.5, fill_value=float("nan"), scale=1.0, offset=0.0):
    """mpg_regrid_masked_dev's recipe; returns (nfields, nlev, n_dst).  flags: 1 = NaN is missing, 2 = missing_value is missing."""
    src = _src(src, pat, nlev, nfields)
    dst = _dst(pat.n_dst, nlev, nfields, dst_dtype, False)
    mask = None if src_mask is None else np.ascontiguousarray(src_mask, np.uint8)
    p = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    fixed = (p(pat.idx), p(pat.w), None, None, None) if pat.nnz else (None, None, p(pat.rowptr), p(pat.col), p(pat.val))
    rc = lib().cr_apply_masked(pat.nnz, *fixed, pat.n_src, pat.n_dst, src.ctypes.data, int(src.dtype == np.float32), int(src_lev_fast), nlev, nfields,
                               dst.ctypes.data, int(dst.dtype == np.float32), int(flags), float(missing_value), p(mask), float(min_valid_frac),
                               float(fill_value), float(scale), float(offset))
    assert rc == 0, "contract_ref: rc %d" % rc
    return dst


def wind_pair(mode, pat_u, pat_v, u, v, c, s, nlev, dst_dtype=np.float64, dst_lev_fast=False, tangential=True):
    """mode "mesh": (ue, ve) = (a c - b s, a s + b c), or (a, b) with c = s = None; mode "edges": un = a c + b s and, tangential,
    ut = b c - a s.  a, b: the float64 Regrids of u through pat_u and v through pat_v with epilogue (1, 0); +0.0 wherever either
    pattern leaves the point unmapped or empty; one cast.  u, v: [nlev][n_src of their pattern], float32 or float64."""
    a = apply(pat_u, u, nlev, 1, False, np.float64, dst_lev_fast, True, 1.0, 0.0)
    b = apply(pat_v, v, nlev, 1, False, np.float64, dst_lev_fast, True, 1.0, 0.0)
    un = np.ascontiguousarray(pat_u.unmapped | pat_v.unmapped, np.uint8)
    n = pat_u.n_dst
    o0 = _dst(n, nlev, 1, dst_dtype, dst_lev_fast)[0]
    o1 = np.empty_like(o0) if (mode == "mesh" or tangential) else None
    p = lambda x: None if x is None else x.ctypes.data   # noqa: E731
    c = None if c is None else np.ascontiguousarray(c, np.float64)
    s = None if s is None else np.ascontiguousarray(s, np.float64)
    rc = lib().cr_wind_pair(0 if mode == "mesh" else 1, a.ctypes.data, b.ctypes.data, p(c), p(s), un.ctypes.data, n, nlev, int(dst_lev_fast),
                            o0.ctypes.data, p(o1), int(o0.dtype == np.float32))
    assert rc == 0
    return (o0, o1) if o1 is not None else (o0,)


def pole_caps(pat, src, nlev, nfields, src_lev_fast, dst_dtype, epilogue, scale, offset):
    """The cap points of a periodic Grid -> Grid handle: fma(wp, m, acc4) then the epilogue, with m the mean of the point's CENTER row
    computed exactly (math.fsum / row_len).

    Returns (points [n_cap], want, bound, must_be_nan, free), the last four (nfields, nlev, n_cap); `want` is float64, before the cast.

    The header does not fix the summation order of the mean, so a cap point gets a bound.  Any order of row_len - 1 additions and one
    division is within (row_len + 1) * 2^-53 * mean|x_row| of the exact mean: each partial sum has magnitude <= sum|x| and rounds once,
    the division once.  The product with wp and the two fma roundings that follow move the result by at most that times |wp| * |scale|,
    plus the roundings of `want` itself, which the caller's one unit in the last place of the destination type covers.  Hence
        (row_len + 3) * 2^-53 * |wp| * mean|x_row| * |scale|  +  1 ulp.
    must_be_nan: the row holds a NaN or infinities of both signs.  A row with one infinity, or infinities of one sign, has that infinity
    as its mean in any order: `want` is then held by its bits.
    free: the one exemption.  Where sum|x_row| itself exceeds the largest float64 (math.fsum overflows), a partial sum can overflow in
    one order and stay finite in another, and nothing is promised; that takes at least two values near 1.7e308 in one row of one plane.
    A row with a single such value cannot overflow in any order and is held to the bound."""
    dst, src0, wp, row_len = pat.pole
    keep = wp != 0.0
    dst, src0, wp = dst[keep], src0[keep], wp[keep]
    s = np.asarray(src, np.float64)
    s = s.reshape(nfields, pat.n_src, nlev).transpose(0, 2, 1) if src_lev_fast else s.reshape(nfields, nlev, pat.n_src)
    acc4 = apply(pat, src, nlev, nfields, src_lev_fast, np.float64, False, False)[:, :, dst]
    rows = sorted(set(int(r) for r in src0))
    mean, mabs, nan, loose = {}, {}, {}, {}
    for r in rows:
        x = s[:, :, r:r + row_len]
        mean[r] = np.empty((nfields, nlev))
        mabs[r] = np.empty((nfields, nlev))
        nan[r] = np.zeros((nfields, nlev), bool)
        loose[r] = np.zeros((nfields, nlev), bool)
        for f in range(nfields):
            for k in range(nlev):
                row = x[f, k]
                if np.isnan(row).any() or (np.isposinf(row).any() and np.isneginf(row).any()):
                    nan[r][f, k], mean[r][f, k], mabs[r][f, k] = True, np.nan, np.nan
                elif np.isinf(row).any():
                    mean[r][f, k], mabs[r][f, k] = row[np.isinf(row)][0], np.inf
                else:
                    try:
                        mabs[r][f, k] = math.fsum(np.abs(row)) / row_len
                        mean[r][f, k] = math.fsum(row) / row_len
                    except OverflowError:                     # sum|x| beyond the largest float64: see `free` above
                        mean[r][f, k], mabs[r][f, k], loose[r][f, k] = 0.0, np.inf, True
    m = np.stack([mean[int(r)] for r in src0], axis=-1)
    ma = np.stack([mabs[int(r)] for r in src0], axis=-1)
    must_nan = np.stack([nan[int(r)] for r in src0], axis=-1)
    free = np.stack([loose[int(r)] for r in src0], axis=-1)
    acc = fma_vec(wp[None, None, :], m, acc4)
    off = _offsets(offset, nfields)[:, None, None]
    want = fma_vec(acc, scale, off) if epilogue else acc
    with np.errstate(invalid="ignore", over="ignore"):
        bound = (row_len + 3) * 2.0 ** -53 * np.abs(wp)[None, None, :] * ma * abs(scale if epilogue else 1.0)
    return dst, want, bound, must_nan, free


# ---- comparison by bits -------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def differs(got, want):
    """elementwise: the bits differ and not both are NaN (payloads are not part of the contract)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    return (bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))


def same(got, want):
    return not differs(got, want).any()


def swap(a):
    """the big-endian bytes of a little-endian array, in an array of the same dtype"""
    return np.ascontiguousarray(a).byteswap()


# ---- sources ------------------------------------------------------------------------------------------------------------------
F32_MIN_SUB = float(np.float32(1.401298464324817e-45))
SPECIALS = (("nan", float("nan")), ("+inf", float("inf")), ("-inf", float("-inf")), ("-0.0", -0.0), ("f64 subnormal", 3.0e-310),
            ("+1.7e308", 1.7e308), ("-1.7e308", -1.7e308), ("+3.5e38", 3.5e38), ("-3.5e38", -3.5e38), ("1e-42", 1.0e-42),
            ("smallest f32 subnormal", F32_MIN_SUB))


def ordinary(n_src, nlev, nfields, seed=0):
    """N(280, 30) shifted away from zero, (nfields, nlev, n_src) float64"""
    x = np.random.default_rng(1000 * nlev + 7 + seed).normal(280.0, 30.0, (nfields, nlev, n_src))
    return np.where(np.abs(x) < 1.0, 1.0, x)


def _row_counts(pat):
    """how many stored entries read each source, [n_src]"""
    cols = pat.idx[~pat.unmapped].reshape(-1) if pat.nnz else pat.col
    return np.bincount(cols[cols >= 0], minlength=pat.n_src)


def _special_share(pat):
    """Seven of the eleven kinds make a sum non-finite, so a row of L entries stays finite with probability about (1 - 0.0064)^L.  For the
    reference to stay informative (at least 90 % finite outputs) the share is 1 % up to five entries per row and 5 % / L beyond: the
    conservative rows of a grid much coarser than its mesh hold 60 entries and more."""
    per_row = pat.nnz if pat.nnz else pat.col.size / max(1, int((~pat.unmapped).sum()))
    return min(0.01, 0.05 / max(1.0, per_row))


def _heavy_sources(pat, count):
    """Sources that serve more than 0.2 % of the rows (at least 8).  The rim of a grid under nearest-neighbour points far outside it
    serves a fifth of a global mesh: one special element there would decide the finite share by itself, so such sources take no
    random special."""
    return count > max(8.0, 0.002 * max(1, int((~pat.unmapped).sum())))


def _place(x, where, name, v, f, k, c):
    """element (f, k, c) becomes the special value `name`, and belongs to no other kind"""
    for other in where.values():
        other[f, k, c] = False
    x[f, k, c] = v
    where[name][f, k, c] = True


def special(pat, nlev, nfields, seed=0, with_nan=True):
    """`ordinary` with about 1 % of the elements (_special_share) replaced by the SPECIALS.  On top of the random picks, which avoid
    _heavy_sources: every kind sits, in EVERY field, on a source the pattern reads; source 0 and source n_src - 1 of plane (0, 0) are
    special (finite kinds: these two may be heavy); one (field, level) plane of a source that 2 to 8 rows share is poisoned (NaN, or
    +Inf without NaN) with its other levels left finite.  A row of a thousand entries and more (the from_weights pattern) is non-finite
    at most levels of such a run: those rows are checked by the ordinary runs.
    Returns (array, {kind: boolean mask of its elements}); special_is_informative() is the check of the result."""
    x = ordinary(pat.n_src, nlev, nfields, seed)
    rng = np.random.default_rng(4242 + 31 * nlev + seed)
    kinds = [k for k in SPECIALS if with_nan or k[0] != "nan"]
    count = _row_counts(pat)
    heavy = _heavy_sources(pat, count)
    pick = rng.choice(x.size, size=max(len(kinds), int(x.size * _special_share(pat))), replace=False)
    pick = pick[~heavy[pick % pat.n_src]]
    flat, where = x.reshape(-1), {}
    for j, (name, v) in enumerate(kinds):
        sel = pick[j::len(kinds)]
        flat[sel] = v
        where[name] = np.zeros(x.size, bool)
        where[name][sel] = True
        where[name] = where[name].reshape(x.shape)
    few = np.nonzero((count >= 2) & (count <= 8))[0]              # shared by several rows; failing that, by as few above one as there are
    if few.size == 0 and (count >= 2).any():
        few = np.nonzero(count == count[count >= 2].min())[0]
    shared = int(few[few.size // 2]) if few.size else int(count.argmax()) if count.any() else -1
    # every kind in every field on a source of its own that the pattern reads, away from the three sources set below
    taken = (0, pat.n_src - 1, shared)
    cand = np.setdiff1d(pat.used[~heavy[pat.used]], taken)
    if cand.size < len(kinds):
        cand = np.setdiff1d(pat.used, taken) if np.setdiff1d(pat.used, taken).size else pat.used
    cand = rng.permutation(cand)
    for f in range(nfields):
        for j, (name, v) in enumerate(kinds):
            _place(x, where, name, v, f, (j // cand.size + f) % nlev, int(cand[j % cand.size]))
    _place(x, where, "smallest f32 subnormal", F32_MIN_SUB, 0, 0, 0)
    _place(x, where, "-0.0", -0.0, 0, 0, pat.n_src - 1)
    if shared >= 0:
        _place(x, where, kinds[0][0], kinds[0][1], nfields - 1, nlev // 2, shared)
    return x, where


def reaches(pat, mask):
    """Does a special element reach an output?  mask: (nfields, nlev, n_src) or one field's (nlev, n_src).  An element (f, k, c) is read by
    output (f, k, p) of every row p that stores an entry on source c, so it does as soon as c is one of the sources the pattern reads."""
    srcs = np.nonzero(mask.reshape(-1, pat.n_src).any(axis=0))[0]
    return bool(np.isin(srcs, pat.used).any())


def special_is_informative(pat, x, where, nlev, nfields, kinds=None):
    """The two conditions on a special source: every kind reaches an output in every field (each field may be used on its own, as the wind
    calls do), and at least 90 % of the mapped outputs of the reference are finite.  Returns the finite share."""
    names = [k for k, _ in SPECIALS] if kinds is None else kinds
    assert set(where) == set(names), (sorted(where), names)
    for name, m in where.items():
        for f in range(nfields):
            assert reaches(pat, m[f]), "special kind %r reaches no output of field %d" % (name, f)
    fin = float(np.isfinite(apply(pat, x, nlev, nfields)[:, :, ~pat.unmapped]).mean())
    assert fin >= 0.9, "only %.1f %% of the special run's outputs are finite" % (100.0 * fin)
    return fin


# ---- the from_weights pattern -------------------------------------------------------------------------------------------------
FW_N_SRC, FW_NX, FW_NY = 2500, 70, 3


def from_weights_case():
    """(row, col, S) 1-based for RouteHandle.from_weights(FW_N_SRC, FW_NX, FW_NY, ...) and the Pattern it must give: 210 rows (the last
    64-point block is partial) with empty rows, a one-entry row, a row that repeats one column, a stored zero weight, descending and
    shuffled column orders, and rows of 1024, 1025 and 2049 entries that open a 64-row block each -- a row that ends exactly at, just
    past and two chunks past a 1024-entry staging chunk."""
    rng = np.random.default_rng(20240)
    n_dst = FW_NX * FW_NY
    rows = [None] * n_dst
    for p in range(n_dst):
        n = int(rng.integers(2, 9))
        rows[p] = (rng.permutation(FW_N_SRC)[:n], rng.uniform(0.0, 1.0, n))
    empty = np.empty(0, np.int64), np.empty(0)
    for p in (0, 5, 63, 100, 208):
        rows[p] = empty
    rows[1] = (np.array([17]), np.array([0.75]))
    rows[2] = (np.full(5, 1234), rng.uniform(0.0, 1.0, 5))
    c, w = rows[3]
    w = w.copy()
    w[1] = 0.0
    rows[3] = (c, w)
    rows[4] = (np.sort(rng.permutation(FW_N_SRC)[:6])[::-1].copy(), rng.uniform(0.0, 1.0, 6))
    rows[209] = (np.array([FW_N_SRC - 1, 0, 77, 3]), rng.uniform(0.0, 1.0, 4))
    for p, n in ((64, 1024), (128, 1025), (192, 2049)):
        rows[p] = (rng.permutation(FW_N_SRC)[:n], rng.uniform(0.0, 2.0 / n, n))
    row = np.concatenate([np.full(len(c), p + 1, np.int32) for p, (c, _) in enumerate(rows)])
    col = np.concatenate([np.asarray(c, np.int32) + 1 for c, _ in rows]).astype(np.int32)
    S = np.concatenate([w for _, w in rows])
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int64)
    return (row, col, S), Pattern(FW_N_SRC, n_dst, 0, rowptr=rowptr, col=col - 1, val=S)


def synthetic_fixed(nnz, n_src=4001, n_dst=2000, seed=5):
    """a fixed pattern without a Store: random distinct sources, U(0, 1) weights normalised per row, every 17th point unmapped"""
    rng = np.random.default_rng(seed + nnz)
    idx = np.stack([rng.permutation(n_src)[:nnz] for _ in range(n_dst)]).astype(np.int32)
    w = rng.uniform(0.0, 1.0, (n_dst, nnz))
    w /= w.sum(axis=1, keepdims=True)
    idx[::17] = -1
    w[::17] = 0.0
    return Pattern(n_src, n_dst, nnz, idx=idx, w=w)


EPI, EPI_SHARP = (9.81, -300.0), (9.81, -2700.0)


# ---- can the inputs tell the contract from its neighbours? ----------------------------------------------------------------------
def recipe_shares(pat, src, nlev, nfields, src_lev_fast=False):
    """{wrong recipe: share of the compared outputs whose bits differ from the contract's}, reference against reference, on one source
    array.  Only the recipes that can differ on this kind of pattern are listed: slot order and separate multiply / add need at least
    three entries (nnz 3, 4, CSR), the column order a CSR pattern with a row that is not ascending.  The multiply-then-add epilogue runs
    at EPI_SHARP: at (9.81, -300) on N(280, 30) data the product (about 2750) and the result (about 2450) share a binade, the offset is
    a multiple of their unit in the last place, and the two recipes differ only on the few sums below 238.6 whose result drops under
    2048 -- under 1 % of a 3- or 4-point average.  An offset of -2700 cancels most of the product, so the product's rounding shows in
    nearly every result.  The share at EPI (9.81, -300) is returned as information under a key ending in "[info]".  "Skipped at (1, 0)"
    differs only where a sum is -0.0, which a chain from +0.0 never is: for 3- and 1-slot patterns it gets an all -0.0 source, and its
    share is over the mapped points whose weights are all non-negative."""
    def share(variant, **kw):
        a = apply(pat, src, nlev, nfields, src_lev_fast, variant=0, **kw)
        b = apply(pat, src, nlev, nfields, src_lev_fast, variant=variant, **kw)
        d = differs(a, b)[:, :, ~pat.unmapped]
        return float(d.mean()) if d.size else 0.0
    out = {}
    if pat.nnz != 1:
        out["slots reversed"] = share(REVERSED)
        out["separate multiply and add"] = share(MULADD)
    out["epilogue as acc * scale + offset"] = share(EPI_MULADD, scale=EPI_SHARP[0], offset=EPI_SHARP[1])
    out["epilogue as acc * scale + offset at (9.81, -300) [info]"] = share(EPI_MULADD, scale=EPI[0], offset=EPI[1])
    if pat.nnz in (1, 3):
        zeros = np.full(nfields * nlev * pat.n_src, -0.0)
        a = apply(pat, zeros, nlev, nfields, src_lev_fast)
        b = apply(pat, zeros, nlev, nfields, src_lev_fast, variant=EPI_SKIP)
        qual = ~pat.unmapped & ~np.signbit(pat.w).any(axis=1)
        d = differs(a, b)[:, :, qual]
        out["epilogue skipped at (1, 0)"] = float(d.mean()) if d.size else 0.0
    if pat.nnz == 0 and (np.diff(pat.col) < 0)[np.setdiff1d(np.arange(pat.col.size - 1), pat.rowptr[1:-1] - 1)].any():
        out["CSR row in ascending-column order"] = share(COLSORT)
    return out


def to_f32(x):
    """the float32 source set: values beyond float32's range become infinities, 1e-42 a float32 subnormal"""
    with np.errstate(over="ignore", under="ignore"):
        return np.ascontiguousarray(x, np.float64).astype(np.float32)


# ---- the patterns of the small Stores, saved ------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contract_patterns.npz")
GOLDEN_NAMES = ("narrow 3", "narrow 1", "narrow csr", "pole 4")


def golden_patterns():
    """{name: Pattern} of the Stores of tests/test_contract_gpu.py that are small enough to keep in the repository: the tiny mesh under the
    19 x 11 grid (bilinear, nearest, conservative) and the periodic 72 x 36 grid CENTER -> EDGE2 without its cap list, as Pattern.of()
    gives them.  test_contract_gpu.py checks that the live Stores still give these; when a Store changes on purpose,
    tests/golden/make_contract_patterns.py (needs a GPU) writes the file again."""
    z = np.load(GOLDEN)
    out = {}
    for name in GOLDEN_NAMES:
        n_src, n_dst, nnz = (int(v) for v in z[name + "/shape"])
        if nnz:
            out[name] = Pattern(n_src, n_dst, nnz, idx=z[name + "/idx"], w=z[name + "/w"])
        else:
            out[name] = Pattern(n_src, n_dst, 0, rowptr=z[name + "/rowptr"], col=z[name + "/col"], val=z[name + "/val"])
    return out
