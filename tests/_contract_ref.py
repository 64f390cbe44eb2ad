"""The exact host restatement of include/mpassit_amd.h's "contract by identity" arithmetic (tests/c/contract_ref.c), bound with ctypes,
and what the two test modules that hang from it share: the source arrays, the from_weights pattern and the comparison by bits.

The C file is written from the header's text -- explicit fma() where the header says fma, separate products, sums and quotients
elsewhere -- and built at first use with  gcc -O2 -fPIC -shared -ffp-contract=off  into a temporary directory.  It takes a handle's
own exported pattern (RouteHandle.weights(), .csr(), .pole()) and host arrays; nothing here touches a GPU.

`variant` (REVERSED, MULADD, EPI_MULADD, EPI_SKIP, COLSORT) selects a deliberately wrong recipe; 0 is the contract.

Besides the forward Regrids, the masked recipe and the mesh wind products: the transpose (transpose, transposed, special_g,
transpose_shares, synthetic_transpose_case), the rotation (rotate) and the Grid -> Grid wind chain (wind_destagger, mass_winds,
winds_are_informative)."""
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
        L.cr_apply_transpose.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                         C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int]
        L.cr_rotate.restype = None
        L.cr_rotate.argtypes = [C.c_int64, C.c_int] + [C.c_void_p] * 4
        L.cr_wind_destagger.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 4 + [
            C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]
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


# ---- the transpose, the rotation and the Grid -> Grid wind chain -------------------------------------------------------------------
def transposed(pat):
    """The pattern of A^T as a CSR Pattern: one row per source of `pat`, its entries in ascending (destination point, slot or CSR
    position) order, a nearest handle's weight 1.0.  Built with a stable sort, not with cr_apply_transpose's dealing loop: cr.apply on
    it (the CSR chain in stored order, no epilogue) is a second statement of the transpose's sum, and the source generators (special,
    special_is_informative) work on it as they do on a forward pattern.  Pole caps are not part of it."""
    if pat.nnz:
        keep = (pat.idx >= 0).reshape(-1)
        c = pat.idx.reshape(-1)[keep].astype(np.int64)
        p = np.repeat(np.arange(pat.n_dst, dtype=np.int64), pat.nnz)[keep]
        w = np.ones(c.size) if pat.nnz == 1 else pat.w.reshape(-1)[keep]
    else:
        c = pat.col.astype(np.int64)
        p = np.repeat(np.arange(pat.n_dst, dtype=np.int64), np.diff(pat.rowptr))
        w = pat.val
    order = np.argsort(c, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=pat.n_src))])
    return Pattern(pat.n_dst, pat.n_src, 0, rowptr=rowptr, col=p[order], val=w[order])


def transpose(pat, g, nlev=1, nfields=1, dst_dtype=np.float64, dst_lev_fast=False, g_level_stride=0, variant=0):
    """mpg_regrid_transpose_dev without the pole term.  g: float32 / float64, nfields * nlev planes of n_dst, g_level_stride elements
    apart (0: dense).  Returns ((nfields, nlev, n_src) or, dst_lev_fast, (nfields, n_src, nlev) of dst_dtype, cap [n_src] bool: the
    sources of the CENTER rows that a pole cap adds its term to -- there the result is the segment sum alone)."""
    g = np.ascontiguousarray(g)
    ld = g_level_stride or pat.n_dst
    assert g.dtype in (np.float32, np.float64) and g.size >= (nfields * nlev - 1) * ld + pat.n_dst, (g.dtype, g.size, nfields, nlev, ld)
    dst = _dst(pat.n_src, nlev, nfields, dst_dtype, dst_lev_fast)
    cap = np.zeros(pat.n_src, np.uint8)
    p = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    if pat.nnz:
        w = None if pat.nnz == 1 else pat.w
        handle = (p(pat.idx), p(w), None, None, None)
    else:
        handle = (None, None, p(pat.rowptr), p(pat.col), p(pat.val))
    if pat.pole is not None:
        _, src0, wp, row_len = pat.pole
        src0, wp = np.ascontiguousarray(src0, np.int32), np.ascontiguousarray(wp, np.float64)
        pole = (p(src0), p(wp), src0.size, int(row_len))
    else:
        pole = (None, None, 0, 0)
    rc = lib().cr_apply_transpose(pat.nnz, *handle, pat.n_src, pat.n_dst, g.ctypes.data, int(g.dtype == np.float32), int(g_level_stride), nlev, nfields,
                                  dst.ctypes.data, int(dst.dtype == np.float32), int(dst_lev_fast), *pole, cap.ctypes.data, int(variant))
    assert rc == 0, "contract_ref: rc %d" % rc
    return dst, cap.astype(bool)


def rotate(cosa, sina, u, v):
    """mpg_rotate_winds on copies: (u', v') of u, v [nlev][npts] float64"""
    cosa, sina = (np.ascontiguousarray(a, np.float64).reshape(-1) for a in (cosa, sina))
    u, v = (np.array(a, np.float64, order="C") for a in (u, v))
    assert u.shape == v.shape and u.size % cosa.size == 0 and cosa.size == sina.size
    lib().cr_rotate(cosa.size, u.size // cosa.size, cosa.ctypes.data, sina.ctypes.data, u.ctypes.data, v.ctypes.data)
    return u, v


def wind_destagger(pat1, pat2, cosa, sina, umass, vmass, nlev, dst_type=0, dst_level_stride=0, keep_mass=False):
    """The Grid -> Grid wind chain.  pat1 / pat2: the EDGE1 / EDGE2 patterns (4 slots) or None; cosa / sina [n_mass] or None; umass / vmass
    [nlev][n_mass] float64.  dst_type as MPG_TYPE_*: 0 float64 (the sum as it stands), 1 float32, 2 float64 big-endian, 3 float32
    big-endian.  Returns (U, V, umass', vmass'): U / V (nlev, ld) of float64 / float32 with ld = dst_level_stride or the component's n_dst,
    elements past n_dst NaN (never written); None for a component without a pattern; the rotated mass winds only with keep_mass."""
    n_mass = (pat1 or pat2).n_src
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float64)   # noqa: E731
    cosa, sina, umass, vmass = f(cosa), f(sina), f(umass), f(vmass)
    dt = np.float32 if dst_type & 1 else np.float64
    outs = [None if pat is None else np.full((nlev, dst_level_stride or pat.n_dst), np.nan, dt) for pat in (pat1, pat2)]
    rots = [np.empty((nlev, n_mass)) if keep_mass and cosa is not None else None for _ in range(2)]
    p = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    args = []
    for pat in (pat1, pat2):
        assert pat is None or (pat.nnz == 4 and pat.n_src == n_mass)
        args += [None, None, 0] if pat is None else [p(pat.idx), p(pat.w), pat.n_dst]
    rc = lib().cr_wind_destagger(*args, n_mass, p(cosa), p(sina), p(umass), p(vmass), nlev, p(outs[0]), p(outs[1]), int(dst_type), int(dst_level_stride),
                                 p(rots[0]), p(rots[1]))
    assert rc == 0, "contract_ref: rc %d" % rc
    return outs[0], outs[1], rots[0], rots[1]


# the segment lengths the synthetic transpose handle must hold: they bracket the 4-slot form, TR_SHORT = 16 and a wave of 64 lanes
SYN_LENGTHS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 18, 63, 64, 65, 300)
SYN_N_SRC, SYN_NX, SYN_NY = 41, 401, 1


def synthetic_transpose_case():
    """(row, col, S) 1-based for RouteHandle.from_weights(SYN_N_SRC, SYN_NX, SYN_NY, ...) and the Pattern it must give: 401 destination
    points over 41 sources (not a multiple of 64) whose transposed segments have exactly the SYN_LENGTHS, on sources spread over the
    index range, and 1 to 8 entries on each of the others; a destination's entries are drawn with replacement, so (row, col) pairs repeat
    (the 300-entry source has fewer than 300 distinct rows by construction, and one pair is repeated on purpose in adjacent and in
    separated positions); the entries come in shuffled order, so a row's stored order is not its column order.  Destination point 0
    holds one entry: the padded slots of the register kernels load row 0."""
    rng = np.random.default_rng(77)
    n_dst = SYN_NX * SYN_NY
    special_src = rng.permutation(SYN_N_SRC)[:len(SYN_LENGTHS)]
    length = rng.integers(1, 9, SYN_N_SRC)
    length[special_src] = SYN_LENGTHS
    rows, cols = [], []
    for c in range(SYN_N_SRC):
        r = rng.integers(1, n_dst, int(length[c]))                 # point 0 is given its one entry below
        if length[c] == 5:
            r[:] = (200, 200, 7, 200, 390)                          # one pair three times: adjacent and separated
        rows.append(r)
        cols.append(np.full(r.size, c))
    row, col = np.concatenate(rows), np.concatenate(cols)
    one = int(np.nonzero(length == 1)[0][0])                        # the one-entry source sits on destination point 0
    row[np.nonzero(col == one)[0][0]] = 0
    S = rng.uniform(0.0, 1.0, row.size)
    shuffle = rng.permutation(row.size)
    row, col, S = row[shuffle], col[shuffle], S[shuffle]
    order = np.argsort(row, kind="stable")                          # from_weights keeps the caller's order inside a row
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n_dst))]).astype(np.int64)
    pat = Pattern(SYN_N_SRC, n_dst, 0, rowptr=rowptr, col=col[order], val=S[order])
    return ((row + 1).astype(np.int32), (col + 1).astype(np.int32), S), pat


def segment_lengths(pat):
    """entries per source of the transposed index, [n_src]"""
    return _row_counts(pat)


def special_g(pat, nlev, nfields, seed=0):
    """Grid values for the transpose of `pat`, (nfields, nlev, n_dst): `special` on the transposed pattern, and a NaN at destination
    point 0 of every plane -- the row the padded slots of the register kernels load.  Returns (g, where, the transposed pattern):
    special_is_informative(transposed pattern, g, where, ...) is the check of the result.

    A handle with fewer than 1000 destination points cannot take `special`'s placements: with 40 sources (the synthetic handle) one
    level of one field has 40 outputs, four may be non-finite, and five kinds of a float32 source are (NaN, the infinities,
    +-3.5e38); with 180 points read by six sources each (the composed handle) every non-finite element costs six outputs.  There each
    kind sits once per field, kind j at level (j + f) % nlev, on the points that cost least: points that only the LONGEST segment reads
    where it has eleven of them (one output of a level is lost however many kinds share it; from 17 levels on every kind has a level
    to itself, below that an infinity beside a NaN shows nothing of its own), else the points with the fewest readers.  The random
    picks (_special_share of the elements, any point, no minimum) add the rest."""
    pt = transposed(pat)
    if pt.n_src >= 1000:
        x, where = special(pt, nlev, nfields, seed)
    else:
        x = ordinary(pt.n_src, nlev, nfields, seed)
        rng = np.random.default_rng(991 + 31 * nlev + seed)
        where = {name: np.zeros(x.shape, bool) for name, _ in SPECIALS}
        readers = _row_counts(pt)
        longest = int(np.diff(pt.rowptr).argmax())
        own = pt.col[pt.rowptr[longest]:pt.rowptr[longest + 1]]
        own = rng.permutation(np.unique(own[(readers[own] == 1) & (own != 0)]))
        if own.size < len(SPECIALS):
            read = np.nonzero(readers > 0)[0]
            read = rng.permutation(read[read != 0])
            own = read[np.argsort(readers[read], kind="stable")]
        assert own.size >= len(SPECIALS)
        pick = rng.choice(x.size, size=int(x.size * _special_share(pt)), replace=False)
        for j, e in enumerate(pick):
            name, v = SPECIALS[j % len(SPECIALS)]
            f, k, c = np.unravel_index(e, x.shape)
            _place(x, where, name, v, f, k, c)
        for f in range(nfields):
            for j, (name, v) in enumerate(SPECIALS):
                _place(x, where, name, v, f, (j + f) % nlev, int(own[j]))
    for f in range(nfields):
        for k in range(nlev):
            _place(x, where, "nan", float("nan"), f, k, 0)
    return x, where, pt


def transpose_shares(pat, g, nlev, nfields):
    """{wrong recipe: share of the outputs that can differ whose bits do differ}, reference against reference.  Reversing a segment can
    change a source with two entries or more (fma(w1, x1, round(w0 x0)) against fma(w0, x0, round(w1 x1))) -- three or more where all its
    weights are 1.0 (a nearest handle, mpg_reconstruct_store's values), where two terms add exactly either way; a separate multiply
    and add can change a source with two entries or more, and none whose weights are all 1.0 (every product is exact).  A recipe that can
    change no source of the pattern is not listed."""
    pt = transposed(pat)
    n = np.diff(pt.rowptr)
    unit = np.ones(pat.n_src, bool)
    unit[np.repeat(np.arange(pat.n_src), n)[pt.val != 1.0]] = False
    want, _ = transpose(pat, g, nlev, nfields)
    out = {}
    for name, variant, can in (("segment reversed", REVERSED, n >= np.where(unit, 3, 2)), ("separate multiply and add", MULADD, (n >= 2) & ~unit)):
        if can.any():
            out[name] = float(differs(want, transpose(pat, g, nlev, nfields, variant=variant)[0])[:, :, can].mean())
    return out


def mass_winds(nx, ny, nlev, kind, seed=0):
    """(umass, vmass, {kind: (mask in umass, mask in vmass)}) for the wind chain and the rotation, [nlev][ny * nx] float64: N(0, 12)
    winds kept away from zero.  "special": 0.3 % of the elements replaced by the SPECIALS, and every kind once on the rim of each
    array -- kind j of array a on side (j + 2 a) % 4 of first row, last row, first column, last column, so NaN and both infinities
    sit on every side between the two arrays; the NaN of umass on the first corner and the +Inf of vmass on the last -- so that the halo
    of the first and of the last tile sees them.  One placement per kind and array, no more: a mass point is read by up to four U and
    four V points, and rotated by both components, so on the 19 x 11 grid at one level six non-finite elements already cost 8 % of
    the outputs."""
    rng = np.random.default_rng(515 + 7 * nx + 3 * nlev + seed)
    uv = rng.normal(0.0, 12.0, (2, nlev, ny * nx))
    uv = np.where(np.abs(uv) < 0.5, 0.5, uv)
    where = {name: np.zeros(uv.shape, bool) for name, _ in SPECIALS}
    if kind == "special":
        for j, e in enumerate(rng.choice(uv.size, size=int(0.003 * uv.size), replace=False)):
            a, k, c = np.unravel_index(e, uv.shape)
            _place(uv, where, SPECIALS[j % len(SPECIALS)][0], SPECIALS[j % len(SPECIALS)][1], a, k, c)
        for a in range(2):
            for j, (name, v) in enumerate(SPECIALS):
                t = 3 * j + a
                y, x = ((0, t % nx), (ny - 1, nx - 1 - t % nx), (t % ny, 0), (ny - 1 - t % ny, nx - 1))[(j + 2 * a) % 4]
                if (a, name) == (1, "+inf"):
                    y, x = ny - 1, nx - 1
                _place(uv, where, name, v, a, (j + a) % nlev, y * nx + x)
    return uv[0].copy(), uv[1].copy(), {k: (m[0], m[1]) for k, m in where.items() if m.any()}


def winds_are_informative(pat1, pat2, rotated, where, u, v):
    """Every special kind placed in the mass winds reaches an output of every field it can (rotated: U and V from either array; else U
    from umass, V from vmass), and at least 90 % of the mapped outputs of the reference (float64) are finite.  Returns that share."""
    assert set(where) == set(k for k, _ in SPECIALS), sorted(where)
    for name, (mu, mv) in where.items():
        for pat, masks in ((pat1, (mu, mv) if rotated else (mu,)), (pat2, (mu, mv) if rotated else (mv,))):
            for m in masks:
                assert pat is None or (m.any() and reaches(pat, m)), "special kind %r reaches no output of a component" % name
    fin = float(np.concatenate([np.isfinite(a[:, :pat.n_dst][:, ~pat.unmapped]).reshape(-1) for a, pat in ((u, pat1), (v, pat2)) if pat is not None]).mean())
    assert fin >= 0.9, "only %.1f %% of the special winds' outputs are finite" % (100.0 * fin)
    return fin


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
