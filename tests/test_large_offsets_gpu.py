"""The Regrid apply kernels at element offsets past 2^31 and 2^32 ("Offsets beyond 32 bits", names the case of every kernel).

Every case asserts its precondition in integers before it launches anything, writes into a NaN-filled buffer between canary bands
(_oracle_compare.Banded, the result one element into a 128-byte line), checks the canaries and that every element is finite, and
compares EVERY element with the float64 / int64 torch reference of tests/_large_offsets_ref.py (the handle's own weights; the bar of
tests/test_csr_rows_apply_gpu.py, row by row; sources i.i.d. uniform in [-40, 40), so a read of any wrong element is an error of order 1).
Where the project claims equal bits they are asserted: rows / csr_rows against regrid_typed(LEV_FAST) transposed, masked without gaps
against typed.  Scale 1 and offset 0 throughout (fma(x, 1.0, 0.0) is exact: the issue's bar holds as it stands).

  A  source side, file order (c * nlev):   A1 CSR from_weights, 78.2 M sources x 55;  A2 Grid -> Mesh (4 and 1 entries) from an 8848 x 8848
     grid (float32) and a 6256 x 6256 one (float64), each buffer read in plane order as well;  A3 3 entries from the 4.30 M / 8.46 M-cell geodesic meshes x 512 levels (32-bit row offsets / their fallback) and the staged
     file-order kernel below and at its 4 GiB guard
  B  source side, plane order (k * n_src + c, k * ld + c):   B1 small handles rebased to 39.1 M / 78.2 M sources, and from_weights
     handles whose ids sit at the top of that range;  B2 source level strides of 39.1 M / 78.2 M elements (to_mesh, csr_to_mesh, transpose)
  C  destination side (p * nlev, k * P + p, k * ld + p):   C1 6256 x 6256 and 8848 x 8848 grids x 55;  C2 pitched results;  C3 to_mesh onto
     the 4.30 M-cell mesh x 512
  and the pole fix on a periodic global grid of 40.5 M points (both sides large)

Which kernel served a call is pinned through the knobs ("lf_variant", "a3_staged") and read back where the library records it
(kernel_choice, tile_stats); the row gather's choice between 32-bit offsets and its fallback is a function of n_src * nlev alone and
leaves no record: the test asserts the product's side of the guard in integers and runs both kernels through the knob.

What the float64 sizes reach: 55 planes of 39.1 M elements span 2^31 elements (17.2 GB), but 54 * 39.1 M + c passes 2^31 only for
c >= 3.6e7 -- with the low ids of a small handle the float64 cases of B1, B2 and C2 cross 2^32 in BYTES and 2^31 in extent only; element
offsets past 2^31 are the float32 cases' (from level 28 on), B1's handles with ids at the top, and the zeros of the transpose's last plane.

No case needs more than about 48 GB; a case the device cannot hold is skipped with both numbers (a skipped case is not done)."""
import gc

import numpy as np
import pytest

import _large_offsets_ref as LR
from _oracle_compare import Banded

pytestmark = pytest.mark.gpu

NLEV = 55
N39, N78 = 39_100_000, 78_200_000
T31, T32 = 1 << 31, 1 << 32
LAMBERT = dict(ref_lat=38.5, ref_lon=-97.5, truelat1=38.5, truelat2=38.5, stand_lon=-97.5)
GB = 1e9


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _tidy(gpu_lib):
    import torch
    yield
    gpu_lib.tune("lf_variant", -1)
    gpu_lib.tune("a3_staged", -1)
    gc.collect()
    torch.cuda.empty_cache()


def _need(torch, nbytes, what):
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if nbytes > free:
        pytest.skip("%s needs %.1f GB of device memory, %.1f GB are free" % (what, nbytes / GB, free / GB))


def _bits(torch, t):
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def _all_finite(torch, t, what, piece=1 << 30):
    t = t.reshape(-1)
    for a in range(0, t.numel(), piece):
        bad = int((~torch.isfinite(t[a:a + piece])).sum())
        assert bad == 0, "%s: %d elements of [%d, %d) are NaN / Inf (an unwritten element?)" % (what, bad, a, min(a + piece, t.numel()))


def _same_bits(torch, a, b, what, piece=1 << 30):
    a, b = a.reshape(-1), b.reshape(-1)
    assert a.dtype == b.dtype and a.numel() == b.numel(), what
    for o in range(0, a.numel(), piece):
        ne = int((_bits(torch, a[o:o + piece]) != _bits(torch, b[o:o + piece])).sum())
        assert ne == 0, "%s: %d elements of [%d, %d) differ in bits" % (what, ne, o, min(o + piece, a.numel()))


def _rows_are_planes_transposed(torch, rows, planes, P, nlev, what):
    """rows [P][nlev] has the bits of planes [nlev][P] transposed."""
    r, q = rows.reshape(P, nlev), planes.reshape(nlev, P)
    step = max(1, (1 << 28) // nlev)
    for p0 in range(0, P, step):
        ne = int((_bits(torch, r[p0:p0 + step]) != _bits(torch, q[:, p0:p0 + step].t().contiguous())).sum())
        assert ne == 0, "%s: %d elements of points [%d, %d) differ in bits" % (what, ne, p0, min(p0 + step, P))


def _run(torch, n, dt, call, what):
    """call(out) writes n elements of dt into a banded, NaN-filled buffer; canaries and finiteness are checked.  -> the Banded."""
    band = Banded(torch, n, dt, shift=1)
    out = call(band.res)
    assert out.data_ptr() == band.ptr(), what
    torch.cuda.synchronize()
    band.assert_canaries(what)
    _all_finite(torch, band.res, what)
    return band


def _entries(W, p):
    """The (source id, weight) list of destination point p, in stored order ([] for an unmapped point / an empty row)."""
    if W.kind == "csr":
        b, e = int(W.rowptr[p]), int(W.rowptr[p + 1])
        return list(zip(W.col[b:e].tolist(), W.val[b:e].tolist()))
    idx = W.idx[p].tolist()
    return [] if idx[0] < 0 else list(zip([max(c, 0) for c in idx], W.w[p].tolist()))


def _spot_check(torch, W, src, nlev, lev_fast, stride, points, what):
    """The reference's own indexing at these sizes: a few of its elements against Python integers and floats, one source element at a
    time (src[int]: a pointer offset, no index kernel)."""
    flat = src.reshape(-1)
    for p in points:
        ref = LR.apply_ref(W, flat, nlev, lev_fast, stride, p, p + 1, dst_rows=True)[0].tolist()
        for k in (0, nlev // 2, nlev - 1):
            acc = 0.0
            for c, w in _entries(W, p):
                acc = acc + w * float(flat[c * nlev + k if lev_fast else k * stride + c])
            assert ref[k] == acc, "%s: the reference's element (%d, %d) is %r, element by element it is %r" % (what, p, k, ref[k], acc)


def _top_points(W, n=3):
    """Destination points that reference the highest source ids."""
    if W.kind == "csr":
        pos = W.col.topk(min(n, W.col.numel())).indices.cpu().numpy()
        return [int(r) for r in np.searchsorted(W.rowptr.cpu().numpy(), pos, side="right") - 1]
    return [int(p) for p in W.idx.max(dim=1).values.topk(min(n, W.n_dst)).indices.tolist()]


def _check(torch, W, band, src, nlev, lev_fast, what, stride=None, dst_rows=False, dst_stride=None):
    worst = LR.compare(W, band.res, src.reshape(-1), nlev, lev_fast, stride=stride, dst_rows=dst_rows, dst_stride=dst_stride, what=what)
    print("%s: largest difference %.3g of its bar" % (what, worst))
    return worst


def _source(torch, n, dt, seed, device="cuda"):
    src = torch.empty(n, dtype=dt, device=device)
    return LR.fill_uniform(torch, src, seed)


# ---- shared objects --------------------------------------------------------------------------------------------------------------------
class _Geo:
    """A global geodesic mesh and a 256 x 65 lat-lon grid (0.03 degrees) laid over its highest-numbered cells."""

    def __init__(self, torch, R, freq):
        from mpassit_amd import synth
        self.m = synth.geodesic_mesh(freq)
        self.mesh = R.Mesh.from_mpas(self.m)
        top = slice(self.m.nCells - 1000, self.m.nCells)
        lat0, lon0 = float(np.degrees(self.m.latCell[top]).mean()), float(np.degrees(self.m.lonCell[top]).mean())
        nx, ny, d = 256, 65, 0.03
        xe, ye = lon0 + (np.arange(nx + 1) - nx / 2) * d, lat0 + (np.arange(ny + 1) - ny / 2) * d
        lon_c, lat_c = np.meshgrid(xe, ye)
        lon, lat = np.meshgrid(0.5 * (xe[:-1] + xe[1:]), 0.5 * (ye[:-1] + ye[1:]))
        self.grid = R.Grid(lon, lat, lon_c, lat_c)
        self.rh = R.regrid_store(self.mesh, self.grid, R.REGRIDMETHOD_BILINEAR)
        assert self.rh.nnz_per_row == 3 and self.rh.n_src == self.m.nCells and (self.rh.nx_dst, self.rh.ny_dst) == (nx, ny)
        self.W = LR.Weights.from_handle(torch, self.rh)
        assert bool((self.W.idx[:, 0] >= 0).all()), "the grid lies inside the global mesh"

    def close(self):
        self.rh.release()
        self.grid.destroy()
        self.mesh.destroy()


@pytest.fixture(scope="module")
def geo656(gpu_lib):
    import torch
    from mpassit_amd import regrid as R
    g = _Geo(torch, R, 656)
    assert g.m.nCells == 4_303_362
    yield g
    g.close()


@pytest.fixture(scope="module")
def geo920(gpu_lib):
    import torch
    from mpassit_amd import regrid as R
    g = _Geo(torch, R, 920)
    assert g.m.nCells == 8_464_002
    yield g
    g.close()


class _BigGrid:
    """A library-made n x n Lambert grid (300 m) and two regional hex meshes: `over` (about 2500 cells, covers the grid's domain: the
    source of the Mesh -> Grid handles) and `inside` (70 x 59 cells inside the domain whose last row lies in the grid's last rows: the
    destination of the Grid -> Mesh handles)."""

    def __init__(self, R, n):
        from mpassit_amd import synth, target_grid as tg
        self.n = n
        self.g = tg.define_target_grid_params("lambert", n + 1, n + 1, dx=300.0, dy=300.0, arrays=False, **LAMBERT)
        self.grid = R.Grid.from_proj(self.g, fill_target=False)
        assert (self.grid.nx, self.grid.ny) == (n, n)
        self.m_over = synth.regional_mesh_for_lambert(self.g.proj, n, n, 2500, margin=0.03, seed=7)
        spacing = (n - 12.0) / (69 * 3.0 ** 0.5 / 2.0)
        self.m_inside = synth.regional_hex_mesh(self.g.proj, 6.0, 6.0, 59, 70, spacing, seed=8, jitter=0.02)
        self.mesh_over, self.mesh_inside = R.Mesh.from_mpas(self.m_over), R.Mesh.from_mpas(self.m_inside)

    def close(self):
        self.mesh_over.destroy()
        self.mesh_inside.destroy()
        self.grid.destroy()


@pytest.fixture(scope="module")
def grid6256(gpu_lib):
    from mpassit_amd import regrid as R
    b = _BigGrid(R, 6256)
    yield b
    b.close()


@pytest.fixture(scope="module")
def grid8848(gpu_lib):
    from mpassit_amd import regrid as R
    b = _BigGrid(R, 8848)
    yield b
    b.close()


@pytest.fixture(scope="module")
def small(gpu_lib):
    """Small handles of every kind on objects of their own (nothing shared with the Store cache of other modules): Mesh -> Grid bilinear
    (3), nearest (1), conservative (CSR), CENTER -> EDGE1 (4) on a 120 x 70 Lambert grid under a 6000-cell hex mesh; Grid -> Mesh bilinear (4),
    nearest (1) and conservative (CSR) onto a 3000-cell mesh inside it."""
    from mpassit_amd import regrid as R, synth, target_grid as tg
    g = tg.define_target_grid_params("lambert", 121, 71, dx=30000.0, dy=30000.0, arrays=False, **LAMBERT)
    grid = R.Grid.from_proj(g, fill_target=False)
    m_over = synth.regional_mesh_for_lambert(g.proj, 120, 70, 6000, margin=0.04, seed=17)
    m_in = synth.regional_mesh_for_lambert(g.proj, 120, 70, 3000, margin=-0.05, seed=18)
    mesh_over, mesh_in = R.Mesh.from_mpas(m_over), R.Mesh.from_mpas(m_in)
    made = []

    def fresh(kind):
        """The Store's handle of that kind.  One that a test rebased has left the Store cache (the next call builds it again); one that was
        only released is parked there and comes back as it was."""
        rh = {"m2g3": lambda: R.regrid_store(mesh_over, grid, R.REGRIDMETHOD_BILINEAR),
              "m2g1": lambda: R.regrid_store(mesh_over, grid, R.REGRIDMETHOD_NEAREST_STOD),
              "m2gc": lambda: R.regrid_store(mesh_over, grid, R.REGRIDMETHOD_CONSERVE),
              "g2g4": lambda: R.regrid_store_grid(grid, R.STAGGERLOC_EDGE1),
              "g2m4": lambda: R.regrid_store_to_mesh(grid, mesh_in, R.REGRIDMETHOD_BILINEAR),
              "g2m1": lambda: R.regrid_store_to_mesh(grid, mesh_in, R.REGRIDMETHOD_NEAREST_STOD),
              "g2mc": lambda: R.regrid_store_conserve_to_mesh(grid, mesh_in)}[kind]()
        made.append(rh)
        return rh

    yield dict(fresh=fresh, grid=grid, nx=120, ny=70)
    for rh in made:
        if rh._h:
            rh.release()
    mesh_over.destroy()
    mesh_in.destroy()
    grid.destroy()


# ---- A1: CSR, file order -----------------------------------------------------------------------------------------------------------------
class _Compact:
    """A CSR handle's matrix on its referenced sources only, for _masked_ref (which works on host arrays of n_src columns)."""

    def __init__(self, rh):
        self.rowptr, col, self.val = rh.csr()
        self.ids = np.unique(col)
        self.col = np.searchsorted(self.ids, col).astype(np.int32)
        self.n_src, self.n_dst, self.nnz_per_row = int(self.ids.size), rh.n_dst, 0

    def csr(self):
        return self.rowptr, self.col, self.val


def test_a1_csr_file_order(gpu_lib):
    import torch
    from _masked_ref import check_masked, masked_ref
    from mpassit_amd import regrid as R
    nlev, n_src, P = LR.A1_NLEV, LR.A1_NSRC, LR.A1_NX * LR.A1_NY
    _need(torch, 4 * n_src * nlev + 2 * GB, "A1")
    row, col, S, lens = LR.a1_columns()
    rh = R.RouteHandle.from_weights(n_src, LR.A1_NX, LR.A1_NY, row, col, S)
    assert rh.nnz_per_row == 0 and rh.n_dst == P and np.array_equal(np.diff(rh.csr()[0]), lens)
    assert (rh.source_range()[1] - 1) * nlev + nlev - 1 >= T32
    W = LR.Weights.from_handle(torch, rh)
    assert W.max_id * nlev + nlev - 1 == n_src * nlev - 1 >= T32
    src = _source(torch, n_src * nlev, torch.float32, 101)                       # [cell][lev]
    _spot_check(torch, W, src, nlev, True, n_src, _top_points(W) + [0, P - 1], "A1")
    typed = {}
    for ddt in (torch.float32, torch.float64):
        typed[ddt] = _run(torch, nlev * P, ddt, lambda o: rh.regrid_typed(src, nlev=nlev, layout=R.LAYOUT_LEV_FAST, out_dtype=ddt, out=o), "A1 typed")
        _check(torch, W, typed[ddt], src, nlev, True, "A1 regrid_typed(LEV_FAST) %s" % ddt)
        rows = _run(torch, nlev * P, ddt, lambda o: rh.regrid_csr_rows(src.view(1, n_src, nlev), nlev=nlev, out_dtype=ddt, out=o), "A1 csr_rows")
        _check(torch, W, rows, src, nlev, True, "A1 regrid_csr_rows %s" % ddt, dst_rows=True)
        _rows_are_planes_transposed(torch, rows.res, typed[ddt].res, P, nlev, "A1 regrid_csr_rows against regrid_typed(LEV_FAST)")
        msk = _run(torch, nlev * P, ddt, lambda o: rh.regrid_masked(src, nlev=nlev, layout=R.LAYOUT_LEV_FAST, fill_value=0.0, out_dtype=ddt, out=o),
                   "A1 masked, no gaps")
        _same_bits(torch, msk.res, typed[ddt].res, "A1 regrid_masked without gaps against regrid_typed")
        del rows, msk
    # 15 % NaN, against _masked_ref on the referenced sources (gathered with int64 offsets)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    for a in range(0, src.numel(), 1 << 30):
        piece = src[a:a + (1 << 30)]
        piece[torch.rand(piece.numel(), device="cuda", generator=gen) < 0.15] = float("nan")
    cm = _Compact(rh)
    ids = torch.as_tensor(cm.ids.astype(np.int64), device="cuda")
    src_c = src[LR.src_offsets(torch, ids, nlev, True, n_src, False)].to(torch.float64).cpu().numpy()      # [nlev][referenced]
    assert 0.10 < np.isnan(src_c).mean() < 0.20
    ref = masked_ref(cm, src_c)
    fill = -9999.0
    for ddt in (torch.float32, torch.float64):
        msk = _run(torch, nlev * P, ddt, lambda o: rh.regrid_masked(src, nlev=nlev, layout=R.LAYOUT_LEV_FAST, fill_value=fill, out_dtype=ddt, out=o),
                   "A1 masked, 15 % NaN")
        edge = check_masked(msk.res.cpu().numpy().reshape(nlev, P), ref, fill, "A1 masked, 15 %% NaN, %s" % ddt)
        assert ref.defined.any() and (~ref.defined).any() and edge < 0.01 * ref.defined.size
        del msk
    rh.release()


# ---- A2: Grid -> Mesh, 4 and 1 entries: file order, and the same buffer read in plane order ----------------------------------------
@pytest.mark.parametrize("size", [8848, 6256])
def test_a2_grid_to_mesh(request, size):
    """8848^2 sources, float32: c * nlev and k * n_src + c pass 2^32.  6256^2 sources, float64 (17.2 GB): both pass 2^31, and the float64
    entry point runs k_apply1 / k_applyN<4> there.  The destination cells reach into the grid's last rows, so the ids sit at the top."""
    import torch
    from mpassit_amd import regrid as R
    b, nlev = request.getfixturevalue("grid%d" % size), NLEV
    n_src = b.n * b.n
    sdt, thr = (torch.float32, T32) if size == 8848 else (torch.float64, T31)
    assert n_src == (78_287_104 if size == 8848 else 39_137_536)
    _need(torch, (4 if size == 8848 else 8) * n_src * nlev + 2 * GB, "A2")
    src = _source(torch, n_src * nlev, sdt, 102)                                  # [point][lev], and read again as [lev][point]
    for method, nnz in ((R.REGRIDMETHOD_BILINEAR, 4), (R.REGRIDMETHOD_NEAREST_STOD, 1)):
        rh = R.regrid_store_to_mesh(b.grid, b.mesh_inside, method)
        P = rh.n_dst
        assert rh.nnz_per_row == nnz and rh.n_src == n_src and P == b.m_inside.nCells == 70 * 59
        top = rh.source_range()[1] - 1
        assert top * nlev + nlev - 1 >= thr and (nlev - 1) * n_src + top >= thr
        W = LR.Weights.from_handle(torch, rh)
        mapped = W.idx[:, 0] >= 0
        c0 = W.idx[:, 0].to(torch.int64)
        assert int(mapped.sum()) > 0.95 * P and int(((c0 * nlev >= thr) & mapped).sum()) > 0 and int(((c0 * nlev < T31) & mapped).sum()) > 0
        assert int((((nlev - 1) * n_src + c0 >= thr) & mapped).sum()) > 0
        _spot_check(torch, W, src, nlev, True, n_src, _top_points(W), "A2 nnz %d" % nnz)
        _spot_check(torch, W, src, nlev, False, n_src, _top_points(W, 1), "A2 nnz %d" % nnz)
        for ddt in (torch.float32, torch.float64):
            what = "A2 %d^2 %d entries %s" % (size, nnz, ddt)
            typed = _run(torch, nlev * P, ddt, lambda o: rh.regrid_typed(src, nlev=nlev, layout=R.LAYOUT_LEV_FAST, out_dtype=ddt, out=o), what)
            _check(torch, W, typed, src, nlev, True, what + " regrid_typed(LEV_FAST)")
            rows = _run(torch, nlev * P, ddt, lambda o: rh.regrid_rows(src.view(1, n_src, nlev), nlev=nlev, out_dtype=ddt, out=o), what)
            _check(torch, W, rows, src, nlev, True, what + " regrid_rows", dst_rows=True)
            _rows_are_planes_transposed(torch, rows.res, typed.res, P, nlev, what + " regrid_rows against regrid_typed(LEV_FAST)")
            msk = _run(torch, nlev * P, ddt, lambda o: rh.regrid_masked(src, nlev=nlev, layout=R.LAYOUT_LEV_FAST, fill_value=0.0, out_dtype=ddt, out=o), what)
            _check(torch, W, msk, src, nlev, True, what + " regrid_masked")
            _same_bits(torch, msk.res, typed.res, what + " regrid_masked without gaps against regrid_typed")
            del typed, rows, msk
            # plane order: k * n_src + c
            typed = _run(torch, nlev * P, ddt, lambda o: rh.regrid_typed(src, nlev=nlev, out_dtype=ddt, out=o), what)
            _check(torch, W, typed, src, nlev, False, what + " regrid_typed(CELL_FAST)")
            msk = _run(torch, nlev * P, ddt, lambda o: rh.regrid_masked(src, nlev=nlev, fill_value=0.0, out_dtype=ddt, out=o), what)
            _check(torch, W, msk, src, nlev, False, what + " regrid_masked(CELL_FAST)")
            _same_bits(torch, msk.res, typed.res, what + " regrid_masked(CELL_FAST) without gaps against regrid_typed")
            del typed, msk
        if sdt == torch.float64:                                                  # the float64 entry: k_apply1 / k_applyN<4> in plane order, the generic kernels in file order
            for lay, levf in ((R.LAYOUT_CELL_FAST, False), (R.LAYOUT_LEV_FAST, True)):
                what = "A2 %d^2 %d entries regrid (float64 entry) layout %d" % (size, nnz, lay)
                band = _run(torch, nlev * P, torch.float64, lambda o: rh.regrid(src, nlev=nlev, layout=lay, out=o), what)
                _check(torch, W, band, src, nlev, levf, what)
                del band
        rh.release()


# ---- A3: 3 entries, file order: 32-bit row offsets, their fallback, the staged kernel and its guard ----------------------------------
def _a3_pre(g, nlev):
    first, end = g.rh.source_range()
    assert end == g.W.max_id + 1
    return g.m.nCells * nlev, (end - 1) * nlev + nlev - 1


def test_a3_row_gather_with_32_bit_offsets(geo656, gpu_lib):
    """4.30 M cells x 512 levels = 2.20e9 elements, in [2^31, 2^32 - 1): k_apply3_lf_rows takes it with its 32-bit premultiplied offsets
    ("lf_variant" 0); k_apply3_lf ("lf_variant" 2) is its cross-check."""
    import torch
    from mpassit_amd import regrid as R
    g, nlev = geo656, 512
    total, last = _a3_pre(g, nlev)
    assert T31 <= total < 0xFFFFFFFF and last >= T31, (total, last)
    assert int((g.W.idx.to(torch.int64) * nlev >= T31).sum()) > 0.25 * g.W.idx.numel()
    _need(torch, 4 * total + 2 * GB, "A3 (4.30 M cells)")
    src = _source(torch, total, torch.float32, 103)
    P = g.rh.n_dst
    _spot_check(torch, g.W, src, nlev, True, g.m.nCells, _top_points(g.W), "A3 4.30 M")
    res = {}
    for lfv in (0, 2, -1):
        gpu_lib.tune("lf_variant", lfv)
        res[lfv] = _run(torch, nlev * P, torch.float32, lambda o: g.rh.regrid_typed(src, nlev=nlev, layout=R.LAYOUT_LEV_FAST, out=o), "A3 lf_variant %d" % lfv)
        _check(torch, g.W, res[lfv], src, nlev, True, "A3 4.30 M cells x 512, lf_variant %d" % lfv)
    rows = _run(torch, nlev * P, torch.float32, lambda o: g.rh.regrid_rows(src.view(1, g.m.nCells, nlev), nlev=nlev, out=o), "A3 rows")
    _check(torch, g.W, rows, src, nlev, True, "A3 4.30 M cells x 512, regrid_rows", dst_rows=True)
    _rows_are_planes_transposed(torch, rows.res, res[-1].res, P, nlev, "A3 regrid_rows against regrid_typed(LEV_FAST)")


def test_a3_staged_kernel_below_and_at_its_guard(geo656, gpu_lib):
    """The staged file-order kernel addresses the source through a buffer descriptor with 32-bit byte offsets: 240 float32 levels are
    4.13e9 bytes, below the guard, with byte offsets past 2^31; 256 levels are at the guard and the call goes through the fallback."""
    import torch
    from mpassit_amd import regrid as R
    g, P = geo656, geo656.rh.n_dst
    _need(torch, 4 * g.m.nCells * 256 + 2 * GB, "A3 staged")
    src = _source(torch, g.m.nCells * 256, torch.float32, 104)
    for nlev in (240, 256):
        total, last = _a3_pre(g, nlev)
        nbytes = 4 * total
        if nlev == 240:
            assert T31 <= nbytes < 0xFFFFFFFF and 4 * last >= T31, (nbytes, last)
        else:
            assert nbytes >= 0xFFFFFFFF and total < 0xFFFFFFFF, nbytes
        s = src[:total]
        gpu_lib.tune("lf_variant", 1)
        staged = _run(torch, nlev * P, torch.float32, lambda o: g.rh.regrid_typed(s, nlev=nlev, layout=R.LAYOUT_LEV_FAST, out=o), "A3 staged %d" % nlev)
        ts, ut_max = g.rh.tile_stats(), g.rh.kernel_choice()[2]
        assert ts is not None and ts[:2] == (64, 8) and 0 < ut_max <= 1024, (ts, ut_max)       # its tile lists exist and fit: only the byte guard can refuse it
        _check(torch, g.W, staged, s, nlev, True, "A3 4.30 M cells x %d, lf_variant 1" % nlev)
        gpu_lib.tune("lf_variant", 0)
        rows = _run(torch, nlev * P, torch.float32, lambda o: g.rh.regrid_typed(s, nlev=nlev, layout=R.LAYOUT_LEV_FAST, out=o), "A3 rows %d" % nlev)
        _check(torch, g.W, rows, s, nlev, True, "A3 4.30 M cells x %d, lf_variant 0" % nlev)
        if nlev == 256:
            _same_bits(torch, staged.res, rows.res, "A3 at the guard: the staged call is the fallback's result")
        del staged, rows


def test_a3_row_gather_fallback_past_2_32(geo920, gpu_lib):
    """8.46 M cells x 512 levels = 4.33e9 elements >= 2^32: the 32-bit row offsets do not reach, every "lf_variant" must end in k_apply3_lf
    (or, for the staged one, in its refusal and then there) and be right."""
    import torch
    from mpassit_amd import regrid as R
    g, nlev = geo920, 512
    total, last = _a3_pre(g, nlev)
    assert total >= T32 and last >= T32, (total, last)
    assert int((g.W.idx.to(torch.int64) * nlev >= T32).sum()) > 0.25 * g.W.idx.numel()
    _need(torch, 4 * total + 2 * GB, "A3 (8.46 M cells)")
    src = _source(torch, total, torch.float32, 105)
    P = g.rh.n_dst
    _spot_check(torch, g.W, src, nlev, True, g.m.nCells, _top_points(g.W), "A3 8.46 M")
    res = {}
    for lfv in (0, 2, 1, -1):
        gpu_lib.tune("lf_variant", lfv)
        res[lfv] = _run(torch, nlev * P, torch.float32, lambda o: g.rh.regrid_typed(src, nlev=nlev, layout=R.LAYOUT_LEV_FAST, out=o), "A3 lf_variant %d" % lfv)
        _check(torch, g.W, res[lfv], src, nlev, True, "A3 8.46 M cells x 512, lf_variant %d" % lfv)
        _same_bits(torch, res[lfv].res, res[0].res, "A3 past 2^32: every variant is the one fallback kernel")
    rows = _run(torch, nlev * P, torch.float32, lambda o: g.rh.regrid_rows(src.view(1, g.m.nCells, nlev), nlev=nlev, out=o), "A3 rows")
    _check(torch, g.W, rows, src, nlev, True, "A3 8.46 M cells x 512, regrid_rows", dst_rows=True)
    _rows_are_planes_transposed(torch, rows.res, res[-1].res, P, nlev, "A3 regrid_rows against regrid_typed(LEV_FAST)")
    msk = _run(torch, nlev * P, torch.float32, lambda o: g.rh.regrid_masked(src, nlev=nlev, layout=R.LAYOUT_LEV_FAST, fill_value=0.0, out=o), "A3 masked")
    _same_bits(torch, msk.res, res[-1].res, "A3 regrid_masked without gaps against regrid_typed")


# ---- B1: plane order, k * n_src + c ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_b1_plane_order(small, gpu_lib, sdt):
    import torch
    from mpassit_amd import regrid as R
    dt, N = (torch.float64, N39) if sdt == "f64" else (torch.float32, N78)
    nlev = NLEV
    _need(torch, N * nlev * (8 if sdt == "f64" else 4) + 2 * GB, "B1 " + sdt)
    # the small handles keep their low ids: float32, (nlev - 1) * N + c passes 2^31 from level 28 on; float64, 54 * 39.1 M + c stays 3.6e7
    # short of 2^31 in ELEMENTS (the source spans 2^31 elements and 2^34 bytes) -- the handles with ids at the top of the range, below, pass it
    assert nlev * N >= T31 and (nlev - 1) * N * 8 >= T32 if sdt == "f64" else (nlev - 1) * N >= T31 and nlev * N >= T32
    src = _source(torch, N * nlev, dt, 106)                                       # [lev][N]
    for kind in ("m2g3", "g2g4", "m2g1", "m2gc"):
        rh = small["fresh"](kind)
        rh.rebase(0, N)
        assert rh.n_src == N
        W = LR.Weights.from_handle(torch, rh)
        P = rh.n_dst
        assert W.n_src == N and (sdt == "f64" or (nlev - 1) * N + W.max_id >= T31)
        _spot_check(torch, W, src, nlev, False, N, _top_points(W, 1), "B1 " + kind)
        runs = []
        if sdt == "f64":                                                           # the float64 entry: k_apply1, k_applyN, the EPI = false instances
            runs.append(("regrid", -1, lambda o: rh.regrid(src, nlev=nlev, out=o), torch.float64))
        for staged in ((-2, 0) if kind == "m2g3" else (-1,)):                      # 3 entries: lane gather / LDS-staged; else the generic kernels
            runs.append(("regrid_typed a3_staged %d" % staged, staged, lambda o: rh.regrid_typed(src, nlev=nlev, out_dtype=torch.float32, out=o), torch.float32))
            runs.append(("regrid_typed f64 a3_staged %d" % staged, staged, lambda o: rh.regrid_typed(src, nlev=nlev, out_dtype=torch.float64, out=o), torch.float64))
        typed64 = []                                                               # the float64 results of every variant
        for name, staged, call, ddt in runs:
            gpu_lib.tune("a3_staged", staged)
            band = _run(torch, nlev * P, ddt, call, "B1 %s %s" % (kind, name))
            _check(torch, W, band, src, nlev, False, "B1 %s %s, %s sources x %d" % (kind, name, sdt, N))
            if name.startswith("regrid_typed f64"):
                typed64.append(band)
            if kind == "m2g3" and staged == 0:
                assert rh.kernel_choice()[0] == 1 and rh.tile_stats() is not None, "the staged cell-fast kernel (variant 0) served the call"
        gpu_lib.tune("a3_staged", -1)
        msk = _run(torch, nlev * P, torch.float64, lambda o: rh.regrid_masked(src, nlev=nlev, fill_value=0.0, out_dtype=torch.float64, out=o), "B1 masked")
        _check(torch, W, msk, src, nlev, False, "B1 %s regrid_masked" % kind)
        for t64 in typed64:           # (3 entries: the lane gather's and the staged kernel's results)
            _same_bits(torch, msk.res, t64.res, "B1 %s regrid_masked without gaps against regrid_typed" % kind)
        del msk, typed64, band
        rh.release()
    # ids at the TOP of the declared range: k * n_src + c past 2^32 (float32) / 2^31 (float64) -- a fixed 3-entry and a CSR handle of
    # from_weights (positive weights: the masked Regrid defines every point)
    rng = np.random.default_rng(3)
    for per_row in (3, 5):
        P = 1000
        row = np.repeat(np.arange(1, P + 1), per_row)
        col = N - rng.integers(0, 5000, size=row.size)
        rh = R.RouteHandle.from_weights(N, P, 1, row, col, 0.2 + 0.8 * rng.random(row.size))
        assert rh.nnz_per_row == (3 if per_row == 3 else 0)
        W = LR.Weights.from_handle(torch, rh)
        assert (nlev - 1) * N + W.max_id >= (T32 if sdt == "f32" else T31)
        _spot_check(torch, W, src, nlev, False, N, _top_points(W, 1), "B1 top ids")
        bands = []
        for staged in (-2, 0):
            gpu_lib.tune("a3_staged", staged)
            band = _run(torch, nlev * P, torch.float32, lambda o: rh.regrid_typed(src, nlev=nlev, out_dtype=torch.float32, out=o), "B1 top ids")
            _check(torch, W, band, src, nlev, False, "B1 top ids, %d per row, a3_staged %d" % (per_row, staged))
            bands.append(band)
            if per_row == 3 and staged == 0:
                assert rh.kernel_choice()[0] == 1 and rh.tile_stats() is not None, "the staged cell-fast kernel (variant 0) served the call"
        gpu_lib.tune("a3_staged", -1)
        msk = _run(torch, nlev * P, torch.float32, lambda o: rh.regrid_masked(src, nlev=nlev, fill_value=0.0, out_dtype=torch.float32, out=o), "B1 top ids masked")
        _check(torch, W, msk, src, nlev, False, "B1 top ids, %d per row, regrid_masked" % per_row)
        for t in bands:               # (3 per row: the lane gather's and the staged kernel's results)
            _same_bits(torch, msk.res, t.res, "B1 top ids: regrid_masked without gaps against regrid_typed")
        del bands
        if sdt == "f64":
            band = _run(torch, nlev * P, torch.float64, lambda o: rh.regrid(src, nlev=nlev, out=o), "B1 top ids, float64 entry")
            _check(torch, W, band, src, nlev, False, "B1 top ids, %d per row, regrid (float64 entry)" % per_row)
        del band, msk
        rh.release()


# ---- B2: source level strides (k * ld + c) and the transpose ---------------------------------------------------------------------------
def _pitched_source(torch, nlev, ld, n, dt, seed, device="cuda"):
    """nlev planes of n elements, ld apart, in a NaN-filled buffer: (buffer, view [nlev][n])."""
    buf = torch.full(((nlev - 1) * ld + n,), float("nan"), dtype=dt, device=device)
    view = buf.as_strided((nlev, n), (ld, 1))
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    for k in range(nlev):
        view[k].uniform_(-LR.SPAN / 2, LR.SPAN / 2, generator=gen)
    return buf, view


def _transposed(torch, W, N, device="cuda"):
    """The handle's A^T as a CSR Weights over its N declared sources: row c lists the destination points that reference c, ascending."""
    if W.kind == "csr":
        rowptr, col, val = (t.cpu().numpy() for t in (W.rowptr, W.col, W.val))
        pts = np.repeat(np.arange(W.n_dst), np.diff(rowptr))
    else:
        idx, w = W.idx.cpu().numpy(), W.w.cpu().numpy()
        keep = (idx >= 0) & (idx[:, :1] >= 0)
        pts = np.broadcast_to(np.arange(W.n_dst)[:, None], idx.shape)[keep]
        col, val = idx[keep], w[keep]
    order = np.lexsort((np.arange(col.size), col))                # by source, then by entry order (= ascending point, slot)
    rowptr_t = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=N))])
    return LR.Weights(torch, W.n_dst, N, rowptr=rowptr_t, col=pts[order], val=val[order], device=device)


@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_b2_source_level_strides(small, sdt):
    import torch
    from mpassit_amd import regrid as R
    dt, ld = (torch.float64, N39) if sdt == "f64" else (torch.float32, N78)
    nlev, nx, ny = NLEV, small["nx"], small["ny"]
    n_src = nx * ny
    _need(torch, nlev * ld * (8 if sdt == "f64" else 4) + 2 * GB, "B2 " + sdt)
    # float32: k * ld passes 2^31 elements from level 28 on; float64: 54 * 39.1 M stays 3.6e7 elements short of it -- the source spans 2^31
    # elements and k * ld * 8 passes 2^32 BYTES from level 14 on
    assert nlev * ld >= T31 and (nlev - 1) * ld * 8 >= T32 if sdt == "f64" else (nlev - 1) * ld >= T31
    buf, planes = _pitched_source(torch, nlev, ld, n_src, dt, 107)
    src = buf.as_strided((nlev, ny, nx), (ld, nx, 1))
    for kind in ("g2m4", "g2m1", "g2mc"):
        rh = small["fresh"](kind)
        W = LR.Weights.from_handle(torch, rh)
        P = rh.n_dst
        assert rh.n_src == n_src and (sdt == "f64" or (nlev - 1) * ld + W.max_id >= T31)
        fn = rh.regrid_csr_to_mesh if kind == "g2mc" else rh.regrid_to_mesh
        _spot_check(torch, W, buf, nlev, False, ld, _top_points(W, 1), "B2 " + kind)
        for layout, rows in ((R.LAYOUT_CELL_FAST, False), (R.LAYOUT_LEV_FAST, True)):
            for ddt in (torch.float32, torch.float64):
                what = "B2 %s layout %d %s, source stride %d" % (kind, layout, ddt, ld)
                band = _run(torch, nlev * P, ddt, lambda o: fn(src, nlev=nlev, layout=layout, out_dtype=ddt, out=o), what)
                _check(torch, W, band, buf, nlev, False, what, stride=ld, dst_rows=rows)
                del band
    del buf, planes, src


@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_b2_transpose(small, sdt):
    """A^T with a pitched source (grid planes ld apart) and a handle rebased to N sources: the result planes lie N apart, sources that no
    entry references are exactly 0 (their bar is 0).  The two Store handles have at most 16 entries per source (k_tr_short_*); a from_weights
    handle declared with N sources, a few of them referenced by hundreds of rows, runs k_tr_long."""
    import torch
    from mpassit_amd import regrid as R
    dt, N = (torch.float64, N39) if sdt == "f64" else (torch.float32, N78)
    es = 8 if sdt == "f64" else 4
    nlev, nx, ny = NLEV, small["nx"], small["ny"]
    _need(torch, 2 * nlev * N * es + 4 * GB, "B2 transpose " + sdt)
    assert nlev * N - 1 >= T31 and (sdt == "f64" or ((nlev - 1) * N >= T31 and nlev * N >= T32))     # the result's last element (an exact 0.0)
    buf, planes = _pitched_source(torch, nlev, N, nx * ny, dt, 108)               # the grid values, planes N apart as well
    for kind in ("m2g3", "m2gc", "long"):
        if kind == "long":            # k_tr_long: sources with more than 16 transposed entries (one wave each), the LAST source among them
            rng = np.random.default_rng(9)
            P = nx * ny
            hot = np.array([N, N - 1, N - 70_000, 1, 4097])                        # 1-based source ids referenced by hundreds of rows each
            row = np.repeat(np.arange(1, P + 1), 2)
            col = np.stack([hot[rng.integers(0, hot.size, size=P)], N - rng.integers(0, 2_000_000, size=P)], axis=1).reshape(-1)
            rh = R.RouteHandle.from_weights(N, nx, ny, row, col, 0.2 + 0.8 * rng.random(row.size))
            assert rh.nnz_per_row == 0
            nref, longest = rh.transpose_stats()
            assert longest > 16 and nref > hot.size, (nref, longest)
        else:
            rh = small["fresh"](kind)
            rh.rebase(0, N)
        W = LR.Weights.from_handle(torch, rh)
        assert rh.n_dst == nx * ny and rh.n_src == N
        WT = _transposed(torch, W, N)
        assert WT.n_dst == N and WT.max_id < nx * ny and (sdt == "f64" or (nlev - 1) * N + W.max_id >= T31)
        if kind == "long":
            assert W.max_id == N - 1 and int(WT.n[N - 1]) > 16 and nlev * N - 1 >= T31    # the last source is a long one: its store is the result's last element
        src = buf.as_strided((nlev, ny, nx), (N, nx, 1))
        for layout, rows in ((R.LAYOUT_CELL_FAST, False), (R.LAYOUT_LEV_FAST, True)):
            what = "B2 transpose %s layout %d %s, %d sources" % (kind, layout, sdt, N)
            band = _run(torch, nlev * N, dt, lambda o: rh.regrid_transpose(src, nlev=nlev, layout=layout, out=o), what)
            _check(torch, WT, band, buf, nlev, False, what, stride=N, dst_rows=rows)
            view = LR.result_view(band.res, N, nlev, rows)
            tail = view[W.max_id + 1:] if rows else view[:, W.max_id + 1:]
            assert int(torch.count_nonzero(tail)) == 0, what + ": an unreferenced source is not 0"
            del band, view, tail
        rh.release()


# ---- C1: destination side, 39.1 M and 78.3 M points ------------------------------------------------------------------------------------
def _c1(torch, R, gpu_lib, rh, nlev, f64_too, tag):
    """Every entry point and variant of one handle onto a large grid; float32 results, float64 ones as well where asked."""
    P, n_src, nnz = rh.n_dst, rh.n_src, rh.nnz_per_row
    assert (P - 1) * nlev + nlev - 1 >= T31 and (nlev - 1) * P + P - 1 >= T31
    W = LR.Weights.from_handle(torch, rh)
    src = _source(torch, n_src * nlev, torch.float32, 109)                        # read as [lev][cell] and as [cell][lev]
    src64 = src.to(torch.float64) if f64_too and n_src * nlev * 8 < 10 * GB else None
    _spot_check(torch, W, src, nlev, True, n_src, [P - 1, P // 2], tag)
    _spot_check(torch, W, src, nlev, False, n_src, [P - 1, 0], tag)
    for ddt in ((torch.float32, torch.float64) if f64_too else (torch.float32,)):
        _need(torch, 2.2 * P * nlev * (4 if ddt == torch.float32 else 8) + 2 * GB, tag)
        n = P * nlev

        def typed(lay, o):
            return rh.regrid_typed(src, nlev=nlev, layout=lay, out_dtype=ddt, out=o)

        ref_lf = None
        for lay, name, knob in ((R.LAYOUT_CELL_FAST, "cell-fast", "a3_staged"), (R.LAYOUT_LEV_FAST, "file order", "lf_variant")):
            levf = lay == R.LAYOUT_LEV_FAST
            values = (-1,) if nnz != 3 else ((-1, 0, 1, 2) if levf else (-1, -2, 0, 1, 2))      # every 3-entry variant the knob selects
            ref = None
            for v in values:
                gpu_lib.tune(knob, v)
                what = "%s regrid_typed %s %s %d -> %s" % (tag, name, knob, v, ddt)
                band = _run(torch, n, ddt, lambda o: typed(lay, o), what)
                _check(torch, W, band, src, nlev, levf, what)
                gpu_lib.tune(knob, -1)
                if v == -1:
                    ref = band
                del band
            what = "%s regrid_masked %s -> %s" % (tag, name, ddt)
            msk = _run(torch, n, ddt, lambda o: rh.regrid_masked(src, nlev=nlev, layout=lay, fill_value=0.0, out_dtype=ddt, out=o), what)
            _check(torch, W, msk, src, nlev, levf, what)
            _same_bits(torch, msk.res, ref.res, what + " without gaps against regrid_typed")
            del msk
            if levf:
                ref_lf = ref
            del ref
        if nnz == 3:
            assert rh.tile_stats() is not None
        what = "%s %s -> %s" % (tag, "regrid_csr_rows" if nnz == 0 else "regrid_rows", ddt)
        fn = rh.regrid_csr_rows if nnz == 0 else rh.regrid_rows
        rows = _run(torch, n, ddt, lambda o: fn(src.view(1, n_src, nlev), nlev=nlev, out_dtype=ddt, out=o), what)
        _check(torch, W, rows, src, nlev, True, what, dst_rows=True)
        _rows_are_planes_transposed(torch, rows.res, ref_lf.res, P, nlev, what + " against regrid_typed(LEV_FAST)")
        del rows, ref_lf
        if ddt == torch.float64 and src64 is not None:                            # the float64 entry point (EPI = false; k_apply1 / k_applyN cell-fast)
            for lay, name in ((R.LAYOUT_CELL_FAST, "cell-fast"), (R.LAYOUT_LEV_FAST, "file order")):
                what = "%s regrid (float64 entry) %s" % (tag, name)
                band = _run(torch, n, ddt, lambda o: rh.regrid(src64, nlev=nlev, layout=lay, out=o), what)
                _check(torch, W, band, src64, nlev, lay == R.LAYOUT_LEV_FAST, what)
                del band


@pytest.mark.parametrize("method", ["bilinear", "nearest"])
@pytest.mark.parametrize("size", [6256, 8848])
def test_c1_mesh_to_large_grid(request, gpu_lib, size, method):
    import torch
    from mpassit_amd import regrid as R
    b = request.getfixturevalue("grid%d" % size)
    rh = R.regrid_store(b.mesh_over, b.grid, R.REGRIDMETHOD_BILINEAR if method == "bilinear" else R.REGRIDMETHOD_NEAREST_STOD)
    assert rh.n_dst == size * size and rh.nnz_per_row == (3 if method == "bilinear" else 1)
    assert (size == 6256 and rh.n_dst == 39_137_536 and rh.n_dst * NLEV >= T31) or (size == 8848 and rh.n_dst * NLEV >= T32)
    try:
        _c1(torch, R, gpu_lib, rh, NLEV, size == 6256, "C1 %d^2 %s" % (size, method))
    finally:
        rh.release()


def test_c1_center_to_edge1_both_sides_large(grid6256, gpu_lib):
    import torch
    from mpassit_amd import regrid as R
    b = grid6256
    rh = R.regrid_store_grid(b.grid, R.STAGGERLOC_EDGE1)
    assert rh.nnz_per_row == 4 and rh.n_src == 6256 * 6256 and rh.n_dst == 6257 * 6256
    assert (rh.source_range()[1] - 1) * NLEV + NLEV - 1 >= T31 and (NLEV - 1) * rh.n_src + rh.source_range()[1] - 1 >= T31
    try:
        _c1(torch, R, gpu_lib, rh, NLEV, False, "C1 6256^2 CENTER -> EDGE1")
    finally:
        rh.release()


def test_c1_conservative_store(grid6256, gpu_lib):
    import torch
    from mpassit_amd import regrid as R
    b = grid6256
    rh = R.regrid_store(b.mesh_over, b.grid, R.REGRIDMETHOD_CONSERVE)
    assert rh.nnz_per_row == 0 and rh.n_dst == 6256 * 6256
    try:
        _c1(torch, R, gpu_lib, rh, NLEV, True, "C1 6256^2 conservative")
    finally:
        rh.release()


# ---- the pole fix: a periodic global grid of 40.5 M points, both sides large ------------------------------------------------------------------
def test_pole_caps_of_a_large_periodic_grid(gpu_lib):
    """CENTER -> EDGE2 on a global 0.04-degree lat-lon grid (9000 x 4500 mass points, 9000 x 4501 V points): the 4-entry generic kernel, then
    k_pole_fix rewrites the 2 x 9000 V points of the pole rows as their four slots + w_pole * mean(nearest CENTER row).  The north row's
    sources are the last 9000 ids: (n_src - 1) * nlev in file order, (nlev - 1) * n_src + c in plane order, both past 2^31; its results
    sit at (nlev - 1) * n_dst + p.  The cap points' bar: the row's own with one more term (n = 5), plus |w_pole| * row_len * eps64 * max |x| for
    the mean (two summations of row_len terms and a division, each within row_len / 2 * eps64 * max |x|)."""
    import torch
    from mpassit_amd import regrid as R, target_grid as tg
    nlev, nx, ny = NLEV, 9000, 4500
    g = tg.define_target_grid_params("lat-lon", nx=nx + 1, ny=ny + 1, stand_lon=0.0, is_regional=False)
    grid = R.Grid.from_target(g)
    rh = R.regrid_store_grid(grid, R.STAGGERLOC_EDGE2)
    n_src, P = nx * ny, nx * (ny + 1)
    assert rh.nnz_per_row == 4 and rh.n_src == n_src and rh.n_dst == P
    dst, src0, wp, row_len = rh.pole()
    assert row_len == nx and dst.size == 2 * nx and (wp != 0.0).all() and set(src0.tolist()) == {0, n_src - nx}
    assert (n_src - 1) * nlev + nlev - 1 >= T31 and (nlev - 1) * n_src + n_src - 1 >= T31 and (nlev - 1) * P + int(dst.max()) >= T31
    _need(torch, 4 * (n_src + P) * nlev + 6 * GB, "pole caps")
    W = LR.Weights.from_handle(torch, rh)
    src = _source(torch, n_src * nlev, torch.float32, 112)
    cap = torch.zeros(P, dtype=torch.bool, device="cuda")
    dst_t = torch.as_tensor(dst.astype(np.int64), device="cuda")
    cap[dst_t] = True
    Wc = LR.Weights(torch, n_src, dst.size, idx=W.idx[dst_t].cpu().numpy(), w=W.w[dst_t].cpu().numpy(), device="cuda")
    wp_t, north = torch.as_tensor(wp, device="cuda"), torch.as_tensor(src0 != 0, device="cuda")
    bar = (5 + 1.0) * LR.EPS64 * (Wc.sumw + wp_t.abs()) * LR.XMAX + wp_t.abs() * row_len * LR.EPS64 * LR.XMAX
    for lay, name in ((R.LAYOUT_CELL_FAST, "cell-fast"), (R.LAYOUT_LEV_FAST, "file order")):
        levf = lay == R.LAYOUT_LEV_FAST
        what = "pole caps, regrid_typed %s" % name
        band = _run(torch, nlev * P, torch.float32, lambda o: rh.regrid_typed(src, nlev=nlev, layout=lay, out=o), what)
        worst = LR.compare(W, band.res, src, nlev, levf, what=what, skip=cap)
        rows = [src[LR.src_offsets(torch, torch.arange(a, a + nx, dtype=torch.int64, device="cuda"), nlev, levf, n_src, False)].to(torch.float64)
                for a in (0, n_src - nx)]                                            # [nlev][row_len] each
        mean = torch.stack([r.sum(dim=1) / row_len for r in rows])                    # [2][nlev]
        ref = LR.apply_ref(Wc, src, nlev, levf) + wp_t[None, :] * mean[north.long()].t()
        got = LR.result_view(band.res, P, nlev, False)[:, dst_t].to(torch.float64)
        d, tol = (got - ref).abs(), bar[None, :] + LR.F32_ROUND * ref.abs()
        assert bool((d <= tol).all()), "%s: %d cap values beyond their bar, largest %.3g of it" % (what, int((~(d <= tol)).sum()), float((d / tol).max()))
        print("%s: largest difference %.3g of its bar, the caps' %.3g of theirs" % (what, worst, float((d / tol).max())))
        del band
    rh.release()
    grid.destroy()


# ---- C2: pitched results (k * ld + p) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ddt_name", ["f64", "f32"])
def test_c2_pitched_results(small, gpu_lib, ddt_name):
    import torch
    from mpassit_amd import regrid as R
    ddt, ld = (torch.float64, N39) if ddt_name == "f64" else (torch.float32, N78)
    nlev = NLEV
    _need(torch, nlev * ld * (8 if ddt_name == "f64" else 4) + 3 * GB, "C2 " + ddt_name)
    # (float64: 54 * 39.1 M + p stays short of 2^31 elements; the result spans 2^31 elements, k * ld * 8 passes 2^32 bytes from level 14 on)
    assert nlev * ld >= T31 and (nlev - 1) * ld * 8 >= T32 if ddt_name == "f64" else (nlev - 1) * ld >= T31
    for kind in ("m2g3", "g2g4", "m2g1", "m2gc"):
        rh = small["fresh"](kind)
        W = LR.Weights.from_handle(torch, rh)
        P, nx, ny = rh.n_dst, rh.nx_dst, rh.ny_dst
        src = _source(torch, rh.n_src * nlev, torch.float64, 110)
        n = (nlev - 1) * ld + P
        def typed(lay):
            return lambda o: rh.regrid_typed(src, nlev=nlev, layout=lay, out_dtype=ddt, out=o)

        calls = [("regrid_typed", None, -1, typed(R.LAYOUT_CELL_FAST)), ("regrid_typed(LEV_FAST)", None, -1, typed(R.LAYOUT_LEV_FAST)),
                 ("regrid_masked", None, -1, lambda o: rh.regrid_masked(src, nlev=nlev, fill_value=0.0, out_dtype=ddt, out=o))]
        if kind == "m2g3":            # every 3-entry kernel by its knob: lane gather, staged cell-fast; row gather, staged file order, grid-row gather
            calls += [("regrid_typed a3_staged %d" % v, "a3_staged", v, typed(R.LAYOUT_CELL_FAST)) for v in (-2, 0)]
            calls += [("regrid_typed(LEV_FAST) lf_variant %d" % v, "lf_variant", v, typed(R.LAYOUT_LEV_FAST)) for v in (0, 1, 2)]
        if ddt_name == "f64":
            calls.append(("regrid (float64 entry)", None, -1, lambda o: rh.regrid(src, nlev=nlev, out=o)))
        for name, knob, value, call in calls:
            if knob:
                gpu_lib.tune(knob, value)
            what = "C2 %s %s, result stride %d %s" % (kind, name, ld, ddt_name)
            band = Banded(torch, n, ddt, shift=1)
            out = band.res.as_strided((1, nlev, ny, nx), (nlev * ld, ld, nx, 1))
            got = call(out)
            assert got.data_ptr() == band.ptr()
            torch.cuda.synchronize()
            if knob:
                gpu_lib.tune(knob, -1)
                if (knob, value) == ("a3_staged", 0):
                    assert rh.kernel_choice()[0] == 1 and rh.tile_stats() is not None, "the staged cell-fast kernel (variant 0) served the call"
                if (knob, value) == ("lf_variant", 1):
                    assert rh.tile_stats()[:2] == (64, 8) and 0 < rh.kernel_choice()[2] <= 1024, "the staged file-order kernel's lists exist and fit"
            band.assert_canaries(what)
            planes = LR.result_view(band.res, P, nlev, False, ld)
            _all_finite(torch, planes[:, :P], what)
            written = sum(int(torch.isfinite(band.res[a:a + (1 << 30)]).sum()) for a in range(0, n, 1 << 30))
            assert written == nlev * P, "%s: %d elements written, the planes hold %d (the pad of a plane is never written)" % (what, written, nlev * P)
            _check(torch, W, band, src, nlev, "LEV_FAST" in name, what, dst_stride=ld)
            del band, out, got, planes
        rh.release()


# ---- C3: to_mesh onto 4.30 M cells x 512 levels, [cell][lev] ----------------------------------------------------------------------------
def test_c3_to_mesh_onto_4m_cells(geo656):
    import torch
    from mpassit_amd import regrid as R
    g, nlev = geo656, 512
    P = g.m.nCells
    assert P * nlev >= T31
    _need(torch, 2.2 * 4 * P * nlev + 2 * GB, "C3")
    for kind in ("bilinear", "conservative"):
        rh = R.regrid_store_to_mesh(g.grid, g.mesh) if kind == "bilinear" else R.regrid_store_conserve_to_mesh(g.grid, g.mesh)
        assert rh.n_dst == P and rh.n_src == 256 * 65 and rh.nnz_per_row == (4 if kind == "bilinear" else 0)
        W = LR.Weights.from_handle(torch, rh)
        mapped = torch.nonzero(W.n > 0).reshape(-1)
        assert mapped.numel() > 500 and int(mapped.max()) * nlev + nlev - 1 >= T31, "mapped cells beyond element 2^31 of the result"
        src = _source(torch, rh.n_src * nlev, torch.float32, 111)                 # [lev][point]
        fn = rh.regrid_to_mesh if kind == "bilinear" else rh.regrid_csr_to_mesh
        _spot_check(torch, W, src, nlev, False, rh.n_src, [int(mapped.max()), int(mapped.min())], "C3 " + kind)
        what = "C3 %s onto 4.30 M cells x 512, [cell][lev]" % kind
        band = _run(torch, P * nlev, torch.float32, lambda o: fn(src.view(nlev, 65, 256), nlev=nlev, layout=R.LAYOUT_LEV_FAST, out=o), what)
        _check(torch, W, band, src, nlev, False, what, dst_rows=True)
        planes = _run(torch, P * nlev, torch.float32, lambda o: fn(src.view(nlev, 65, 256), nlev=nlev, layout=R.LAYOUT_CELL_FAST, out=o), what)
        _check(torch, W, planes, src, nlev, False, what + " / [lev][cell]")
        _rows_are_planes_transposed(torch, band.res, planes.res, P, nlev, what + ": the two layouts hold the same bits")
        del band, planes
        rh.release()
