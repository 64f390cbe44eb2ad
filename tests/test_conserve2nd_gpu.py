"""Second-order conservative regridding on the GPU (mpg_handle_conserve2nd): the CSR handle against the numpy mirror
target_grid.conserve2nd_rows fed with the library's own unit vectors, csr() pattern and triangles -- rowptr and col identical, val BIT
FOR BIT -- on Mesh -> Mesh (the four cell pairs of tests/_mesh_to_mesh_cases.py, both norms, small compose blocks), Mesh -> Grid (the
regional case) and Grid -> Mesh (small Lambert grids, a 1 x 5 grid whose stencils are all collinear); the re-clip against the parent's
Store; conservation and row sums; dst_frac, masks, determinism, statistics; every consumer against the contract's host restatement; every
refusal; and the accuracy the method is for, through regrid_typed."""
import ctypes as C

import numpy as np
import pytest

import _conserve2nd_cases as CC
import _contract_ref as cr
import _mesh_conserve_ref as MR
import _mesh_to_mesh_cases as MC
from conftest import LAMBERT

pytestmark = pytest.mark.gpu

NORMS = [MR.NORM_DSTAREA, MR.NORM_FRACAREA]
_NAMES = {"geo10_to_vor1500": ("geo10", "vor1500"), "vor2500_to_hex": ("vor2500", "hex_small"), "hex_to_geo10": ("hex_large", "geo10"),
          "varres3000_to_geo8": ("varres3000", "geo8")}
SMALL = ((3, 3), (7, 5), (2, 2), (1, 5))      # cells of the small source grids


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _same(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def world(gpu_lib, regional_case):
    """Device objects by name, first-order handles and second-order handles, each made on first use; all released at the end."""
    from mpassit_amd import regrid as R, synth, target_grid as tg
    syn, obj, first, second = {}, {}, {}, {}

    def get(name):
        if name not in obj:
            if name == "regional":
                syn[name], obj[name] = regional_case[0], R.Mesh.from_mpas(regional_case[0])
            elif name == "regional grid":
                syn[name], obj[name] = regional_case[1], R.Grid.from_target(regional_case[1])
            elif name == "hex":
                g61 = tg.define_target_grid_params("lambert", 61, 41, dx=30000.0, dy=30000.0, **LAMBERT)
                syn[name] = synth.regional_mesh_for_lambert(g61.proj, 61, 41, 1201, margin=0.05, seed=11)    # the hex mesh of test_patch_gpu.py
                obj[name] = R.Mesh.from_mpas(syn[name])
            elif name.startswith("small "):
                px, py = (int(v) for v in name[6:].split("x"))
                syn[name] = tg.define_target_grid_params("lambert", px + 1, py + 1, dx=300000.0, dy=300000.0, **LAMBERT)
                obj[name] = R.Grid.from_target(syn[name])
                assert obj[name].stagger_shape(R.STAGGERLOC_CENTER) == (py, px)
            elif name.startswith("geodesic "):
                syn[name] = CC.accuracy_mesh(int(name[9:]))
                obj[name] = R.Mesh.from_mpas(syn[name])
            else:
                syn[name], obj[name] = MC.mesh(name), R.Mesh.from_mpas(MC.mesh(name))
        return obj[name]

    def store(sname, dname, norm):
        key = (sname, dname, norm)
        if key not in first:
            s, d = get(sname), get(dname)
            if isinstance(s, R.Mesh) and isinstance(d, R.Grid):
                first[key] = R.regrid_store(s, d, R.REGRIDMETHOD_CONSERVE)
            elif isinstance(s, R.Grid):
                first[key] = R.regrid_store_conserve_to_mesh(s, d, norm)
            else:
                first[key] = R.regrid_store_conserve_mesh(s, d, norm)
        return first[key]

    def convert(sname, dname, norm):
        key = (sname, dname, norm)
        if key not in second:
            second[key] = R.conserve_2nd(store(sname, dname, norm), get(sname), get(dname), norm)
        return second[key]

    w = dict(syn=syn, obj=get, store=store, convert=convert, mirror={})
    yield w
    for h in list(second.values()) + list(first.values()):
        h.release()
    for x in obj.values():
        x.destroy()


def _polys(world, name):
    from mpassit_amd import regrid as R, target_grid as tg
    o, s = world["obj"](name), world["syn"][name]
    if isinstance(o, R.Mesh):
        return tg.conserve2nd_polygons_mesh(s.verticesOnCell, o.xyz(R.MESHLOC_NODE), o.xyz(R.MESHLOC_ELEMENT))
    ny, nx = o.stagger_shape(R.STAGGERLOC_CENTER)
    return tg.conserve2nd_polygons_grid(o.xyz(R.STAGGERLOC_CORNER), nx, ny, o.xyz(R.STAGGERLOC_CENTER))


def _neighbours(world, name):
    from mpassit_amd import regrid as R, target_grid as tg
    o = world["obj"](name)
    if isinstance(o, R.Mesh):
        return tg.patch_neighbours_mesh(world["syn"][name].verticesOnCell, o.triangles())
    ny, nx = o.stagger_shape(R.STAGGERLOC_CENTER)
    return tg.patch_neighbours_grid(nx, ny)


def _mirror(world, sname, dname, norm, src_mask=None, rh=None):
    """The mirror on the device handle's own pattern (cached for the unmasked calls)."""
    from mpassit_amd import target_grid as tg
    key = (sname, dname, norm)
    if src_mask is None and rh is None and key in world["mirror"]:
        return world["mirror"][key]
    rp, col, _ = (rh if rh is not None else world["store"](sname, dname, norm)).csr()
    out = tg._conserve2nd_rows(rp, col, _polys(world, sname), _polys(world, dname), _neighbours(world, sname), norm, src_mask)
    if src_mask is None and rh is None:
        world["mirror"][key] = out
    return out


def _assert_is_mirror(out, want, what):
    rp, col, val = out.csr()
    wrp, wcol, wval, info = want
    assert np.array_equal(rp, wrp) and np.array_equal(col, wcol), what + ": the pattern"
    bad = _bits(val) != _bits(wval)
    print("%s: nnz %d, stats %s, %.3f ms; %d of %d values differ, worst %.3e" % (
        what, out.nnz, out.store_stats[1:7], out.store_ms, int(bad.sum()), bad.size, float(np.abs(val - wval).max()) if val.size else 0.0))
    assert not bad.any(), what + ": the values, bit for bit"
    st = out.store_stats
    assert [st[1], st[2], st[3], st[4], st[6]] == info["stats"], (st, info["stats"])


# ---- 1. the handle against the mirror -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", NORMS, ids=["dstarea", "fracarea"])
@pytest.mark.parametrize("name", MR.PAIRS)
def test_mesh_to_mesh_is_the_mirror(world, name, norm):
    from mpassit_amd import regrid as R
    sname, dname = _NAMES[name]
    rh = world["store"](sname, dname, norm)
    before = [a.copy() for a in rh.csr()]
    out = world["convert"](sname, dname, norm)
    assert (out.n_src, out.n_dst, out.nx_dst, out.ny_dst, out.nnz_per_row) == (rh.n_src, rh.n_dst, rh.nx_dst, rh.ny_dst, 0)
    assert out.store_ms > 0.0 and out.store_stats[1] == rh.nnz
    _assert_is_mirror(out, _mirror(world, sname, dname, norm), "%s norm %d" % (name, norm))
    assert _same(before, rh.csr()), "the input handle is untouched"
    rp = rh.csr()[0]
    if name == "hex_to_geo10":
        assert (np.diff(rp) == 0).sum() > 100 and np.diff(rp).max() > 24, "empty rows, rows longer than 24"
        assert np.array_equal(np.diff(out.csr()[0]) == 0, np.diff(rp) == 0), "an empty input row stays empty"
    if name == "varres3000_to_geo8":
        assert np.diff(rp).max() >= 64, "the long-row path"


def test_small_compose_blocks_give_the_same_bytes(world, gpu_lib):
    from mpassit_amd import regrid as R
    sname, dname = _NAMES["varres3000_to_geo8"]
    want = world["convert"](sname, dname, MR.NORM_DSTAREA)
    try:
        gpu_lib.tune("compose_block_rows", 7)
        got = R.conserve_2nd(world["store"](sname, dname, MR.NORM_DSTAREA), world["obj"](sname), world["obj"](dname))
    finally:
        gpu_lib.tune("compose_block_rows", 0)
    assert _same(got.csr(), want.csr()) and got.store_stats[1:7] == want.store_stats[1:7]
    got.release()


def test_mesh_to_grid_is_the_mirror(world):
    rh = world["store"]("regional", "regional grid", MR.NORM_DSTAREA)
    out = world["convert"]("regional", "regional grid", MR.NORM_DSTAREA)
    assert (out.nx_dst, out.ny_dst) == (rh.nx_dst, rh.ny_dst) and (np.diff(rh.csr()[0]) == 0).sum() > 1000, "the unmapped strip"
    _assert_is_mirror(out, _mirror(world, "regional", "regional grid", MR.NORM_DSTAREA), "regional Mesh -> Grid")


@pytest.mark.parametrize("norm", NORMS, ids=["dstarea", "fracarea"])
@pytest.mark.parametrize("cells", SMALL, ids=["%dx%d" % c for c in SMALL])
def test_grid_to_mesh_is_the_mirror(world, cells, norm):
    sname = "small %dx%d" % cells
    rh = world["store"](sname, "hex", norm)
    out = world["convert"](sname, "hex", norm)
    want = _mirror(world, sname, "hex", norm)
    _assert_is_mirror(out, want, "%s -> hex norm %d" % (sname, norm))
    assert rh.nnz > 0
    if cells == (1, 5):     # every stencil is collinear: first order, the pattern of the input and w_q alone
        rp, col, _ = rh.csr()
        orp, ocol, oval = out.csr()
        assert out.store_stats[2] == 0 and out.store_stats[3] == 5 and out.store_stats[4] == 5
        assert np.array_equal(orp, rp) and np.array_equal(ocol, col)
        from mpassit_amd import target_grid as tg
        info = want[3]
        rows = np.repeat(np.arange(rh.n_dst), np.diff(rp))
        div = info["area_d"][rows] if norm == MR.NORM_DSTAREA else tg._c2_seq_sum(info["Aq"], rows, rh.n_dst)[rows]
        assert np.array_equal(_bits(oval), _bits(info["Aq"] / div)), "the values are w_q exactly"
    else:
        assert out.store_stats[2] == cells[0] * cells[1] and out.store_stats[3] == 0


# ---- 2. the re-clip against the parent's Store, the identities ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MR.PAIRS)
def test_reclip_agrees_with_the_store(world, oracle, name):
    """A_q / area(d) against the first-order handle's DSTAREA values, within the project's conservative bar."""
    sname, dname = _NAMES[name]
    tol = MR.answer(oracle, name).tol
    rh = world["store"](sname, dname, MR.NORM_DSTAREA)
    rp, col, val = rh.csr()
    info = _mirror(world, sname, dname, MR.NORM_DSTAREA)[3]
    w = info["Aq"] / info["area_d"][np.repeat(np.arange(rh.n_dst), np.diff(rp))]
    print("%s: re-clip worst |A_q / area(d) - stored| %.3e, bar %.3e" % (name, np.abs(w - val).max(), tol))
    assert np.abs(w - val).max() <= tol


@pytest.mark.parametrize("name", MR.PAIRS)
def test_conservation_and_row_sums(world, oracle, name):
    """sum_j area(d_j) c_(j,e) = A_e, as test_conservation_global_to_global applies the bar, and the first-order row sums."""
    sname, dname = _NAMES[name]
    a = MR.answer(oracle, name)
    out = world["convert"](sname, dname, MR.NORM_DSTAREA)
    rp1, col1, val1 = world["store"](sname, dname, MR.NORM_DSTAREA).csr()
    rp, col, val = out.csr()
    rows, rows1 = np.repeat(np.arange(out.n_dst), np.diff(rp)), np.repeat(np.arange(out.n_dst), np.diff(rp1))
    x = np.random.default_rng(17).normal(size=out.n_src)
    lhs = float((a.area_d * np.bincount(rows, weights=val * x[col], minlength=out.n_dst)).sum())
    info = _mirror(world, sname, dname, MR.NORM_DSTAREA)[3]
    rhs, bar = float((info["Ai"] * x).sum()), a.tol * float((a.area_s * np.abs(x)).sum())
    print("conservation %s: %.3e apart, bar %.3e" % (name, abs(lhs - rhs), bar))
    assert abs(lhs - rhs) <= bar
    cs = np.bincount(col, weights=val * a.area_d[rows], minlength=out.n_src)
    assert np.abs(cs - info["Ai"]).max() <= a.tol * a.area_s.max()
    rs, rs1 = np.bincount(rows, weights=val, minlength=out.n_dst), np.bincount(rows1, weights=val1, minlength=out.n_dst)
    print("row sums %s: worst %.3e" % (name, np.abs(rs - rs1).max()))
    assert np.abs(rs - rs1).max() <= a.tol
    for norm in NORMS:
        o2 = world["convert"](sname, dname, norm)
        assert np.array_equal(_bits(o2.dst_frac()), _bits(world["store"](sname, dname, norm).dst_frac())), "dst_frac is carried over bit for bit"
    assert val.min() < 0.0, "weights can be negative: no limiter"


# ---- 3. masks, determinism ------------------------------------------------------------------------------------------------------------------
def test_masks_and_determinism(world):
    from mpassit_amd import regrid as R
    sname, dname = _NAMES["geo10_to_vor1500"]
    src, dst = world["obj"](sname), world["obj"](dname)
    rh = world["store"](sname, dname, MR.NORM_FRACAREA)
    want = world["convert"](sname, dname, MR.NORM_FRACAREA)
    again = R.conserve_2nd(rh, src, dst, MR.NORM_FRACAREA)
    zero = R.conserve_2nd(rh, src, dst, MR.NORM_FRACAREA, src_mask=np.zeros(rh.n_src, bool))
    assert _same(again.csr(), want.csr()) and again.store_stats[1:7] == want.store_stats[1:7], "two calls, the same bytes"
    assert _same(zero.csr(), want.csr()), "an all-zero mask gives the bytes of no mask"
    # ESMF's order: mask the first-order handle with the ENTRY rule, then convert with the same source mask
    sm = np.zeros(rh.n_src, bool)
    sm[np.random.default_rng(5).choice(rh.n_src, 60, replace=False)] = True
    masked1 = R.mask_handle(rh, src_mask=sm, rule=R.MASKRULE_ENTRY, norm_type=MR.NORM_FRACAREA)
    masked2 = R.conserve_2nd(masked1, src, dst, MR.NORM_FRACAREA, src_mask=sm)
    rp, col, val = masked2.csr()
    assert not sm[col].any(), "no stencil holds a masked id"
    wrp, wcol, wval, info = _mirror(world, sname, dname, MR.NORM_FRACAREA, src_mask=sm, rh=masked1)
    assert np.array_equal(rp, wrp) and np.array_equal(col, wcol) and np.array_equal(_bits(val), _bits(wval))
    assert masked2.store_stats[3] >= 60 and [masked2.store_stats[k] for k in (1, 2, 3, 4, 6)] == info["stats"]
    assert np.array_equal(_bits(masked2.dst_frac()), _bits(masked1.dst_frac()))
    with pytest.raises(Exception):
        R.mask_handle(want, src_mask=sm)          # MPG_MASKRULE_AUTO does not know method 4
    assert R.REGRIDMETHOD_CONSERVE_2ND == 4
    for h in (again, zero, masked1, masked2):
        h.release()
    # Store, convert, release in one call
    one = R.regrid_store_conserve_2nd(src, dst, MR.NORM_FRACAREA)
    assert _same(one.csr(), want.csr())
    one.release()


# ---- 4. the handle under every consumer -----------------------------------------------------------------------------------------------------
def _held(got, want, what):
    import torch
    w = torch.from_numpy(np.ascontiguousarray(want)).cuda()
    g = got.contiguous().reshape(w.shape)
    assert g.dtype == w.dtype, (what, g.dtype, w.dtype)
    it = torch.int64 if g.dtype == torch.float64 else torch.int32
    bad = g.view(it) != w.view(it)
    assert not bool(bad.any()), (what, int(bad.sum()), bad.numel())


def test_consumers_on_the_grid(world):
    import torch
    from mpassit_amd import regrid as R
    rh = world["convert"]("regional", "regional grid", MR.NORM_DSTAREA)
    pat = cr.Pattern.of(rh)
    nlev, nf = 3, 2
    x64 = cr.ordinary(rh.n_src, nlev, nf, 5)
    for sdt, ddt in ((np.float64, np.float64), (np.float32, np.float32)):
        x = cr.to_f32(x64) if sdt == np.float32 else x64
        cf = torch.from_numpy(x).cuda()
        lf = cf.transpose(1, 2).contiguous()
        tdt = torch.float32 if ddt == np.float32 else torch.float64
        want = cr.apply(pat, x, nlev, nf, dst_dtype=ddt)
        for layout, s in ((R.LAYOUT_CELL_FAST, cf), (R.LAYOUT_LEV_FAST, lf)):
            _held(rh.regrid_typed(s.view(-1), nlev=nlev, nfields=nf, layout=layout, out_dtype=tdt), want, ("typed", sdt, ddt, layout))
        _held(rh.regrid_masked(cf.view(-1), nlev=nlev, nfields=nf, out_dtype=tdt), cr.apply_masked(pat, x, nlev, nf, dst_dtype=ddt, flags=1),
              ("masked", sdt, ddt))
        g = cr.to_f32(cr.ordinary(rh.n_dst, nlev, nf, 9)) if sdt == np.float32 else cr.ordinary(rh.n_dst, nlev, nf, 9)
        want64, cap = cr.transpose(pat, g, nlev, nf)
        assert not cap.any()
        _held(rh.regrid_transpose(torch.from_numpy(g).cuda(), nlev=nlev, nfields=nf, out_dtype=tdt), want64.astype(ddt), ("transpose", sdt, ddt))
    rowptr, col, val = rh.csr()
    twin = R.RouteHandle.from_weights(rh.n_src, rh.nx_dst, rh.ny_dst, np.repeat(np.arange(1, rh.n_dst + 1, dtype=np.int32), np.diff(rowptr)),
                                      (col + 1).astype(np.int32), val)
    assert _same(twin.csr(), (rowptr, col, val)), "csr() round-trips through from_weights"
    twin.release()


@pytest.mark.parametrize("pairing", ["m2m", "g2m"])
def test_consumers_on_the_mesh(world, pairing):
    import torch
    from mpassit_amd import regrid as R
    rh = world["convert"](*(_NAMES["varres3000_to_geo8"] if pairing == "m2m" else ("small 7x5", "hex")), MR.NORM_DSTAREA)
    pat = cr.Pattern.of(rh)
    nlev, nf = 3, 2
    x64 = cr.ordinary(rh.n_src, nlev, nf, 7)
    for sdt, ddt in ((np.float64, np.float64), (np.float32, np.float32)):
        x = cr.to_f32(x64) if sdt == np.float32 else x64
        cf = torch.from_numpy(x).cuda()
        lf = cf.transpose(1, 2).contiguous()
        tdt = torch.float32 if ddt == np.float32 else torch.float64
        for layout, lev_fast in ((R.LAYOUT_CELL_FAST, False), (R.LAYOUT_LEV_FAST, True)):
            want = cr.apply(pat, x, nlev, nf, dst_dtype=ddt, dst_lev_fast=lev_fast)
            if pairing == "g2m":
                _held(rh.regrid_csr_to_mesh(cf, nlev=nlev, nfields=nf, layout=layout, out_dtype=tdt), want, (pairing, "csr_to_mesh", sdt, ddt, layout))
        want = cr.apply(pat, x, nlev, nf, dst_dtype=ddt, dst_lev_fast=True)
        _held(rh.regrid_csr_rows(lf, nlev=nlev, nfields=nf, out_dtype=tdt), want, (pairing, "csr_rows", sdt, ddt))


# ---- 5. the accuracy the method is for, through regrid_typed --------------------------------------------------------------------------------
def test_accuracy_on_the_device(world, oracle):
    """RMS error over the destination cells whose sources are all fully covered, geodesic_mesh(8) and (16) onto vor1500: second order below
    first order at both resolutions, and falling by more than 2^1.5 from frequency 8 to 16."""
    import torch
    err = {}
    for freq in CC.ACCURACY_FREQS:
        a, xs, xd = CC.accuracy_case(oracle, freq)
        sname = "geodesic %d" % freq
        h1, h2 = world["store"](sname, "vor1500", MR.NORM_DSTAREA), world["convert"](sname, "vor1500", MR.NORM_DSTAREA)
        f = torch.from_numpy(xs.copy()).cuda()
        y1 = h1.regrid_typed(f, out_dtype=torch.float64).reshape(-1).cpu().numpy()
        y2 = h2.regrid_typed(f, out_dtype=torch.float64).reshape(-1).cpu().numpy()
        rp1, col1, val1 = h1.csr()
        rows1 = np.repeat(np.arange(h1.n_dst), np.diff(rp1))
        full = np.bincount(col1, weights=val1 * a.area_d[rows1], minlength=h1.n_src) >= a.area_s * (1.0 - 1e-9)
        use = (np.bincount(rows1, weights=~full[col1], minlength=h1.n_dst) == 0) & (np.diff(rp1) > 0)
        err[freq] = (float(np.sqrt(np.mean((y1[use] - xd[use]) ** 2))), float(np.sqrt(np.mean((y2[use] - xd[use]) ** 2))))
        print("geodesic_mesh(%d) -> vor1500: %d cells, RMS first order %.4e, second order %.4e" % (freq, int(use.sum()), err[freq][0], err[freq][1]))
        assert use.sum() > 1000 and err[freq][1] < err[freq][0]
    r1, r2 = err[8][0] / err[16][0], err[8][1] / err[16][1]
    print("ratio from 8 to 16: first order %.2f, second order %.2f (bar 2^1.5 = %.2f)" % (r1, r2, 2 ** 1.5))
    assert r2 > 2 ** 1.5


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(world, gpu_lib):
    from mpassit_amd import _lib as L, regrid as R, synth, target_grid as tg
    lib = L.load()
    get = world["obj"]
    sname, dname = _NAMES["geo10_to_vor1500"]
    src, dst = get(sname), get(dname)
    m2m = world["store"](sname, dname, MR.NORM_DSTAREA)
    who = "mpg_handle_conserve2nd"
    h = C.c_void_p()

    def pts(obj, loc=0):
        return R._points(obj, loc, "x")

    def opts(norm=0):
        return L.Conserve2ndOpts(norm_type=norm, src_mask_dev=None)

    def call(rh=m2m, s=None, d=None, op=None, out=h, no_opts=False):
        ps = pts(src) if s is None else s
        pd = pts(dst) if d is None else d
        op = opts() if op is None else op
        return L.handle_conserve2nd(rh._h if rh is not None else None, C.byref(ps), C.byref(pd), None if no_opts else C.byref(op),
                                    C.byref(out) if out is not None else None)

    def refused(rc, want, *words):
        msg = lib.mpg_last_error().decode()
        assert rc == want and who in msg, (rc, want, msg)
        for word in words:
            assert word in msg, msg

    INV, UNS = L.MPG_ERR_INVALID_ARG, L.MPG_ERR_UNSUPPORTED
    # NULL arguments, point sets that break the rules, sizes, the norm
    refused(call(rh=None), INV, "NULL")
    refused(call(out=None), INV, "NULL")
    refused(call(no_opts=True), INV, "NULL")
    pd = pts(dst)
    refused(L.handle_conserve2nd(m2m._h, None, C.byref(pd), C.byref(opts()), C.byref(h)), INV, "NULL")
    refused(L.handle_conserve2nd(m2m._h, C.byref(pd), None, C.byref(opts()), C.byref(h)), INV, "NULL")
    grid = get("regional grid")
    refused(call(s=L.Points(mesh=src._h, meshloc=0, grid=grid._h, staggerloc=0)), INV, "exactly one", "both")
    refused(call(d=L.Points(mesh=None, meshloc=0, grid=None, staggerloc=0)), INV, "exactly one", "neither")
    refused(call(s=pts(src, R.MESHLOC_NODE)), INV, "MPG_MESHLOC_ELEMENT")
    refused(call(d=pts(dst, R.MESHLOC_NODE)), INV, "MPG_MESHLOC_ELEMENT")
    refused(call(d=pts(grid, R.STAGGERLOC_EDGE1)), INV, "MPG_STAGGERLOC_CENTER")
    refused(call(s=pts(get("geo8"))), INV, "n_src = 1002", "642")
    refused(call(d=pts(get("geo8"))), INV, "n_dst = 1500", "642")
    refused(call(op=opts(7)), INV, "norm_type", "MPG_NORM_DSTAREA")
    # the method, the kind
    bil = R.regrid_store_mesh(src, dst)
    refused(call(rh=bil), INV, "MPG_REGRIDMETHOD_CONSERVE")
    second = world["convert"](sname, dname, MR.NORM_DSTAREA)
    refused(call(rh=second), INV, "MPG_REGRIDMETHOD_CONSERVE")
    # a grid without CORNER coordinates (the check precedes the sizes: any grid made from centres alone)
    lon, lat = np.meshgrid(-110.0 + 2.0 * np.arange(6), 30.0 + 2.0 * np.arange(5))
    bare = R.Grid(lon, lat)
    m2g = world["store"]("regional", "regional grid", MR.NORM_DSTAREA)
    refused(call(rh=m2g, s=pts(get("regional")), d=pts(bare)), INV, "CORNER", "destination")
    g2m = world["store"]("small 7x5", "hex", MR.NORM_DSTAREA)
    refused(call(rh=g2m, s=pts(bare), d=pts(get("hex"))), INV, "CORNER", "source")
    # a periodic source grid (the rings do not wrap)
    per = R.Grid.from_target(tg.define_target_grid_params("lat-lon", nx=25, ny=13, stand_lon=0.0, is_regional=False))
    refused(call(rh=g2m, s=pts(per), d=pts(get("hex"))), UNS, "MPG_GRID_PERIODIC_I")
    # maxEdges > 12: the same cells in a wider verticesOnCell
    import dataclasses
    g8 = MC.mesh("geo8")
    wide = R.Mesh.from_mpas(dataclasses.replace(g8, verticesOnCell=np.pad(g8.verticesOnCell, ((0, 0), (0, 13 - g8.verticesOnCell.shape[1])))))
    self8 = R.regrid_store_conserve_mesh(get("geo8"), get("geo8"))
    refused(call(rh=self8, s=pts(wide), d=pts(get("geo8"))), UNS, "maxEdges 13 > 12")
    refused(call(rh=self8, s=pts(get("geo8")), d=pts(wide)), UNS, "maxEdges 13 > 12")
    wide.destroy()
    # a source window, a mesh cut to a grid, a localized handle
    g2 = tg.define_target_grid_params("lambert", 41, 31, dx=30000.0, dy=30000.0, **LAMBERT)      # a mesh larger than its grid: the handle references
    m2 = R.Mesh.from_mpas(synth.regional_mesh_for_lambert(g2.proj, 41, 31, 3001, margin=0.3, seed=3))   # a proper part of the cells
    grid2 = R.Grid.from_target(g2)
    win = R.regrid_store(m2, grid2, R.REGRIDMETHOD_CONSERVE)
    first, end = win.source_range()
    assert 0 < first < end <= m2.nCells
    assert call(rh=win, s=pts(m2), d=pts(grid2)) == 0, "the same call without a window"
    L.check(lib.mpg_handle_release(h))
    h = C.c_void_p()
    m2.set_source_window(first, end - first)
    refused(call(rh=win, s=pts(m2), d=pts(grid2), out=h), UNS, "source window", "mpg_mesh_set_source_window")
    m2.set_source_window(0, m2.nCells)
    win.release()
    m2.destroy()
    grid2.destroy()
    cut = R.Mesh.from_mpas(world["syn"]["regional"], window_grid=grid)
    refused(call(rh=m2g, s=pts(cut), d=pts(grid)), UNS, "mpg_mesh_create_window", "whole mesh")
    cut.destroy()
    twin = R.conserve_2nd(self8, get("geo8"), get("geo8"))
    assert twin.store_stats[2] == 642
    twin.release()
    self8.localize()
    refused(call(rh=self8, s=pts(get("geo8")), d=pts(get("geo8"))), UNS, "localized or rebased")
    assert h.value is None, "a refused call leaves *out alone"
    # (a fixed conservative handle and a conservative handle with pole terms are made by no Store: those two refusals are the entry point's
    # text alone.)  The wrappers' own checks, and the library still works afterwards
    with pytest.raises(ValueError):
        R.conserve_2nd(m2m, "mesh", dst)
    with pytest.raises(ValueError):
        R.regrid_store_conserve_2nd(grid, grid)
    again = R.conserve_2nd(m2m, src, dst)
    assert _same(again.csr(), second.csr())
    for x in (again, bil, self8):
        x.release()
    per.destroy()
    bare.destroy()
