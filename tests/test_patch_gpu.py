"""Patch regridding on the GPU (mpg_handle_patch): the CSR handle against the numpy mirror target_grid.patch_rows fed with the library's
own unit vectors, weights() and triangles -- rowptr and col identical, val BIT FOR BIT -- on every geometry pairing; every attempt of the
ladder the Stores reach (A, B on meshes, C on the narrow grids; D is reached by no Store-made handle: tests/c/patch_test.cpp is its test);
the handle under every consumer against the contract's host restatement; the accuracy the method is for, through regrid_typed; and every
refusal."""
import ctypes as C

import numpy as np
import pytest

import _contract_ref as cr
from conftest import LAMBERT

pytestmark = pytest.mark.gpu

SMALL = ((3, 3), (7, 5), (2, 5), (2, 2))      # points of the small source staggers


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _field(xyz):
    x, y, z = xyz
    return np.sin(3 * x + 0.3) * np.cos(2 * y) + z ** 3 + 0.5 * x * z


def _small_grid(tg, px, py, stagger):
    """a Lambert grid (300 km) whose CENTER (stagger 0) or EDGE1 (stagger 1) points are px x py"""
    return tg.define_target_grid_params("lambert", px + 1 - stagger, py + 1, dx=300000.0, dy=300000.0, **LAMBERT)


@pytest.fixture(scope="module")
def world(gpu_lib, regional_case, global_mesh, conus_grid_30km):
    from mpassit_amd import regrid as R, synth, target_grid as tg
    E, EDGE, C_, E1, E2 = R.MESHLOC_ELEMENT, R.MESHLOC_EDGE, R.STAGGERLOC_CENTER, R.STAGGERLOC_EDGE1, R.STAGGERLOC_EDGE2
    syn, obj, pairs = {}, {}, {}

    def mesh(name, m):
        syn[name], obj[name] = m, R.Mesh.from_mpas(m)
        return obj[name]

    def grid(name, g):
        syn[name], obj[name] = g, R.Grid.from_target(g)
        return obj[name]

    rm, rg = regional_case
    mesh("regional", rm), grid("regional grid", rg)
    mesh("global", global_mesh), grid("conus", conus_grid_30km)
    mesh("coarse", synth.geodesic_mesh(1))
    lon, lat = np.meshgrid(-150.0 + 75.0 * np.arange(5), -60.0 + 40.0 * np.arange(4))
    obj["latlon"] = R.Grid(lon, lat)
    mesh("vor2000", synth.global_voronoi_mesh(2000))
    g61 = tg.define_target_grid_params("lambert", 61, 41, dx=30000.0, dy=30000.0, **LAMBERT)
    mesh("hex", synth.mesh_edges(synth.regional_mesh_for_lambert(g61.proj, 61, 41, 1201, margin=0.05, seed=11)))
    grid("g97", tg.define_target_grid_params("lambert", 10, 8, dx=30000.0, dy=30000.0, **LAMBERT))
    # name -> (bilinear handle, src name, src_loc, dst name, dst_loc)
    pairs["regional m2g"] = (R.regrid_store(obj["regional"], obj["regional grid"]), "regional", E, "regional grid", C_)
    pairs["global m2g"] = (R.regrid_store(obj["global"], obj["conus"]), "global", E, "conus", C_)
    pairs["coarse m2g"] = (R.regrid_store(obj["coarse"], obj["latlon"]), "coarse", E, "latlon", C_)
    pairs["m2m"] = (R.regrid_store_mesh(obj["vor2000"], obj["hex"]), "vor2000", E, "hex", E)
    for px, py in SMALL:
        for st, sname in ((C_, "C"), (E1, "E1")):
            gname = "small %dx%d %s" % (px, py, sname)
            grid(gname, _small_grid(tg, px, py, 1 if st == E1 else 0))
            assert obj[gname].stagger_shape(st) == (py, px)
            for loc, lname in ((E, "cells"), (EDGE, "edges")):
                pairs["g2m %dx%d %s %s" % (px, py, sname, lname)] = (R.regrid_store_to_mesh(obj[gname], obj["hex"], staggerloc=st, meshloc=loc),
                                                                     gname, st, "hex", loc)
    pairs["g2g e1"] = (R.regrid_store_grid(obj["g97"], E1), "g97", C_, "g97", E1)
    pairs["g2g e2"] = (R.regrid_store_grid(obj["g97"], E2), "g97", C_, "g97", E2)
    d = dict(syn=syn, obj=obj, pairs=pairs, patched={}, mirror={}, stats=np.zeros(4, np.int64))
    yield d
    for h in list(d["patched"].values()) + [p[0] for p in pairs.values()]:
        h.release()
    for x in obj.values():
        x.destroy()


def _neighbours(world, sname, sloc):
    from mpassit_amd import regrid as R, target_grid as tg
    src = world["obj"][sname]
    if isinstance(src, R.Mesh):
        return tg.patch_neighbours_mesh(world["syn"][sname].verticesOnCell, src.triangles())
    ny, nx = src.stagger_shape(sloc)
    return tg.patch_neighbours_grid(nx, ny)


def _patched(world, name):
    from mpassit_amd import regrid as R
    if name not in world["patched"]:
        rh, sname, sloc, dname, dloc = world["pairs"][name]
        world["patched"][name] = R.patch(rh, world["obj"][sname], world["obj"][dname], src_loc=sloc, dst_loc=dloc)
    return world["patched"][name]


def _mirror(world, name):
    from mpassit_amd import target_grid as tg
    if name not in world["mirror"]:
        rh, sname, sloc, dname, dloc = world["pairs"][name]
        idx, w = rh.weights()
        world["mirror"][name] = tg.patch_rows(idx, w, world["obj"][sname].xyz(sloc), world["obj"][dname].xyz(dloc), _neighbours(world, sname, sloc))
    return world["mirror"][name]


def _pairing_names():
    names = ["regional m2g", "global m2g", "coarse m2g", "m2m"]
    for px, py in SMALL:
        for sname in ("C", "E1"):
            for lname in ("cells", "edges"):
                names.append("g2m %dx%d %s %s" % (px, py, sname, lname))
    return names + ["g2g e1", "g2g e2"]


# ---- 1. the handle against the mirror -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _pairing_names())
def test_handle_is_the_mirror(world, name):
    from mpassit_amd import regrid as R
    rh, sname, sloc, dname, dloc = world["pairs"][name]
    src, dst = world["obj"][sname], world["obj"][dname]
    S = 3 if isinstance(src, R.Mesh) else 4
    assert rh.nnz_per_row == S
    before = [a.copy() for a in rh.weights()]
    out = _patched(world, name)
    want_ptr, want_col, want_val, want_stats = _mirror(world, name)
    stats = out.store_stats
    print("%s: n_src %d, n_dst %d, nnz %d, stats %s, %.3f ms" % (name, rh.n_src, rh.n_dst, out.nnz, stats[1:7], out.store_ms))
    assert (out.n_src, out.n_dst, out.nx_dst, out.ny_dst, out.nnz_per_row) == (rh.n_src, rh.n_dst, rh.nx_dst, rh.ny_dst, 0)
    rowptr, col, val = out.csr()
    assert np.array_equal(rowptr, want_ptr) and out.nnz == want_col.size
    assert np.array_equal(col, want_col)
    bad = np.flatnonzero(_bits(val) != _bits(want_val))
    assert bad.size == 0, (name, bad.size, val.size, float(np.abs(val - want_val).max()))
    assert stats[1:7] == want_stats, (stats, want_stats)
    mapped = before[0][:, 0] >= 0
    assert stats[1] == mapped.sum() and np.array_equal(np.diff(rowptr) > 0, mapped), "an unmapped row is empty, a mapped one is not"
    assert sum(stats[2:6]) == int((before[0][mapped] >= 0).sum()) and stats[6] == np.diff(rowptr).max()
    assert out.store_ms > 0.0
    with pytest.raises(Exception):
        out.dst_frac()
    world["stats"] += np.array(stats[2:6], np.int64)
    # two calls give the same bytes, and rh is as it was
    again = R.patch(rh, src, dst, src_loc=sloc, dst_loc=dloc)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(out.csr(), again.csr()))
    again.release()
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(before, rh.weights()))
    if name == "regional m2g":
        assert (~mapped).sum() == 2401 and stats[3] > 0, "the rim: 2 401 unmapped rows, and ring-2 slots"
    if name == "global m2g":
        assert stats[3] > 0, "valence-4 cells: ring 2"
    if name == "coarse m2g":
        assert rh.n_src in (12, 42) and stats[2] > 0
    if name.startswith("g2m 2x2"):
        assert stats[4] == sum(stats[2:6]) > 0, "four points: degree 1 everywhere"
    if name.startswith("g2m 2x5"):
        # six points in two columns are rank deficient on a plane only: on the sphere the columns are curved in the local frame, the pivot
        # ratio is about (spacing / radius)^2 -- far above 2^-26 -- and the rule serves them with attempt A (tests/c/patch_test.cpp has the
        # planar block that falls to C)
        assert stats[2] == sum(stats[2:6]) > 0


def test_every_attempt_a_store_reaches(world):
    for name in _pairing_names():
        _patched(world, name)
    total = np.zeros(4, np.int64)
    for h in world["patched"].values():
        total += np.array(h.store_stats[2:6], np.int64)
    print("pairs served by A, B, C, D across the file:", total.tolist())
    assert (total[:3] > 0).all()
    assert total[3] == 0, "no Store-made handle reaches D: the host program is its test"


def test_release_before_the_first_regrid(world, gpu_lib):
    import torch
    from mpassit_amd import regrid as R
    o = world["obj"]
    out = R.regrid_store_patch(o["vor2000"], o["hex"])         # Store bilinear, patch, release the bilinear handle
    want = _patched(world, "m2m")
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(out.csr(), want.csr()))
    x = torch.from_numpy(cr.ordinary(out.n_src, 3, 1, 2)[0]).cuda()
    a = out.regrid_csr_to_mesh(x.view(-1), nlev=3)
    b = want.regrid_csr_to_mesh(x.view(-1), nlev=3)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    out.release()


# ---- 2. consumers ---------------------------------------------------------------------------------------------------------------------------
def _held(got, want, what):
    import torch
    w = torch.from_numpy(np.ascontiguousarray(want)).cuda()
    g = got.contiguous().reshape(w.shape)
    assert g.dtype == w.dtype, (what, g.dtype, w.dtype)
    it = torch.int64 if g.dtype == torch.float64 else torch.int32
    bad = g.view(it) != w.view(it)
    assert not bool(bad.any()), (what, int(bad.sum()), bad.numel())


def test_consumers_on_the_grid(world, gpu_lib):
    import torch
    from mpassit_amd import regrid as R, synth, target_grid as tg
    rh = _patched(world, "regional m2g")
    pat = cr.Pattern.of(rh)
    assert pat.nnz == 0 and pat.unmapped.sum() == 2401
    nlev, nf = 5, 2
    x64 = cr.ordinary(rh.n_src, nlev, nf, 5)
    F64, F32 = np.float64, np.float32
    for sdt in (F64, F32):
        x = cr.to_f32(x64) if sdt == F32 else x64
        cf = torch.from_numpy(x).cuda()
        lf = cf.transpose(1, 2).contiguous()
        for ddt in (F64, F32):
            tdt = torch.float32 if ddt == F32 else torch.float64
            want = cr.apply(pat, x, nlev, nf, dst_dtype=ddt)
            for layout, s in ((R.LAYOUT_CELL_FAST, cf), (R.LAYOUT_LEV_FAST, lf)):
                _held(rh.regrid_typed(s.view(-1), nlev=nlev, nfields=nf, layout=layout, out_dtype=tdt), want, ("typed", sdt, ddt, layout))
            # nothing missing: the masked Regrid has the unmasked bits where the row is mapped
            got = rh.regrid_masked(cf.view(-1), nlev=nlev, nfields=nf, out_dtype=tdt).reshape(nf, nlev, -1).cpu().numpy()
            assert np.array_equal(np.ascontiguousarray(got[:, :, ~pat.unmapped]).view(np.uint8), np.ascontiguousarray(want[:, :, ~pat.unmapped]).view(np.uint8))
            _held(rh.regrid_masked(cf.view(-1), nlev=nlev, nfields=nf, out_dtype=tdt), cr.apply_masked(pat, x, nlev, nf, dst_dtype=ddt, flags=1),
                  ("masked", sdt, ddt))
        g = cr.to_f32(cr.ordinary(rh.n_dst, nlev, nf, 9)) if sdt == F32 else cr.ordinary(rh.n_dst, nlev, nf, 9)
        want64, cap = cr.transpose(pat, g, nlev, nf)
        assert not cap.any()
        for ddt in (F64, F32):
            got = rh.regrid_transpose(torch.from_numpy(g).cuda(), nlev=nlev, nfields=nf, out_dtype=torch.float32 if ddt == F32 else torch.float64)
            _held(got, want64.astype(ddt), ("transpose", sdt, ddt))
    # compose(patch, a reconstruct_store handle): accepted, and the composite has the patch handle's rows
    m = synth.mesh_edges(world["syn"]["regional"])
    nE, eoc = synth.edges_on_cell(m)
    rec = R.reconstruct_store(nE, eoc, m.nEdges)
    c = R.compose(rh, rec)
    assert (c.n_src, c.n_dst, c.nnz_per_row) == (m.nEdges, rh.n_dst, 0) and np.array_equal(np.diff(c.csr()[0]) == 0, pat.unmapped)
    c.release()
    rec.release()
    # extrapolate(patch, STOD) fills exactly the 2 401 rows, every other row verbatim
    o = world["obj"]
    full = R.extrapolate(rh, o["regional"], o["regional grid"])
    assert full.store_stats[1] == 2401 and full.nnz_per_row == 0
    fr, fc, fv = full.csr()
    rows = np.flatnonzero(pat.unmapped)
    assert (np.diff(fr)[rows] == 1).all() and (fv[fr[rows]] == 1.0).all()
    keep = np.repeat(~pat.unmapped, np.diff(fr))
    assert np.array_equal(fc[keep], pat.col) and np.array_equal(_bits(fv[keep]), _bits(pat.val))
    full.release()
    # mask_handle(AUTO) takes the ROW rule: one masked source unmaps every row that references it, nothing else changes
    sm = np.zeros(rh.n_src, bool)
    sm[pat.col[pat.col.size // 2]] = True
    auto, row = R.mask_handle(rh, src_mask=sm), R.mask_handle(rh, src_mask=sm, rule=R.MASKRULE_ROW)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(auto.csr(), row.csr()))
    wr, wc, wv, _, st = tg.mask_rows(pat.rowptr, pat.col, pat.val, None, sm, None, tg.MASKRULE_ROW)
    assert st[0] > 0 and np.array_equal(auto.csr()[0], wr) and np.array_equal(auto.csr()[1], wc) and auto.store_stats[1] == st[0]
    auto.release()
    row.release()
    # csr() round-trips through from_weights
    rowptr, col, val = rh.csr()
    twin = R.RouteHandle.from_weights(rh.n_src, rh.nx_dst, rh.ny_dst, np.repeat(np.arange(1, rh.n_dst + 1, dtype=np.int32), np.diff(rowptr)),
                                      (col + 1).astype(np.int32), val)
    tr, tc, tv = twin.csr()
    assert np.array_equal(tr, rowptr) and np.array_equal(tc, col) and np.array_equal(_bits(tv), _bits(val))
    twin.release()


@pytest.mark.parametrize("name", ["m2m", "g2m 7x5 C cells", "g2m 7x5 E1 edges"])
def test_consumers_on_the_mesh(world, name):
    import torch
    from mpassit_amd import regrid as R
    rh = _patched(world, name)
    pat = cr.Pattern.of(rh)
    nlev, nf = 3, 2
    x64 = cr.ordinary(rh.n_src, nlev, nf, 7)
    for sdt, ddt in ((np.float64, np.float64), (np.float32, np.float32), (np.float32, np.float64)):
        x = cr.to_f32(x64) if sdt == np.float32 else x64
        cf = torch.from_numpy(x).cuda()
        lf = cf.transpose(1, 2).contiguous()
        tdt = torch.float32 if ddt == np.float32 else torch.float64
        for layout, lev_fast in ((R.LAYOUT_CELL_FAST, False), (R.LAYOUT_LEV_FAST, True)):
            want = cr.apply(pat, x, nlev, nf, dst_dtype=ddt, dst_lev_fast=lev_fast)
            _held(rh.regrid_csr_to_mesh(cf, nlev=nlev, nfields=nf, layout=layout, out_dtype=tdt), want, (name, "csr_to_mesh", sdt, ddt, layout))
        want = cr.apply(pat, x, nlev, nf, dst_dtype=ddt, dst_lev_fast=True)
        _held(rh.regrid_csr_rows(lf, nlev=nlev, nfields=nf, out_dtype=tdt), want, (name, "csr_rows", sdt, ddt))


# ---- 3. the accuracy the method is for, through regrid_typed --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["global m2g", "regional m2g"])
def test_accuracy_on_the_device(world, name):
    import torch
    rh, sname, sloc, dname, dloc = world["pairs"][name]
    out = _patched(world, name)
    src, dst = world["obj"][sname].xyz(sloc), world["obj"][dname].xyz(dloc)
    f = torch.from_numpy(_field(src)).cuda()
    exact = _field(dst)
    mapped = rh.weights()[0][:, 0] >= 0
    bil = rh.regrid_typed(f, out_dtype=torch.float64).reshape(-1).cpu().numpy()
    pat = out.regrid_typed(f, out_dtype=torch.float64).reshape(-1).cpu().numpy()
    eb, ep = np.abs(bil - exact)[mapped].max(), np.abs(pat - exact)[mapped].max()
    rowptr, col, val = out.csr()
    rs = np.bincount(np.repeat(np.arange(out.n_dst), np.diff(rowptr)), weights=val, minlength=out.n_dst)
    print("%s: worst error bilinear %.3g, patch %.3g, ratio %.1f; worst |row sum - 1| %.3g" % (name, eb, ep, eb / ep, np.abs(rs - 1.0)[mapped].max()))
    assert ep <= eb / 5.0
    assert np.abs(rs - 1.0)[mapped].max() <= 1e-13


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(world, gpu_lib):
    from mpassit_amd import _lib as L, regrid as R, synth, target_grid as tg
    lib = L.load()
    o = world["obj"]
    m2m = world["pairs"]["m2m"][0]
    who = "mpg_handle_patch"
    h = C.c_void_p()

    def pts(obj, loc=0):
        return R._points(obj, loc, "x")

    def call(rh=m2m, src=None, dst=None, out=h):
        ps = pts(o["vor2000"]) if src is None else src
        pd = pts(o["hex"]) if dst is None else dst
        return L.handle_patch(rh._h if rh is not None else None, C.byref(ps), C.byref(pd), C.byref(out) if out is not None else None)

    def refused(rc, want, *words):
        msg = lib.mpg_last_error().decode()
        assert rc == want and who in msg, (rc, want, msg)
        for word in words:
            assert word in msg, msg

    INV, UNS = L.MPG_ERR_INVALID_ARG, L.MPG_ERR_UNSUPPORTED
    assert call() == 0
    L.check(lib.mpg_handle_release(h))
    h = C.c_void_p()
    # NULL arguments, point sets that break the rules, sizes
    refused(call(rh=None), INV, "NULL")
    refused(call(out=None), INV, "NULL")
    ps, pd = pts(o["vor2000"]), pts(o["hex"])
    refused(L.handle_patch(m2m._h, None, C.byref(pd), C.byref(h)), INV, "NULL")
    refused(L.handle_patch(m2m._h, C.byref(ps), None, C.byref(h)), INV, "NULL")
    both = L.Points(mesh=o["vor2000"]._h, meshloc=0, grid=o["conus"]._h, staggerloc=0)
    neither = L.Points(mesh=None, meshloc=0, grid=None, staggerloc=0)
    refused(call(src=both), INV, "exactly one", "both")
    refused(call(dst=neither), INV, "exactly one", "neither")
    refused(call(dst=pts(o["vor2000"], R.MESHLOC_EDGE)), INV, "no edges", "mpg_mesh_set_edges")
    refused(call(dst=pts(o["conus"], 7)), INV, "stagger")
    refused(call(src=pts(o["vor2000"], R.MESHLOC_NODE)), INV, "MPG_MESHLOC_ELEMENT")
    refused(call(src=pts(o["global"])), INV, "n_src = 2000", "20000")
    refused(call(dst=pts(o["hex"], R.MESHLOC_EDGE)), INV, "n_dst = %d" % m2m.n_dst, "%d" % o["hex"].nEdges)
    # the method, the kind
    near = R.regrid_store_mesh(o["vor2000"], o["hex"], R.REGRIDMETHOD_NEAREST_STOD)
    refused(call(rh=near), INV, "MPG_REGRIDMETHOD_BILINEAR")
    cons = R.regrid_store(o["global"], o["conus"], R.REGRIDMETHOD_CONSERVE)
    refused(call(rh=cons, src=pts(o["global"]), dst=pts(o["conus"])), INV, "MPG_REGRIDMETHOD_BILINEAR")
    filled = R.extrapolate(m2m, o["vor2000"], o["hex"], R.EXTRAPMETHOD_NEAREST_IDAVG, 8, 2.0)
    assert filled.nnz_per_row == 0
    refused(call(rh=filled), UNS, "CSR", "patch first")
    patched = _patched(world, "m2m")
    refused(call(rh=patched), INV, "MPG_REGRIDMETHOD_BILINEAR")
    # the Stores go on refusing method 3
    with pytest.raises((L.MpgError, ValueError)):
        R.regrid_store_mesh(o["vor2000"], o["hex"], 3)
    with pytest.raises(L.MpgError):
        R.regrid_store(o["global"], o["conus"], 3)
    # pole terms, a periodic source, a localized handle, a source window, a windowed mesh
    gp = tg.define_target_grid_params("lat-lon", nx=25, ny=13, stand_lon=0.0, is_regional=False)
    per = R.Grid.from_target(gp)
    pole = R.regrid_store_grid(per, R.STAGGERLOC_EDGE2)
    assert pole.pole()[0].size > 0
    refused(call(rh=pole, src=pts(per), dst=pts(per, R.STAGGERLOC_EDGE2)), UNS, "mpg_handle_pole_count > 0")
    g97 = world["pairs"]["g2g e1"][0]
    refused(call(rh=g97, src=pts(per), dst=pts(o["g97"], R.STAGGERLOC_EDGE1)), UNS, "MPG_GRID_PERIODIC_I")
    g2 = tg.define_target_grid_params("lambert", 41, 31, dx=30000.0, dy=30000.0, **LAMBERT)      # a mesh larger than its grid: the handle references
    m2 = R.Mesh.from_mpas(synth.regional_mesh_for_lambert(g2.proj, 41, 31, 3001, margin=0.3, seed=3))   # a proper part of the cells
    grid2 = R.Grid.from_target(g2)
    win = R.regrid_store(m2, grid2)
    first, end = win.source_range()
    assert 0 < first < end <= m2.nCells
    assert call(rh=win, src=pts(m2), dst=pts(grid2)) == 0, "the same call without a window"
    L.check(lib.mpg_handle_release(h))
    h = C.c_void_p()
    m2.set_source_window(first, end - first)
    refused(call(rh=win, src=pts(m2), dst=pts(grid2)), UNS, "source window", "mpg_mesh_set_source_window")
    m2.set_source_window(0, m2.nCells)
    win.release()
    m2.destroy()
    grid2.destroy()
    cut = R.Mesh.from_mpas(world["syn"]["global"], window_grid=o["conus"])
    wrh = R.regrid_store(cut, o["conus"])
    refused(call(rh=wrh, src=pts(cut), dst=pts(o["conus"])), UNS, "mpg_mesh_create_window", "whole mesh")
    wrh.release()
    cut.destroy()
    small = R.regrid_store_mesh(o["coarse"], o["coarse"])
    small.localize()
    refused(call(rh=small, src=pts(o["coarse"]), dst=pts(o["coarse"])), UNS, "localized or rebased")
    assert h.value is None, "a refused call leaves *out alone"
    # the wrapper's own check, and the library still works afterwards
    with pytest.raises(ValueError):
        R.patch(m2m, "mesh", o["hex"])
    again = R.patch(m2m, o["vor2000"], o["hex"])
    assert again.nnz_per_row == 0 and again.store_stats[1:7] == patched.store_stats[1:7]
    for x in (again, near, cons, filled, pole, small):
        x.release()
    per.destroy()
