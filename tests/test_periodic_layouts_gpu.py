"""The periodic Grid -> Mesh Store (mpg_regrid_store_periodic_to_mesh) on the grid layouts of tests/_periodic_layouts.py: rows numbered north
to south, Gaussian rows, rows on the poles, a seam away from longitude 0 -- each as a periodic array grid (the walk) and, where its rows
are uniform, with its lat-lon projection attached (the index route).

Besides the comparison with the numpy restatement of the rule (tests/_periodic_to_mesh_ref.py) the handle is checked against the FIELD
being interpolated, and against the handle of the same physical grid with its rows reversed: a cap rule that is wrong in kernel and
reference alike passes the first comparison and fails these two (tests/test_periodic_layouts_ref.py shows it for the rule that took the
pole from the row number).

Inputs: the 20 000-cell global mesh, cells for every layout and vertices for `n2s` and `gauss_n2s`; one device mesh and one CPU reference
per (layout, location) for the module."""
import ctypes as C

import numpy as np
import pytest

import _periodic_layouts as PL
import _periodic_to_mesh_ref as PR
from _parity_helpers import assert_csr_equal
from test_periodic_to_mesh_gpu import _bytes_equal, _csr_identical, _mesh_points, _tie_rows

pytestmark = pytest.mark.gpu

TIE_CAP = 1e-4            # tests/test_to_mesh_gpu.py
CASES = [(name, 0) for name in PL.LAYOUTS] + [(name, 1) for name in PL.WITH_VERTICES]


@pytest.fixture(scope="module")
def case(gpu_lib, oracle, global_mesh):
    """Every layout as a periodic array grid (`arr`) and, where its rows are uniform and the library accepts the claim, a second grid with
    its projection attached (`proj`; the library's message in `refused` otherwise); the device mesh; the reference per (layout, location,
    pole method, flags), computed once and left unchanged."""
    from mpassit_amd import _lib as L, regrid as R
    d = dict(m=global_mesh, mesh=R.Mesh.from_mpas(global_mesh), arr={}, proj={}, refused={}, cen={}, ref={}, pts={})
    for name in PL.LAYOUTS:
        lon, lat = PL.coords(name)
        d["arr"][name] = R.Grid(lon, lat, periodic=L.GRID_PERIODIC_I)
        d["cen"][name] = PL.centers(oracle, name)
        if name in PL.UNIFORM:
            g = R.Grid(lon, lat, periodic=L.GRID_PERIODIC_I)
            try:
                g.attach_proj(PL.proj(name))
                d["proj"][name] = g
            except L.MpgError as e:
                d["refused"][name] = str(e)
                g.destroy()
    print("projection attached: %s; refused: %s" % (sorted(d["proj"]), d["refused"]))
    for loc in (0, 1):
        d["pts"][loc] = _mesh_points(oracle, global_mesh, loc)

    def ref(name, loc, pole_method=PR.POLE_ALLAVG, flags=0):
        key = (name, loc, pole_method, flags)
        if key not in d["ref"]:
            d["ref"][key] = PR.periodic_to_mesh(oracle, d["cen"][name], d["pts"][loc], pole_method=pole_method, flags=flags)
        return d["ref"][key]

    def routes(name):
        return [("walk", d["arr"][name])] + ([("index", d["proj"][name])] if name in d["proj"] else [])

    def ref_errors(name, loc):
        r = ref(name, loc)
        src = PL.fields(d["cen"][name].reshape(-1, 3))
        out = {f: PL.apply_csr(r["rowptr"], r["col"], r["val"], src[f]) for f in PL.FIELDS}
        return PL.field_errors(out, PL.fields(d["pts"][loc]), r["kind"] == PR.KIND_CAP)
    d["get_ref"], d["routes"], d["ref_errors"] = ref, routes, ref_errors
    yield d
    d["mesh"].destroy()
    for k in ("proj", "arr"):
        for grid in d[k].values():
            grid.destroy()


def test_uniform_layouts_take_the_index_route(case):
    """A lat-lon projection describes every layout with uniform rows, those numbered north to south (latinc < 0) included."""
    assert not case["refused"], case["refused"]
    assert sorted(case["proj"]) == sorted(PL.UNIFORM)


# ---- the Store against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,loc", CASES)
def test_store_parity(case, name, loc):
    from mpassit_amd import regrid as R
    r = case["get_ref"](name, loc)
    nx, ny = r["nx"], r["ny"]
    share = PR.edge_share(r)
    ncap, nseam = int((r["kind"] == PR.KIND_CAP).sum()), int(PR.seam_rows(r).size)
    print("reference %s loc %d: %d points, %d in caps, %d in seam quads, share within 1e-9 of an edge %.3g" % (name, loc, r["kind"].size, ncap, nseam, share))
    assert share <= TIE_CAP and (ncap, nseam) == PL.COUNTS[(name, loc)]
    assert not (r["kind"] == PR.KIND_NONE).any()
    n = case["m"].nCells if loc == 0 else case["m"].nVertices
    for route, grid in case["routes"](name):
        rh = R.regrid_store_periodic_to_mesh(grid, case["mesh"], meshloc=loc)
        assert (rh.n_src, rh.n_dst, rh.nx_dst, rh.ny_dst, rh.nnz_per_row) == (nx * ny, n, n, 1, 0)
        assert rh.store_path == (1 if route == "index" else 0), "the %s route did not run" % route
        assert rh.nnz == 4 * (n - ncap) + nx * ncap
        st = rh.store_stats
        print("%s route: store_path %d, stats %s, %.3f ms" % (route, rh.store_path, st[:5], rh.store_ms))
        assert st[2] == n and st[3] == ncap and st[4] == nseam
        rp, col, val = rh.csr()
        assert np.isfinite(val).all(), "NaN or Inf in val"
        assert val.min() >= -1e-9, "a weight below -1e-9"
        ties = _tie_rows(r, rp, col)
        print("tie rows %d of %d" % (ties.size, n))
        assert ties.size <= TIE_CAP * n
        assert np.all(r["edge"][ties] < 1e-9), "a row differs from the reference's away from every edge"
        keep = np.ones(n, bool)
        keep[ties] = False
        if ties.size:   # examined above; the entry comparison below runs on the rows both sides agree on
            sel_r, sel_g = np.repeat(keep, np.diff(r["rowptr"])), np.repeat(keep, np.diff(rp))
            rr = (np.concatenate([[0], np.cumsum(np.where(keep, np.diff(r["rowptr"]), 0))]), r["col"][sel_r], r["val"][sel_r])
            gg = (np.concatenate([[0], np.cumsum(np.where(keep, np.diff(rp), 0))]), col[sel_g], val[sel_g])
        else:
            rr, gg = (r["rowptr"], r["col"], r["val"]), (rp, col, val)
        common, only_r, only_g = assert_csr_equal(rr[0], rr[1], rr[2], gg[0], gg[1], gg[2], rh.n_src, tol=1e-11)
        assert only_r == 0 and only_g == 0 and common == rr[1].size
        inside = np.ones(col.size - 1, bool)               # pairs (q, q + 1) of one row
        inside[rp[1:-1][rp[1:-1] < col.size] - 1] = False
        assert np.all(np.diff(col)[inside] > 0), "columns ascend within a row"
        rows = np.repeat(np.arange(n), np.diff(rp))
        assert np.abs(np.bincount(rows, weights=val, minlength=n) - 1.0).max() < 1e-12, "every row sums to 1 under ALLAVG"
        rh.release()


# ---- the handle against the field --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,loc", CASES)
def test_analytic_fields(case, name, loc):
    """z, x and 1 + z + x y sampled on the grid, applied through the device handle (regrid_csr_to_mesh, float64, one level) and compared
    with the field at the mesh points.  The bounds are those of tests/test_periodic_layouts_ref.py: a south-to-north layout within 1.05 x the
    recorded error of bilinear interpolation on that grid, a north-to-south one within 1.01 x the REFERENCE's error on its twin + 1e-12."""
    import torch
    from mpassit_amd import regrid as R
    if name in PL.TWIN:
        bound = PL.twin_bounds(case["ref_errors"](PL.TWIN[name], loc))
    else:
        want = PL.S2N_ERRORS[name]
        bound = {(f, "all"): 1.05 * want[f] for f in PL.FIELDS}
        bound[("z", "cap")] = None if want["cap z"] is None else 1.05 * want["cap z"]
    ref_err = case["ref_errors"](name, loc)
    src = PL.fields(case["cen"][name].reshape(-1, 3))
    truth = PL.fields(case["pts"][loc])
    for route, grid in case["routes"](name):
        rh = R.regrid_store_periodic_to_mesh(grid, case["mesh"], meshloc=loc)
        cap = np.diff(rh.csr()[0]) == rh.n_src // PL.LAYOUTS[name][1].size
        out = {f: rh.regrid_csr_to_mesh(torch.as_tensor(np.ascontiguousarray(src[f]), device="cuda")).reshape(-1).cpu().numpy() for f in PL.FIELDS}
        err = PL.field_errors(out, truth, cap)
        print("%s loc %d %s: %s" % (name, loc, route, ", ".join(
            "%s %s %.4g (reference %.4g)" % (f, w, e, ref_err[(f, w)]) for (f, w), e in err.items() if e is not None)))
        for k, b in bound.items():
            if b is None:
                assert err[k] is None, "cap rows where the reference has none"
            else:
                assert err[k] is not None and err[k] <= b, (route, k, err[k], b)
        rh.release()


# ---- the same physical grid with its rows reversed ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,loc", [c for c in CASES if c[0] in PL.TWIN])
def test_row_flip_identity(case, name, loc):
    """With every column mapped by j -> ny - 1 - j the device handle of a north-to-south layout has the row lengths and column sets of its
    twin's device handle, and its values within 1e-11."""
    from mpassit_amd import regrid as R
    twin = dict(case["routes"](PL.TWIN[name]))
    nx, ny = PL.LAYOUTS[name][0].size, PL.LAYOUTS[name][1].size
    for route, grid in case["routes"](name):
        if route not in twin:
            continue
        ra = R.regrid_store_periodic_to_mesh(grid, case["mesh"], meshloc=loc)
        rb = R.regrid_store_periodic_to_mesh(twin[route], case["mesh"], meshloc=loc)
        rp, col, val = PL.flip_rows(*ra.csr(), nx, ny)
        rpt, colt, valt = rb.csr()
        assert np.array_equal(rp, rpt), "row kinds and lengths differ"
        assert np.array_equal(col, colt), "the column sets differ"
        common, only_a, only_b = assert_csr_equal(rpt, colt, valt, rp, col, val, nx * ny, tol=1e-11)
        assert only_a == 0 and only_b == 0 and common == col.size
        d = np.abs(val - valt)
        cap = np.repeat(np.diff(rp) == nx, np.diff(rp))
        print("%s loc %d %s: largest row-flip difference %.3g on quad rows, %.3g on cap rows" % (
            name, loc, route, d[~cap].max(), d[cap].max() if cap.any() else 0.0))
        ra.release()
        rb.release()


# ---- route identity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,loc", [c for c in CASES if c[0] in PL.UNIFORM])
def test_route_identity(case, name, loc):
    """Where both the index route and the walk ran: rowptr, col and the bytes of val are identical."""
    from mpassit_amd import regrid as R
    routes = dict(case["routes"](name))
    if "index" not in routes:
        assert name in case["refused"]       # (test_uniform_layouts_take_the_index_route fails on it)
        return
    ra = R.regrid_store_periodic_to_mesh(routes["index"], case["mesh"], meshloc=loc)
    rb = R.regrid_store_periodic_to_mesh(routes["walk"], case["mesh"], meshloc=loc)
    assert ra.store_path == 1 and rb.store_path == 0
    print("%s loc %d: index route sent %d of %d points to the walk" % (name, loc, ra.store_stats[1], ra.store_stats[2]))
    assert _csr_identical(ra.csr(), rb.csr())
    ra.release()
    rb.release()


# ---- pole method and row blocks on a grid numbered north to south ----------------------------------------------------------------------------
def test_pole_method_and_row_blocks_n2s(case):
    """The flags name an END of the row range, not a pole: on `n2s` GRID_NO_SOUTH_POLE (the row-0 end) drops the NORTHERN cap."""
    from mpassit_amd import _lib as L, regrid as R
    name, loc = "n2s", 0
    r = case["get_ref"](name, loc)
    nx = r["nx"]
    cap = r["kind"] == PR.KIND_CAP
    first = cap & (r["cap"] < nx)              # the cap of the row-0 end
    assert int(cap.sum()) == 169 and first.any() and (cap & ~first).any()
    assert np.all(case["pts"][loc][first, 2] > 0.9) and np.all(case["pts"][loc][cap & ~first, 2] < -0.9), "row 0 closes on the NORTH pole"
    grid, mesh = case["arr"][name], case["mesh"]
    avg = R.regrid_store_periodic_to_mesh(grid, mesh, meshloc=loc)
    rp, col, val = avg.csr()

    def rows_equal(rp2, col2, val2, rows):
        for p in rows:
            s, s2 = slice(rp[p], rp[p + 1]), slice(rp2[p], rp2[p + 1])
            if not (np.array_equal(col[s], col2[s2]) and np.array_equal(val[s].view(np.int64), val2[s2].view(np.int64))):
                return False
        return True

    none = R.regrid_store_periodic_to_mesh(grid, mesh, meshloc=loc, pole_method=R.POLEMETHOD_NONE)
    rp0, col0, val0 = none.csr()
    assert np.array_equal(np.diff(rp0) == 0, cap), "under NONE exactly the reference's cap points are empty"
    assert none.store_stats[3] == 0 and none.nnz == 4 * int((~cap).sum())
    assert rows_equal(rp0, col0, val0, np.nonzero(~cap)[0]), "a quad row's bytes changed"
    lon, lat = PL.coords(name)
    for flag, gone in ((L.GRID_NO_SOUTH_POLE, first), (L.GRID_NO_NORTH_POLE, cap & ~first)):
        g = R.Grid(lon, lat, periodic=L.GRID_PERIODIC_I | flag)
        blk = R.regrid_store_periodic_to_mesh(g, mesh, meshloc=loc)
        rp1, col1, val1 = blk.csr()
        assert np.array_equal(np.diff(rp1) == 0, gone), "the flag dropped other points than that end's cap"
        assert blk.store_stats[3] == int((cap & ~gone).sum())
        assert rows_equal(rp1, col1, val1, np.nonzero(~gone)[0]), "the other end or a quad row changed its bytes"
        ref = case["get_ref"](name, loc, flags=flag)
        assert np.array_equal(np.diff(ref["rowptr"]) == 0, gone)
        blk.release()
        g.destroy()
    for rh in (avg, none):
        rh.release()


# ---- the existing CSR applies on cap rows of 48 entries ---------------------------------------------------------------------------------------
def test_apply_on_gauss_n2s(case):
    """float32, 3 levels: cap rows of 48 entries between rows of 4.  regrid_csr_to_mesh [lev][cell] has regrid_typed's bytes, [cell][lev] its
    transposition, regrid_csr_rows the LEV_FAST typed result transposed (tests/test_periodic_to_mesh_gpu.py, on rows of 24)."""
    import torch
    from mpassit_amd import regrid as R
    nlev, dt = 3, torch.float32
    rh = R.regrid_store_periodic_to_mesh(case["arr"]["gauss_n2s"], case["mesh"])
    rp, col, val = rh.csr()
    assert set(np.unique(np.diff(rp))) == {4, 48}
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1003)
    src = ((torch.rand((nlev, rh.n_src), dtype=torch.float64, device="cuda", generator=gen) - 0.5) * 80.0).to(dt)
    want = rh.regrid_typed(src.reshape(-1), nlev=nlev).reshape(nlev, rh.n_dst)
    cf = torch.full((1, nlev, rh.n_dst), float("nan"), dtype=dt, device="cuda")
    lf = torch.full((1, rh.n_dst, nlev), float("nan"), dtype=dt, device="cuda")
    rows = torch.full((1, rh.n_dst, nlev), float("nan"), dtype=dt, device="cuda")
    rh.regrid_csr_to_mesh(src, nlev=nlev, layout=R.LAYOUT_CELL_FAST, out=cf)
    rh.regrid_csr_to_mesh(src, nlev=nlev, layout=R.LAYOUT_LEV_FAST, out=lf)
    src_rows = src.t().contiguous()                      # [n_src][nlev]
    rh.regrid_csr_rows(src_rows, nlev=nlev, out=rows)
    for t in (cf, lf, rows):
        assert not torch.isnan(t).any(), "an element was left unwritten"
    assert _bytes_equal(cf[0], want), "[lev][cell] differs from regrid_typed"
    assert _bytes_equal(lf[0], want.t().contiguous()), "[cell][lev] is not the transposition of regrid_typed"
    typed_lf = rh.regrid_typed(src_rows.reshape(-1), nlev=nlev, layout=R.LAYOUT_LEV_FAST).reshape(nlev, rh.n_dst)
    assert _bytes_equal(rows[0], typed_lf.t().contiguous()), "regrid_csr_rows [p][k] is not regrid_typed(LEV_FAST) [k][p]"
    # ... and the values: a float64 sum of the handle's own CSR, within float32 rounding of the result and of each product's source
    ref = np.stack([PL.apply_csr(rp, col, val, src[k].double().cpu().numpy()) for k in range(nlev)])
    r = np.repeat(np.arange(rh.n_dst), np.diff(rp))
    sabs = np.stack([np.bincount(r, weights=np.abs(val * src[k].double().cpu().numpy()[col]), minlength=rh.n_dst) for k in range(nlev)])
    d = np.abs(cf[0].double().cpu().numpy() - ref)
    bound = 2.0 ** -24 * np.abs(ref) + (np.diff(rp) + 2)[None, :] * 2.0 ** -53 * sabs      # one float32 rounding of a float64 fma sum
    print("float32 apply vs a float64 sum of the handle's CSR: largest difference %.3e, %.3f of the bound at worst" % (d.max(), (d / bound).max()))
    assert np.all(d <= bound)
    rh.release()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_grid_to_grid_refuses_rows_numbered_north_to_south(case, gpu_lib):
    """The Grid -> Grid bilinear Store places its caps by row number; a periodic grid numbered north to south is refused, its twin served."""
    from mpassit_amd import _lib as L, regrid as R
    lib = L.load()
    for name, ok in (("s2n", True), ("n2s", False)):
        lon, lat = PL.LAYOUTS[name]
        dlat = lat[1] - lat[0]
        lat_v = np.concatenate([[lat[0] - 0.5 * dlat], 0.5 * (lat[1:] + lat[:-1]), [lat[-1] + 0.5 * dlat]])
        lon2, lat2 = PL.coords(name)
        g = R.Grid(lon2, lat2, lon_v=np.broadcast_to(lon[None, :], (lat_v.size, lon.size)), lat_v=np.broadcast_to(lat_v[:, None], (lat_v.size, lon.size)),
                   periodic=L.GRID_PERIODIC_I)
        h = C.c_void_p()
        rc = lib.mpg_regrid_store_grid(g._h, C.c_int(R.STAGGERLOC_CENTER), C.c_int(R.STAGGERLOC_EDGE2), C.c_int(R.REGRIDMETHOD_BILINEAR), C.byref(h))
        if ok:
            assert rc == L.MPG_SUCCESS, lib.mpg_last_error().decode()
            rh = R.RouteHandle(h)
            assert rh.n_dst == lat_v.size * lon.size and rh.pole()[2].max() > 0.9, "the twin's end rows lie in its caps"
            rh.release()
        else:
            msg = lib.mpg_last_error().decode()
            assert rc == L.MPG_ERR_UNSUPPORTED and "north to south" in msg and "reverse the rows" in msg, (rc, msg)
        g.destroy()
