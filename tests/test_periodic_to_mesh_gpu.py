"""Bilinear Grid -> Mesh from periodic global grids on the GPU: the Store (mpg_regrid_store_periodic_to_mesh) against the numpy
restatement of its rule (tests/_periodic_to_mesh_ref.py), its identity with the non-periodic Store away from the seam, the identity of
its candidate routes, the pole methods and row-block flags, and the existing CSR calls on its handle.

Inputs: the 20 000-cell global mesh (cells and vertices) and two global lat-lon grids, 72 x 36 (rows at +-87.5 degrees) and 24 x 12 (rows
at +-82.5: 169 cells and 336 vertices in the caps), each from its projection (Grid.from_target: the index route) and as arrays with
periodic=True (the pyramid walk)."""
import ctypes as C

import numpy as np
import pytest

import _periodic_to_mesh_ref as PR
from _parity_helpers import assert_csr_equal
from _transpose_ref import assert_f64_close, transpose_ref

pytestmark = pytest.mark.gpu

TIE_CAP = 1e-4            # at most 1 row in 10 000 may be a point within 1e-9 of an edge (tests/test_to_mesh_gpu.py)
GRIDS = {"72x36": (73, 37), "24x12": (25, 13)}
# the reference's counts on these inputs: (cap points, seam-quad points) per grid and mesh location
COUNTS = {("72x36", 0): (19, 280), ("24x12", 0): (169, 829), ("72x36", 1): (39, 550), ("24x12", 1): (336, 1650)}


def _mesh_points(o, m, loc):
    lon, lat = (m.lonCell, m.latCell) if loc == 0 else (m.lonVertex, m.latVertex)
    return o.lonlat_deg_to_xyz(*o.mesh_coords_deg(lon, lat))


def _bytes_equal(a, b):
    import torch
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    bits = torch.int64 if a.dtype == torch.float64 else torch.int32       # compared as integers: -0.0 is not +0.0, NaN equals itself
    return torch.equal(a.reshape(-1).view(bits), b.reshape(-1).view(bits))


def _csr_identical(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x, y)) and np.array_equal(x[2].view(np.int64), y[2].view(np.int64))


@pytest.fixture(scope="module")
def case(gpu_lib, oracle, global_mesh):
    """Both grids from their projection (`proj`) and as periodic arrays (`arr`), the mesh, and the reference per (grid, location),
    computed once and left unchanged."""
    from mpassit_amd import _lib as L, regrid as R, target_grid as tg
    d = dict(m=global_mesh, mesh=R.Mesh.from_mpas(global_mesh), tg={}, proj={}, arr={}, cen={}, ref={})
    for name, (nxn, nyn) in GRIDS.items():
        g = tg.define_target_grid_params("lat-lon", nx=nxn, ny=nyn, stand_lon=0.0, is_regional=False)
        d["tg"][name] = g
        d["proj"][name] = R.Grid.from_target(g)
        d["arr"][name] = R.Grid(g.lon, g.lat, periodic=L.GRID_PERIODIC_I)
        d["cen"][name] = oracle.lonlat_deg_to_xyz(g.lon, g.lat).reshape(g.lat.shape + (3,))

    def ref(name, loc, pole_method=PR.POLE_ALLAVG, flags=0):
        key = (name, loc, pole_method, flags)
        if key not in d["ref"]:
            d["ref"][key] = PR.periodic_to_mesh(oracle, d["cen"][name], _mesh_points(oracle, global_mesh, loc), pole_method=pole_method, flags=flags)
        return d["ref"][key]
    d["get_ref"] = ref
    yield d
    d["mesh"].destroy()
    for k in ("proj", "arr"):
        for grid in d[k].values():
            grid.destroy()


def _tie_rows(r, rp, col):
    """Rows whose column sets differ between the reference and the library: only a point within 1e-9 of an edge may be one."""
    rl, gl = np.diff(r["rowptr"]), np.diff(rp)
    diff = rl != gl
    same = np.nonzero(~diff)[0]
    for length in np.unique(rl[same]):
        if length == 0:
            continue
        rows = same[rl[same] == length]
        a = r["col"][r["rowptr"][rows][:, None] + np.arange(length)[None, :]]
        b = col[rp[rows][:, None] + np.arange(length)[None, :]]
        diff[rows[(a != b).any(axis=1)]] = True
    return np.nonzero(diff)[0]


# ---- 4a: the Store against the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRIDS))
@pytest.mark.parametrize("loc", [0, 1])
def test_store_parity(case, name, loc):
    from mpassit_amd import regrid as R
    r = case["get_ref"](name, loc)
    share = PR.edge_share(r)
    ncap, nseam = int((r["kind"] == PR.KIND_CAP).sum()), int(PR.seam_rows(r).size)
    print("reference %s loc %d: %d points, %d in caps, %d in seam quads, share within 1e-9 of an edge %.3g" % (name, loc, r["kind"].size, ncap, nseam, share))
    assert share <= TIE_CAP and (ncap, nseam) == COUNTS[(name, loc)]
    g = case["tg"][name]
    n = case["m"].nCells if loc == 0 else case["m"].nVertices
    for route, grid in (("index", case["proj"][name]), ("walk", case["arr"][name])):
        rh = R.regrid_store_periodic_to_mesh(grid, case["mesh"], meshloc=loc)
        assert (rh.n_src, rh.n_dst, rh.nx_dst, rh.ny_dst, rh.nnz_per_row) == (g.lon.size, n, n, 1, 0)
        assert rh.nnz == 4 * (n - ncap) + g.lon.shape[1] * ncap
        assert all(a.size == 0 for a in rh.pole()[:3]), "the handle carries no pole terms"
        assert rh.store_ms > 0.0
        st = rh.store_stats
        print("%s route: store_path %d, stats %s, %.3f ms" % (route, rh.store_path, st[:5], rh.store_ms))
        assert st[2] == n and st[3] == ncap and st[4] == nseam
        rp, col, val = rh.csr()
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


# ---- 4b: identity with the non-periodic Store, no tolerance -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRIDS))
@pytest.mark.parametrize("loc", [0, 1])
def test_identity_with_the_non_periodic_store(case, name, loc):
    """The same coordinates as a non-periodic array grid: every point mpg_regrid_store_to_mesh maps has the same four columns here and,
    after the column sort, the same weight BITS."""
    from mpassit_amd import regrid as R
    g = case["tg"][name]
    plain = R.Grid(g.lon, g.lat)
    fx = R.regrid_store_to_mesh(plain, case["mesh"], meshloc=loc)
    rh = R.regrid_store_periodic_to_mesh(case["arr"][name], case["mesh"], meshloc=loc)
    idx, w = fx.weights()
    rp, col, val = rh.csr()
    mapped = np.nonzero(idx[:, 0] >= 0)[0]
    r = case["get_ref"](name, loc)
    assert mapped.size == int(((r["kind"] == PR.KIND_QUAD) & (r["quad"] % r["nx"] != r["nx"] - 1)).sum()), "the old call maps all but seam and caps"
    order = np.argsort(idx[mapped], axis=1, kind="stable")
    ci, wi = np.take_along_axis(idx[mapped], order, axis=1), np.take_along_axis(w[mapped], order, axis=1)
    four = np.diff(rp)[mapped] == 4
    at = rp[mapped][:, None] + np.arange(4)[None, :]
    at = np.where(four[:, None], at, 0)
    same_cols = four & (col[at] == ci).all(axis=1)
    ties = mapped[~same_cols]
    print("%s loc %d: %d points mapped by the non-periodic Store, %d tie rows" % (name, loc, mapped.size, ties.size))
    assert ties.size <= TIE_CAP * idx.shape[0] and np.all(r["edge"][ties] < 1e-9)
    assert np.array_equal(val[at][same_cols].view(np.int64), wi[same_cols].view(np.int64)), "weights differ in their bits"
    fx.release()
    rh.release()
    plain.destroy()


# ---- 4c: route identity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRIDS))
def test_route_identity(case, gpu_lib, name):
    """Index route (projection grid), walk (array twin) and store_boxes 0 on fresh objects: rowptr / col / val identical byte for byte."""
    from mpassit_amd import regrid as R
    for loc in (0, 1):
        ra = R.regrid_store_periodic_to_mesh(case["proj"][name], case["mesh"], meshloc=loc)
        rb = R.regrid_store_periodic_to_mesh(case["arr"][name], case["mesh"], meshloc=loc)
        assert ra.store_path == 1 and rb.store_path == 0
        grid2, mesh2 = R.Grid.from_target(case["tg"][name]), R.Mesh.from_mpas(case["m"])
        gpu_lib.tune("store_boxes", 0)
        try:
            rc = R.regrid_store_periodic_to_mesh(grid2, mesh2, meshloc=loc)
        finally:
            gpu_lib.tune("store_boxes", 1)
        assert rc.store_path == 0
        # a second Store on fresh objects by the index route: the same bytes from run to run
        grid3, mesh3 = R.Grid.from_target(case["tg"][name]), R.Mesh.from_mpas(case["m"])
        rd = R.regrid_store_periodic_to_mesh(grid3, mesh3, meshloc=loc)
        assert rd.store_path == 1 and rd._h.value != ra._h.value
        a = ra.csr()
        for other, what in ((rb, "walk on the array twin"), (rc, "store_boxes 0"), (rd, "a second index Store")):
            assert _csr_identical(a, other.csr()), what
        print("%s loc %d: index route sent %d of %d points to the walk" % (name, loc, ra.store_stats[1], ra.store_stats[2]))
        for rh in (ra, rb, rc, rd):
            rh.release()
        for obj in (mesh2, grid2, mesh3, grid3):
            obj.destroy()


# ---- 4d: pole method, row-block flags, cache --------------------------------------------------------------------------------------------
def test_pole_method_flags_and_cache(case):
    from mpassit_amd import _lib as L, regrid as R
    name, loc = "24x12", 0
    r = case["get_ref"](name, loc)
    cap = r["kind"] == PR.KIND_CAP
    north = cap & (r["cap"] >= r["nx"])
    assert north.any() and (cap & ~north).any()
    grid, mesh = case["arr"][name], case["mesh"]
    avg = R.regrid_store_periodic_to_mesh(grid, mesh, meshloc=loc)
    none = R.regrid_store_periodic_to_mesh(grid, mesh, meshloc=loc, pole_method=R.POLEMETHOD_NONE)
    assert none._h.value != avg._h.value, "the two pole methods are two cached handles"
    again = R.regrid_store_periodic_to_mesh(grid, mesh, meshloc=loc, pole_method=R.POLEMETHOD_ALLAVG)
    assert again._h.value == avg._h.value, "a second Store of the same key returns the cached handle"
    again.release()
    rp, col, val = avg.csr()

    def rows_equal(rp2, col2, val2, rows):
        for p in rows:
            s, s2 = slice(rp[p], rp[p + 1]), slice(rp2[p], rp2[p + 1])
            if not (np.array_equal(col[s], col2[s2]) and np.array_equal(val[s].view(np.int64), val2[s2].view(np.int64))):
                return False
        return True

    rp0, col0, val0 = none.csr()
    assert np.array_equal(np.diff(rp0) == 0, cap), "under NONE exactly the cap points are empty"
    assert none.store_stats[3] == 0 and none.nnz == 4 * int((~cap).sum())
    assert rows_equal(rp0, col0, val0, np.nonzero(~cap)[0])
    # a row block that does not reach the north pole: its north cap is empty, its south cap and its quads unchanged
    g = case["tg"][name]
    nn = R.Grid(g.lon, g.lat, periodic=L.GRID_PERIODIC_I | L.GRID_NO_NORTH_POLE)
    blk = R.regrid_store_periodic_to_mesh(nn, mesh, meshloc=loc)
    rp1, col1, val1 = blk.csr()
    assert np.array_equal(np.diff(rp1) == 0, north) and blk.store_stats[3] == int((cap & ~north).sum())
    assert rows_equal(rp1, col1, val1, np.nonzero(~north)[0])
    for rh in (avg, none, blk):
        rh.release()
    nn.destroy()


def test_quads_are_tried_before_caps_on_the_shared_edge(case, oracle):
    """A cap triangle and the quads of its end row share the great circle through A and B: a point ON it passes both, and the rule gives
    it the quad (tests/test_periodic_to_mesh_ref.py shows that a cap tried first would give it a cap row)."""
    from mpassit_amd import regrid as R, synth
    name = "24x12"
    cen = case["cen"][name]
    ny, nx, _ = cen.shape
    a = np.array([0, 1, nx // 2, nx - 1])
    mid = np.concatenate([cen[ny - 1, a] + cen[ny - 1, (a + 1) % nx], cen[0, a] + cen[0, (a + 1) % nx]])
    mid /= np.linalg.norm(mid, axis=1, keepdims=True)
    m = synth.global_voronoi_mesh(100)
    lat, lon = m.latCell.copy(), m.lonCell.copy()
    lat[:8], lon[:8] = np.arcsin(mid[:, 2]), np.arctan2(mid[:, 1], mid[:, 0])          # eight cell centres moved onto the edges
    mesh = R.Mesh(lat, lon, m.latVertex, m.lonVertex, m.verticesOnCell)
    r = PR.periodic_to_mesh(oracle, cen, oracle.lonlat_deg_to_xyz(*oracle.mesh_coords_deg(lon, lat)))
    assert np.all(r["kind"][:8] == PR.KIND_QUAD) and np.array_equal(r["quad"][:8], np.concatenate([(ny - 2) * nx + a, a]))
    for grid in (case["proj"][name], case["arr"][name]):
        rh = R.regrid_store_periodic_to_mesh(grid, mesh)
        rp, col, val = rh.csr()
        assert np.array_equal(np.diff(rp)[:8], np.full(8, 4)), "a point on the shared edge has a quad row"
        assert np.array_equal(col[:32], r["col"][:32]) and np.abs(val[:32] - r["val"][:32]).max() < 1e-9
        rh.release()
    mesh.destroy()


# ---- 4e: the existing CSR applies on the new handle ---------------------------------------------------------------------------------------
def test_constant_source(case):
    import torch
    from mpassit_amd import regrid as R
    for name in GRIDS:
        rh = R.regrid_store_periodic_to_mesh(case["proj"][name], case["mesh"])
        out = rh.regrid_csr_to_mesh(torch.ones(rh.n_src, dtype=torch.float64, device="cuda"))
        assert float((out - 1.0).abs().max()) < 1e-12
        rh.release()


@pytest.mark.parametrize("dt", ["float64", "float32"])
@pytest.mark.parametrize("nlev", [1, 3, 55])
def test_apply_identities_and_values(case, oracle, dt, nlev):
    """Rows of 24 entries beside rows of 4: regrid_csr_to_mesh [lev][cell] has regrid_typed's bytes, [cell][lev] its transposition,
    regrid_csr_rows the LEV_FAST typed result transposed; float64 results lie within the bound of a sequential fma sum of the library's
    own CSR."""
    import torch
    from mpassit_amd import regrid as R
    dt = getattr(torch, dt)
    rh = R.regrid_store_periodic_to_mesh(case["arr"]["24x12"], case["mesh"])
    rp, col, val = rh.csr()
    assert set(np.unique(np.diff(rp))) == {4, 24}
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1000 + nlev)
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
    if dt == torch.float64:
        s = src.cpu().numpy()
        ref = oracle.apply_csr(rp, col, val, s, nlev)
        r = np.repeat(np.arange(rh.n_dst), np.diff(rp))
        sabs = np.stack([np.bincount(r, weights=np.abs(val * s[k, col]), minlength=rh.n_dst) for k in range(nlev)])
        bound = (np.diff(rp) + 2)[None, :] * 2.0 ** -53 * sabs       # (row_len + 2) u sum |val src|: a sequential fma sum of row_len terms
        d = np.abs(cf[0].cpu().numpy() - ref)
        print("apply vs oracle.apply_csr: largest difference %.3e, %.3f of the bound at worst" % (d.max(), (d / bound).max()))
        assert np.all(d <= bound)
    rh.release()


# ---- 4f: downstream contracts ---------------------------------------------------------------------------------------------------------------
def test_masked_transpose_autograd(case):
    import torch
    from mpassit_amd import regrid as R
    name = "24x12"
    r = case["get_ref"](name, 0)
    nx, ny = r["nx"], r["ny"]
    rh = R.regrid_store_periodic_to_mesh(case["proj"][name], case["mesh"])
    rp, col, val = rh.csr()
    nlev = 2
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    src = torch.rand((nlev, rh.n_src), dtype=torch.float64, device="cuda", generator=gen) + 1.0
    plain = rh.regrid_typed(src.reshape(-1), nlev=nlev).reshape(nlev, -1)
    bad = (ny - 1) * nx + 5                                # one source of the north row
    src2 = src.clone()
    src2[:, bad] = float("nan")
    masked = rh.regrid_masked(src2.reshape(-1), nlev=nlev, min_valid_frac=0.0, fill_value=-1.0).reshape(nlev, -1)
    touched = np.zeros(rh.n_dst, bool)
    touched[np.repeat(np.arange(rh.n_dst), np.diff(rp))[col == bad]] = True
    north = (r["kind"] == PR.KIND_CAP) & (r["cap"] >= nx)
    assert north.any() and touched[north].all(), "every north cap row holds the masked source"
    assert not torch.isnan(masked).any() and bool((masked[:, torch.as_tensor(north, device="cuda")] > 0.99).all()), "cap points stay finite"
    keep = torch.as_tensor(~touched, device="cuda")
    assert _bytes_equal(masked[:, keep].contiguous(), plain[:, keep].contiguous()), "untouched points keep the unmasked bits"
    # <y, A x> = <A^T y, x>, and A^T against the numpy transpose of the handle's own weight list
    rng = np.random.default_rng(3)
    x = torch.as_tensor(rng.normal(size=(nlev, rh.n_src)), device="cuda")
    y = torch.as_tensor(rng.normal(size=(nlev, rh.n_dst)), device="cuda")
    ax = rh.regrid_csr_to_mesh(x, nlev=nlev).reshape(nlev, -1)
    aty = rh.regrid_transpose(y, nlev=nlev).reshape(nlev, -1)
    want, bound = transpose_ref(rh, y.cpu().numpy())
    assert_f64_close(aty.cpu().numpy(), want, bound, "regrid_transpose on the periodic handle")
    lhs, rhs = float((ax * y).sum()), float((x * aty).sum())
    assert abs(lhs - rhs) <= 1e-13 * float(ax.norm() * y.norm())     # the expression and bar of tests/test_transpose_gpu.py
    # the autograd wrapper: forward bytes, backward = that transpose
    for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
        xs = x.clone().requires_grad_(True)
        out = R.regrid_csr_to_mesh_autograd(rh, xs, nlev=nlev, layout=layout)
        assert _bytes_equal(out.detach(), rh.regrid_csr_to_mesh(xs.detach(), nlev=nlev, layout=layout))
        up = torch.as_tensor(rng.normal(size=tuple(out.shape)), device="cuda")
        out.backward(up)
        up_cf = up if layout == R.LAYOUT_CELL_FAST else up.transpose(1, 2).contiguous()
        assert torch.equal(xs.grad, rh.regrid_transpose(up_cf.reshape(1, nlev, rh.n_dst), nlev=nlev).reshape(xs.shape))
    rh.release()
    # gradcheck on a small slice: the 196 vertices of a 100-cell global mesh, 2 of them in the caps and 9 in seam quads
    from mpassit_amd import synth
    tmesh = R.Mesh.from_mpas(synth.global_voronoi_mesh(100))
    small = R.regrid_store_periodic_to_mesh(case["arr"][name], tmesh, meshloc=R.MESHLOC_NODE)
    lens = np.diff(small.csr()[0])
    assert small.n_dst == 196 and int((lens == nx).sum()) == 2 and int((lens == 4).sum()) == 194 and small.store_stats[4] == 9
    for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
        xs = torch.as_tensor(rng.normal(size=(1, 2, small.n_src)), device="cuda").requires_grad_(True)
        assert torch.autograd.gradcheck(lambda t: R.regrid_csr_to_mesh_autograd(small, t, nlev=2, layout=layout), (xs,), eps=1e-6, atol=1e-7)
    small.release()
    tmesh.destroy()


# ---- 4g: refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(case, gpu_lib, conus_grid_30km):
    import torch
    from mpassit_amd import _lib as L, regrid as R
    lib = L.load()

    def refused(rc, want, *words):
        msg = lib.mpg_last_error().decode()
        assert rc == want and msg, (rc, want, msg)
        for word in words:
            assert word in msg, msg

    h = C.c_void_p()
    grid, mesh = case["arr"]["72x36"], case["mesh"]
    store = L.regrid_store_periodic_to_mesh
    refused(store(None, mesh._h, 0, 1, C.byref(h)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(store(grid._h, None, 0, 1, C.byref(h)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(store(grid._h, mesh._h, 0, 1, None), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(store(grid._h, mesh._h, 2, 1, C.byref(h)), L.MPG_ERR_INVALID_ARG, "mesh location", "MPG_MESHLOC_NODE")
    refused(store(grid._h, mesh._h, 0, 2, C.byref(h)), L.MPG_ERR_INVALID_ARG, "pole_method", "MPG_POLEMETHOD_ALLAVG")
    refused(store(grid._h, mesh._h, 0, -1, C.byref(h)), L.MPG_ERR_INVALID_ARG, "pole_method")
    g = case["tg"]["72x36"]
    for shape in ((slice(0, 2), slice(0, 2)), (slice(0, 1), slice(0, 8))):      # nx = 2; ny = 1
        tiny = R.Grid(g.lon[shape], g.lat[shape], periodic=L.GRID_PERIODIC_I)
        refused(store(tiny._h, mesh._h, 0, 1, C.byref(h)), L.MPG_ERR_INVALID_ARG, "nx >= 3 and ny >= 2")
        tiny.destroy()
    plain = R.Grid(g.lon, g.lat)
    refused(store(plain._h, mesh._h, 0, 1, C.byref(h)), L.MPG_ERR_UNSUPPORTED, "MPG_GRID_PERIODIC_I", "mpg_regrid_store_to_mesh")
    plain.destroy()
    # both end rows in one hemisphere: at most one of them closes on a pole, and the flags say which end does not
    north_rows = g.lat[:, 0] > 0.0
    half = R.Grid(g.lon[north_rows], g.lat[north_rows], periodic=L.GRID_PERIODIC_I)
    refused(store(half._h, mesh._h, 0, 1, C.byref(h)), L.MPG_ERR_INVALID_ARG, "northern hemisphere", "MPG_GRID_NO_SOUTH_POLE", "MPG_GRID_NO_NORTH_POLE")
    assert store(half._h, mesh._h, 0, R.POLEMETHOD_NONE, C.byref(h)) == L.MPG_SUCCESS, "without caps no pole is asked for"
    R.RouteHandle(h).release()
    half.destroy()
    block = R.Grid(g.lon[north_rows], g.lat[north_rows], periodic=L.GRID_PERIODIC_I | L.GRID_NO_SOUTH_POLE)
    assert store(block._h, mesh._h, 0, 1, C.byref(h)) == L.MPG_SUCCESS, lib.mpg_last_error().decode()
    R.RouteHandle(h).release()
    block.destroy()
    wgrid = R.Grid.from_target(conus_grid_30km, rows=(10, 60))
    wmesh = R.Mesh.from_mpas(case["m"], window_grid=wgrid)
    refused(store(grid._h, wmesh._h, 0, 1, C.byref(h)), L.MPG_ERR_UNSUPPORTED, "mpg_mesh_create_window", "mpg_mesh_create")
    wmesh.destroy()
    wgrid.destroy()
    # the old call keeps refusing and names the new one
    refused(L.regrid_store_to_mesh(grid._h, 0, mesh._h, 0, R.REGRIDMETHOD_BILINEAR, C.byref(h)), L.MPG_ERR_UNSUPPORTED, "periodic",
            "mpg_regrid_store_periodic_to_mesh")
    # the fixed-handle applies refuse the new handle as CSR and name the CSR calls
    rh = R.regrid_store_periodic_to_mesh(grid, mesh)
    src = torch.zeros(rh.n_src, dtype=torch.float64, device="cuda")
    with pytest.raises(L.MpgError) as e:
        rh.regrid_to_mesh(src)
    assert e.value.rc == L.MPG_ERR_UNSUPPORTED and "mpg_regrid_csr_to_mesh_dev" in str(e.value)
    with pytest.raises(L.MpgError) as e:
        rh.regrid_rows(src)
    assert e.value.rc == L.MPG_ERR_UNSUPPORTED and "mpg_regrid_csr_rows_dev" in str(e.value)
    row, col, S = rh.to_esmf_weights()
    assert row.size == rh.nnz and row.min() == 1 and row.max() == rh.n_dst and col.min() >= 1 and col.max() <= rh.n_src
    rh.release()
