"""Conservative Grid -> Mesh on the GPU at small sizes: the Store (mpg_regrid_store_conserve_to_mesh) against B_ref built from the
oracle's Mesh -> Grid matrix (tests/_conserve_to_mesh_ref.py) and from the 50-digit goldens, its properties (dst fraction,
normalisations, conservation, determinism, route identity, cache), and the CSR mesh-order apply (mpg_regrid_csr_to_mesh_dev) held to
the typed Regrid BYTE FOR BYTE -- [lev][cell] equal, [cell][lev] its transposition -- on this Store's handles, a Mesh -> Grid
conservative one and a from-weights one, plus the contract around them: empty rows, masked fill, adjoint, autograd, graph capture
from the first call, refusals.

Grid (a) is the 61 x 41 Lambert grid of tests/test_to_mesh_gpu.py built from its projection (index boxes), grid (b) its array twin
(pyramid walk).  Meshes: one that overhangs the grid (rim cells with 0 < frac < 1 and uncovered cells), one inside it, and a COARSE one
of ~200 cells whose rows are tens of entries long, so that 64 rows outgrow the apply kernel's LDS chunk."""
import ctypes as C

import numpy as np
import pytest

import _conserve_to_mesh_ref as CR
from _parity_helpers import assert_csr_equal
from conftest import LAMBERT, mesh_xyz
from test_to_mesh_gpu import _arrays_grid, _bytes_equal

pytestmark = pytest.mark.gpu

NORMS = [CR.NORM_DSTAREA, CR.NORM_FRACAREA]
APPLY_BAR = 2.4e-16          # the project's float64 apply bar, of max |src| x the row's sum |w|
LDS_CHUNK = 1024             # entries of a 64-row run the apply kernel keeps in LDS (apply_mesh.h AM_CHUNK)


class Pair:
    """One mesh / grid pair with its reference, computed once: A from the oracle, the areas, the bar."""

    def __init__(self, o, m, g):
        self.m, self.g = m, g
        _, self.vxyz = mesh_xyz(o, m)
        self.kxyz = o.lonlat_deg_to_xyz(g.lon_c, g.lat_c)
        self.area_g = CR.grid_cell_areas(self.kxyz, g.nx, g.ny)
        self.area_c = CR.mesh_cell_areas(m.verticesOnCell, self.vxyz)
        self.A = o.conserve(m.verticesOnCell, self.vxyz, g.nx, g.ny, self.kxyz)[:3]
        self.tol = CR.tol_both(self.kxyz, g.nx, g.ny, m.verticesOnCell, self.vxyz)
        self.n_src = g.nx * g.ny
        self._b = {}

    def b_ref(self, norm):
        if norm not in self._b:
            self._b[norm] = CR.b_ref_from_csr(*self.A, self.area_g, self.area_c, norm)
            assert CR.sliver_share(self._b[norm][2]) <= CR.SLIVER_CAP, "the reference itself holds sliver-sized entries: change the seed"
        return self._b[norm]


@pytest.fixture(scope="module")
def case(gpu_lib, oracle):
    from mpassit_amd import regrid as R, synth, target_grid as tg
    g = tg.define_target_grid_params("lambert", 61, 41, dx=30000.0, dy=30000.0, **LAMBERT)
    meshes = dict(over=synth.regional_mesh_for_lambert(g.proj, 61, 41, 6001, margin=0.05, seed=11),
                  inside=synth.regional_mesh_for_lambert(g.proj, 61, 41, 5003, margin=-0.08, seed=12),
                  coarse=synth.regional_mesh_for_lambert(g.proj, 61, 41, 201, margin=0.05, seed=13))
    ga = R.Grid.from_proj(g, fill_target=False)
    gb, _ = _arrays_grid(R, ga)
    d = dict(g=g, ga=ga, gb=gb, m=meshes, mesh={k: R.Mesh.from_mpas(v) for k, v in meshes.items()},
             pair={k: Pair(oracle, v, g) for k, v in meshes.items()})
    yield d
    for v in d["mesh"].values():
        v.destroy()
    ga.destroy()
    gb.destroy()


def _check_store(R, rh, pair, norm, what):
    """Handle against B_ref of `pair`: shape, parity, ascending columns, frac; returns (rowptr, col, val, frac)."""
    m = pair.m
    assert (rh.n_src, rh.n_dst, rh.nx_dst, rh.ny_dst, rh.nnz_per_row) == (pair.n_src, m.nCells, m.nCells, 1, 0)
    rp, col, val = rh.csr()
    assert rp[0] == 0 and rp[-1] == rh.nnz == col.size and (np.diff(rp) >= 0).all()
    brp, bcol, bval, bfrac = pair.b_ref(norm)
    common, only_r, only_g = assert_csr_equal(brp, bcol, bval, rp, col, val, pair.n_src, tol=pair.tol)
    rows_of = np.repeat(np.arange(m.nCells), np.diff(rp))
    assert (np.diff(col.astype(np.int64))[rows_of[1:] == rows_of[:-1]] > 0).all(), "columns ascend within every row"
    frac = rh.dst_frac()
    dfrac = np.abs(frac - bfrac).max()
    print("%s norm %d: %d entries, %d common, %d / %d on one side only, bar %.1e, frac %.1e from the reference" % (
        what, norm, col.size, common, only_r, only_g, pair.tol, dfrac))
    assert common > 100 and dfrac < pair.tol
    rows = np.bincount(np.repeat(np.arange(m.nCells), np.diff(rp)), weights=val, minlength=m.nCells)
    covered = np.diff(rp) > 0
    assert (frac[~covered] == 0.0).all()
    if norm == CR.NORM_FRACAREA:
        assert np.abs(rows[covered] - 1.0).max() < pair.tol, "FRACAREA: covered rows sum to 1"
    else:
        assert np.abs(rows - frac).max() < pair.tol, "DSTAREA: a row sums to the cell's covered fraction"
    return rp, col, val, frac


@pytest.mark.parametrize("norm", NORMS, ids=["dstarea", "fracarea"])
@pytest.mark.parametrize("which", ["over", "inside", "coarse"])
def test_store_parity_lambert(case, which, norm):
    from mpassit_amd import regrid as R
    rh = R.regrid_store_conserve_to_mesh(case["ga"], case["mesh"][which], norm)
    assert rh.store_path == 1 and rh.store_stats[1] > 0 and rh.store_ms > 0.0
    rp, col, val, frac = _check_store(R, rh, case["pair"][which], norm, which)
    if which == "inside":
        assert np.abs(frac - 1.0).max() < case["pair"][which].tol, "every cell of the inside mesh is covered"
    if which == "over":
        assert (np.diff(rp) == 0).sum() > 10, "the overhanging mesh has uncovered cells: empty rows"
        assert ((frac > 1e-6) & (frac < 1.0 - 1e-6)).sum() > 10, "... and rim cells with 0 < frac < 1"
    if which == "coarse":
        run = rp[np.minimum(np.arange(0, rp.size - 1, 64) + 64, rp.size - 1)] - rp[np.arange(0, rp.size - 1, 64)]
        print("coarse mesh: longest row %d entries, longest 64-row run %d" % (np.diff(rp).max(), run.max()))
        assert np.diff(rp).max() >= 20 and run.max() > LDS_CHUNK, "the coarse mesh exercises the apply kernel's run chunking"
    rh.release()


def test_store_parity_latlon_grid(gpu_lib, oracle):
    """The regional 0.25-degree lat-lon grid, from its projection (index boxes) and from arrays (pyramid): parity and identity."""
    from mpassit_amd import regrid as R, synth, target_grid as tg
    g = tg.define_target_grid_params("lat-lon", 81, 61, dx=0.25, dy=0.25, ref_lat=30.0, ref_lon=-110.0, ref_x=1.0, ref_y=1.0, stand_lon=-110.0)
    m = synth.regional_mesh_for_lambert(g.proj, 81, 61, 4001, margin=0.04, seed=5)
    ga = R.Grid.from_proj(g, fill_target=False)
    gb, _ = _arrays_grid(R, ga)
    mesh = R.Mesh.from_mpas(m)
    pair = Pair(oracle, m, g)
    for norm in NORMS:
        ra, rb = R.regrid_store_conserve_to_mesh(ga, mesh, norm), R.regrid_store_conserve_to_mesh(gb, mesh, norm)
        assert ra.store_path == 1 and rb.store_path == 0
        _check_store(R, ra, pair, norm, "lat-lon 0.25")
        for x, y in zip(ra.csr() + (ra.dst_frac(),), rb.csr() + (rb.dst_frac(),)):
            assert np.array_equal(x, y)
        ra.release()
        rb.release()
    for obj in (mesh, ga, gb):
        obj.destroy()


def test_periodic_global_pair_and_conservation(gpu_lib, oracle):
    """synth.geodesic_mesh (2562 cells) under the periodic 72 x 36 lat-lon grid: pole slivers, every cell covered, the integral kept."""
    from mpassit_amd import regrid as R, synth, target_grid as tg
    g = tg.define_target_grid_params("lat-lon", nx=73, ny=37, stand_lon=0.0, is_regional=False)
    m = synth.geodesic_mesh(16)
    grid, mesh = R.Grid.from_target(g), R.Mesh.from_mpas(m)
    pair = Pair(oracle, m, g)
    assert abs(pair.area_g.sum() - 4 * np.pi) < 1e-10 and abs(pair.area_c.sum() - 4 * np.pi) < 1e-10
    for norm in NORMS:
        rh = R.regrid_store_conserve_to_mesh(grid, mesh, norm)
        rp, col, val, frac = _check_store(R, rh, pair, norm, "periodic global")
        assert np.abs(frac - 1.0).max() < pair.tol, "every cell of a global mesh is covered"
        # conservation: sum_c area(c) (B x)_c == sum_g area(g) x_g for an i.i.d. x
        x = np.random.default_rng(17).normal(size=pair.n_src)
        bx = oracle.apply_csr(rp, col, val, x[None, :], 1)[0]
        lhs, rhs = float((pair.area_c * bx).sum()), float((pair.area_g * x).sum())
        bar = pair.tol * float((pair.area_g * np.abs(x)).sum())
        print("conservation norm %d: %.3e apart, bar %.3e" % (norm, abs(lhs - rhs), bar))
        assert abs(lhs - rhs) <= bar
        rh.release()
    mesh.destroy()
    grid.destroy()


@pytest.mark.parametrize("norm", NORMS, ids=["dstarea", "fracarea"])
def test_library_equals_the_brute_force_goldens(gpu_lib, oracle, norm):
    """The four committed mesh / grid pairs through the C-ABI against B_ref built from their 50-digit entries."""
    from mpassit_amd import regrid as R
    from test_store_goldens import cases
    for c in cases():
        _, vxyz = mesh_xyz(oracle, c.mesh)
        kxyz = oracle.lonlat_deg_to_xyz(c.lon_c, c.lat_c)
        area_g, area_c = CR.grid_cell_areas(kxyz, c.nx, c.ny), CR.mesh_cell_areas(c.mesh.verticesOnCell, vxyz)
        gold = np.array(c.expect["conserve"], np.float64)
        brp, bcol, bval, bfrac = CR.b_ref(gold[:, 0].astype(np.int64), gold[:, 1].astype(np.int64), gold[:, 2], area_g, area_c, norm)
        tol = CR.tol_both(kxyz, c.nx, c.ny, c.mesh.verticesOnCell, vxyz)
        grid, mesh = R.Grid(c.lon, c.lat, c.lon_c, c.lat_c), R.Mesh.from_mpas(c.mesh)
        rh = R.regrid_store_conserve_to_mesh(grid, mesh, norm)
        rp, col, val = rh.csr()
        common, only_r, only_g = assert_csr_equal(brp, bcol, bval, rp, col, val, c.nx * c.ny, tol=tol)
        dfrac = np.abs(rh.dst_frac() - bfrac).max()
        print("%s: %d common, %d / %d one-sided, frac %.1e apart, bar %.1e" % (c.name, common, only_r, only_g, dfrac, tol))
        assert common > 100 and dfrac < tol
        rh.release()
        mesh.destroy()
        grid.destroy()


def test_determinism_routes_and_cache(case, gpu_lib):
    from mpassit_amd import regrid as R
    ga, gb, mesh = case["ga"], case["gb"], case["mesh"]["over"]
    fwd = R.regrid_store(mesh, ga, R.REGRIDMETHOD_CONSERVE)
    fwd0 = fwd.csr()
    ra = R.regrid_store_conserve_to_mesh(ga, mesh)
    rb = R.regrid_store_conserve_to_mesh(gb, mesh)
    assert ra.store_path == 1 and rb.store_path == 0
    wa = ra.csr() + (ra.dst_frac(),)
    for x, y in zip(wa, rb.csr() + (rb.dst_frac(),)):
        assert np.array_equal(x, y), "index boxes and the pyramid walk give the same bytes"
    # the same key again: the cached handle; the other norm: another handle; the Mesh -> Grid handle of the pair: untouched
    again = R.regrid_store_conserve_to_mesh(ga, mesh)
    other = R.regrid_store_conserve_to_mesh(ga, mesh, R.NORM_FRACAREA)
    assert again._h.value == ra._h.value and other._h.value != ra._h.value and fwd._h.value not in (ra._h.value, other._h.value)
    assert not np.array_equal(other.csr()[2], wa[2])
    for x, y in zip(fwd0, fwd.csr()):
        assert np.array_equal(x, y)
    fwd2 = R.regrid_store(mesh, ga, R.REGRIDMETHOD_CONSERVE)
    assert fwd2._h.value == fwd._h.value
    # store_boxes 0 on a fresh grid / mesh pair (nothing from the cache), and a second build from scratch: the same bytes
    ga2, mesh2 = R.Grid.from_proj(case["g"], fill_target=False), R.Mesh.from_mpas(case["m"]["over"])
    gpu_lib.tune("store_boxes", 0)
    try:
        r0 = R.regrid_store_conserve_to_mesh(ga2, mesh2)
    finally:
        gpu_lib.tune("store_boxes", 1)
    assert r0.store_path == 0 and r0._h.value != ra._h.value
    for x, y in zip(wa, r0.csr() + (r0.dst_frac(),)):
        assert np.array_equal(x, y)
    ga3, mesh3 = R.Grid.from_proj(case["g"], fill_target=False), R.Mesh.from_mpas(case["m"]["coarse"])
    rc1 = R.regrid_store_conserve_to_mesh(case["ga"], case["mesh"]["coarse"])
    rc3 = R.regrid_store_conserve_to_mesh(ga3, mesh3)
    for x, y in zip(rc1.csr(), rc3.csr()):
        assert np.array_equal(x, y), "two builds of the coarse pair (cooperative passes) give the same bytes"
    for rh in (fwd, fwd2, ra, rb, again, other, r0, rc1, rc3):
        rh.release()
    # parked handles go with their mesh
    mesh2.destroy()
    ga2.destroy()
    mesh3.destroy()
    ga3.destroy()


# ---- the apply --------------------------------------------------------------------------------------------------------------------
def _check_apply(R, rh, nlev, nfields, sdt, ddt, scale, offset, seed, pitched_src=None):
    """CELL_FAST == regrid_typed, LEV_FAST == its transposition, fields batched == single calls, pitched source == dense source; the
    results land in NaN-filled, canary-banded buffers."""
    import torch
    from _oracle_compare import Banded
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    src = ((torch.rand((nfields, nlev, rh.n_src), dtype=torch.float64, device="cuda", generator=gen) - 0.5) * 80.0).to(sdt)
    want = rh.regrid_typed(src.reshape(-1), nlev=nlev, nfields=nfields, out_dtype=ddt, scale=scale, offset=offset).reshape(nfields, nlev, rh.n_dst)
    n = nfields * nlev * rh.n_dst
    bc, bl = Banded(torch, n, ddt, shift=3), Banded(torch, n, ddt, shift=5)
    cf = rh.regrid_csr_to_mesh(src, nlev=nlev, nfields=nfields, layout=R.LAYOUT_CELL_FAST, scale=scale, offset=offset, out=bc.res)
    lf = rh.regrid_csr_to_mesh(src, nlev=nlev, nfields=nfields, layout=R.LAYOUT_LEV_FAST, scale=scale, offset=offset, out=bl.res)
    torch.cuda.synchronize()
    bc.assert_canaries("CELL_FAST")
    bl.assert_canaries("LEV_FAST")
    cf, lf = cf.reshape(nfields, nlev, rh.n_dst), lf.reshape(nfields, rh.n_dst, nlev)
    assert not torch.isnan(cf).any() and not torch.isnan(lf).any(), "an element was left unwritten"
    assert _bytes_equal(cf, want), "CELL_FAST differs from regrid_typed"
    assert _bytes_equal(lf, want.transpose(1, 2).contiguous()), "LEV_FAST is not the transposition of regrid_typed"
    again = rh.regrid_csr_to_mesh(src, nlev=nlev, nfields=nfields, layout=R.LAYOUT_LEV_FAST, out_dtype=ddt, scale=scale, offset=offset)
    assert tuple(again.shape) == (nfields, rh.n_dst, nlev) and _bytes_equal(again, lf)
    if nfields > 1:
        for f in range(nfields):
            one = rh.regrid_csr_to_mesh(src[f].contiguous(), nlev=nlev, layout=R.LAYOUT_LEV_FAST, out_dtype=ddt, scale=scale, offset=offset)
            assert _bytes_equal(one[0], lf[f]), "field %d of a batch differs from its single call" % f
    if pitched_src is not None:
        ny, nx = pitched_src
        ld = (ny * nx + 37) // 32 * 32 + 32
        buf = torch.full((nfields * nlev * ld,), float("nan"), dtype=sdt, device="cuda")
        view = buf.as_strided((nfields, nlev, ny, nx), (nlev * ld, ld, nx, 1))
        view.copy_(src.reshape(nfields, nlev, ny, nx))
        for layout, ref in ((R.LAYOUT_CELL_FAST, cf), (R.LAYOUT_LEV_FAST, lf)):
            got = rh.regrid_csr_to_mesh(view, nlev=nlev, nfields=nfields, layout=layout, out_dtype=ddt, scale=scale, offset=offset)
            assert _bytes_equal(got, ref), "pitched source differs from dense (its NaN pad was read?)"
    return src, want


def _dtypes(types):
    import torch
    dt = {"f64": torch.float64, "f32": torch.float32}
    return dt[types[:3]], dt[types[3:]]


@pytest.mark.parametrize("nlev", [1, 2, 3, 16, 17, 55])
@pytest.mark.parametrize("types", ["f64f64", "f32f32", "f32f64", "f64f32"])
def test_apply_identities_on_this_stores_handle(case, types, nlev):
    """6001-ish cells (no multiple of 64), empty rows, rows of 1 .. ~9 entries; 16 / 17: either side of one pass of 4 waves x 4 levels."""
    from mpassit_amd import regrid as R
    sdt, ddt = _dtypes(types)
    rh = R.regrid_store_conserve_to_mesh(case["ga"], case["mesh"]["over"])
    assert rh.n_dst % 64 != 0
    g = case["g"]
    for nfields in (1, 3):
        _check_apply(R, rh, nlev, nfields, sdt, ddt, 1.0, 0.0, 100 + nlev + nfields, pitched_src=(g.ny, g.nx))
        _check_apply(R, rh, nlev, nfields, sdt, ddt, 9.81, -300.0, 200 + nlev + nfields)
    rh.release()


@pytest.mark.parametrize("types,nlev", [("f64f64", 127), ("f64f64", 128), ("f32f64", 128), ("f32f32", 255), ("f32f32", 256), ("f64f32", 256)])
def test_apply_level_chunks_and_run_chunks(case, types, nlev):
    """Either side of the [cell][lev] tile's level-chunk threshold (float64 results: 128 levels, float32: 256), on the COARSE mesh, whose
    64-row runs also outgrow the LDS chunk of entries -- and on the fine one."""
    from mpassit_amd import regrid as R
    sdt, ddt = _dtypes(types)
    g = case["g"]
    rh = R.regrid_store_conserve_to_mesh(case["ga"], case["mesh"]["coarse"], R.NORM_FRACAREA)
    _check_apply(R, rh, nlev, 2, sdt, ddt, 2.0, 1.0, 5 + nlev, pitched_src=(g.ny, g.nx))
    rh.release()
    rh = R.regrid_store_conserve_to_mesh(case["ga"], case["mesh"]["inside"])
    _check_apply(R, rh, nlev, 1, sdt, ddt, 1.0, 0.0, 6 + nlev)
    rh.release()


@pytest.mark.parametrize("types", ["f64f64", "f32f32", "f32f64", "f64f32"])
def test_apply_serves_every_csr_handle(case, types):
    """A Mesh -> Grid conservative handle (rows = grid cells) and a from-weights handle (unsorted, with duplicates), and the coarse Store."""
    from mpassit_amd import regrid as R
    sdt, ddt = _dtypes(types)
    g = case["g"]
    fwd = R.regrid_store(case["mesh"]["coarse"], case["ga"], R.REGRIDMETHOD_CONSERVE)
    coarse = R.regrid_store_conserve_to_mesh(case["ga"], case["mesh"]["coarse"])
    rp, col, val = coarse.csr()
    rows = np.repeat(np.arange(coarse.n_dst), np.diff(rp))
    perm = np.random.default_rng(3).permutation(col.size)
    dup = perm[:50]
    fw = R.RouteHandle.from_weights(coarse.n_src, coarse.n_dst, 1, np.concatenate([rows[perm], rows[dup]]) + 1, np.concatenate([col[perm], col[dup]]) + 1,
                                    np.concatenate([val[perm], 0.5 * val[dup]]))
    assert fwd.nnz_per_row == 0 and fw.nnz_per_row == 0 and fw.nnz == col.size + 50
    for rh, pitched in ((fwd, (1, fwd.n_src)), (fw, (g.ny, g.nx)), (coarse, (g.ny, g.nx))):
        for nlev in (3, 55):
            for nfields in (1, 3):
                _check_apply(R, rh, nlev, nfields, sdt, ddt, 0.5, 3.0, 31 + nlev + nfields, pitched_src=pitched)
        rh.release()


def test_apply_empty_rows_values_and_masked_fill(case, oracle):
    import torch
    from mpassit_amd import regrid as R
    rh = R.regrid_store_conserve_to_mesh(case["ga"], case["mesh"]["over"])
    rp, col, val = rh.csr()
    empty = torch.as_tensor(np.diff(rp) == 0, device="cuda")
    assert empty.any()
    nlev, scale, offset = 7, 9.81, -300.0
    src, _ = _check_apply(R, rh, nlev, 1, torch.float64, torch.float64, 1.0, 0.0, 77)
    # an empty row gives (T)(0 * scale + offset)
    for ddt in (torch.float64, torch.float32):
        for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
            out = rh.regrid_csr_to_mesh(src, nlev=nlev, layout=layout, out_dtype=ddt, scale=scale, offset=offset)[0]
            out = out if layout == R.LAYOUT_CELL_FAST else out.t()
            zero = torch.tensor(0.0 * scale + offset, dtype=torch.float64).to(ddt)
            assert (out[:, empty] == zero).all()
    # values against the oracle's apply on the handle's own weights: the float64 apply bar per row
    ref = torch.as_tensor(oracle.apply_csr(rp, col, val, src.cpu().numpy().reshape(nlev, -1), nlev), device="cuda")
    got = rh.regrid_csr_to_mesh(src, nlev=nlev, layout=R.LAYOUT_LEV_FAST)[0].t().contiguous()
    sabs = np.bincount(np.repeat(np.arange(rh.n_dst), np.diff(rp)), weights=np.abs(val), minlength=rh.n_dst)
    bar = torch.as_tensor(APPLY_BAR * sabs, device="cuda") * float(src.abs().max())
    d = (got - ref).abs()
    worst = float((d / torch.clamp(bar, min=1e-300))[:, ~empty].max())
    print("apply vs oracle.apply_csr: largest difference %.3e, %.3f of the row's bar at worst" % (float(d.max()), worst))
    assert (d[:, empty] == 0.0).all() and not torch.isnan(got).any()
    assert bool((d <= bar).all()), "apply differs from the oracle's by %.3f of the bar" % worst
    # regrid_masked fills the uncovered cells and keeps the bits of the covered ones
    plain = rh.regrid_typed(src.reshape(-1), nlev=nlev).reshape(nlev, -1)
    masked = rh.regrid_masked(src.reshape(-1), nlev=nlev, fill_value=float("nan")).reshape(nlev, -1)
    assert torch.isnan(masked[:, empty]).all() and not torch.isnan(masked[:, ~empty]).any()
    assert _bytes_equal(masked[:, ~empty].contiguous(), plain[:, ~empty].contiguous()), "covered cells keep the unmasked bits"
    rh.release()


def test_adjoint_and_autograd(case, gpu_lib):
    import torch
    from mpassit_amd import regrid as R
    rh = R.regrid_store_conserve_to_mesh(case["ga"], case["mesh"]["over"])
    rng = np.random.default_rng(11)
    nlev = 2
    x = torch.as_tensor(rng.normal(size=(nlev, rh.n_src)), device="cuda")
    y = torch.as_tensor(rng.normal(size=(nlev, rh.n_dst)), device="cuda")
    bx = rh.regrid_csr_to_mesh(x, nlev=nlev).reshape(nlev, -1)
    bty = rh.regrid_transpose(y, nlev=nlev).reshape(nlev, -1)
    lhs, rhs = float((bx * y).sum()), float((x * bty).sum())
    assert abs(lhs - rhs) <= 1e-13 * float(bx.norm() * y.norm())     # the expression and bar of tests/test_transpose_gpu.py
    for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
        for dt in (torch.float64, torch.float32):
            xs = x.to(dt).clone().requires_grad_(True)
            out = R.regrid_csr_to_mesh_autograd(rh, xs, nlev=nlev, layout=layout)
            assert _bytes_equal(out.detach(), rh.regrid_csr_to_mesh(xs.detach(), nlev=nlev, layout=layout))
            up = torch.as_tensor(rng.normal(size=tuple(out.shape)), device="cuda").to(dt)
            out.backward(up)
            up_cf = up if layout == R.LAYOUT_CELL_FAST else up.transpose(1, 2).contiguous()
            want = rh.regrid_transpose(up_cf.reshape(1, nlev, rh.n_dst), nlev=nlev, out_dtype=dt).reshape(xs.shape)
            assert torch.equal(xs.grad, want)
    rh.release()
    # gradcheck at a few dozen cells
    from mpassit_amd import synth, target_grid as tg
    g = tg.define_target_grid_params("lambert", 9, 8, dx=120000.0, dy=120000.0, **LAMBERT)
    m = synth.regional_mesh_for_lambert(g.proj, 9, 8, 40, margin=0.05, seed=4)
    grid, mesh = R.Grid.from_proj(g, fill_target=False), R.Mesh.from_mpas(m)
    small = R.regrid_store_conserve_to_mesh(grid, mesh)
    assert 20 <= small.n_dst <= 100 and small.nnz > small.n_dst
    for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
        xs = torch.as_tensor(rng.normal(size=(1, 2, small.n_src)), device="cuda").requires_grad_(True)
        assert torch.autograd.gradcheck(lambda t: R.regrid_csr_to_mesh_autograd(small, t, nlev=2, layout=layout), (xs,), eps=1e-6, atol=1e-7)
    small.release()
    mesh.destroy()
    grid.destroy()


def test_graph_capture_on_the_first_call(gpu_lib):
    """A fresh handle's very first regrid_csr_to_mesh is captured (after mpg_warmup_wait) and replayed: the bytes of the eager call."""
    import torch
    from mpassit_amd import regrid as R, synth, target_grid as tg
    g = tg.define_target_grid_params("lambert", 51, 35, dx=30000.0, dy=30000.0, **LAMBERT)
    m = synth.regional_mesh_for_lambert(g.proj, 51, 35, 3001, margin=0.03, seed=21)
    grid, mesh = R.Grid.from_proj(g, fill_target=False), R.Mesh.from_mpas(m)
    rh = R.regrid_store_conserve_to_mesh(grid, mesh)
    assert gpu_lib.load().mpg_warmup_wait() == 0
    nlev = 55
    src = torch.rand((nlev, rh.n_src), dtype=torch.float32, device="cuda")
    out_lf = torch.full((1, rh.n_dst, nlev), float("nan"), dtype=torch.float32, device="cuda")
    out_cf = torch.full((1, nlev, rh.n_dst), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):        # one stream: a chain, no parallel branches
            rh.regrid_csr_to_mesh(src, nlev=nlev, layout=R.LAYOUT_LEV_FAST, out=out_lf, scale=2.0, offset=1.0)
            rh.regrid_csr_to_mesh(src, nlev=nlev, layout=R.LAYOUT_CELL_FAST, out=out_cf)
    for trial in range(2):
        src.mul_(-0.5).add_(0.25)
        graph.replay()
        torch.cuda.synchronize()
        got_lf, got_cf = out_lf.clone(), out_cf.clone()
        assert _bytes_equal(got_lf, rh.regrid_csr_to_mesh(src, nlev=nlev, layout=R.LAYOUT_LEV_FAST, scale=2.0, offset=1.0))
        assert _bytes_equal(got_cf, rh.regrid_csr_to_mesh(src, nlev=nlev, layout=R.LAYOUT_CELL_FAST, out_dtype=torch.float64))
    rh.release()
    mesh.destroy()
    grid.destroy()


def test_refusals(case, gpu_lib):
    import torch
    from mpassit_amd import _lib as L, regrid as R, synth
    lib = L.load()

    def refused(rc, want, word=None):
        msg = lib.mpg_last_error().decode()
        assert rc == want and msg, (rc, want, msg)
        if word:
            assert word in msg, msg

    h = C.c_void_p()
    ga, mesh = case["ga"], case["mesh"]["over"]
    refused(L.regrid_store_conserve_to_mesh(None, mesh._h, 0, C.byref(h)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(L.regrid_store_conserve_to_mesh(ga._h, None, 0, C.byref(h)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(L.regrid_store_conserve_to_mesh(ga._h, mesh._h, 0, None), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(L.regrid_store_conserve_to_mesh(ga._h, mesh._h, 2, C.byref(h)), L.MPG_ERR_INVALID_ARG, "norm_type")
    refused(L.regrid_store_conserve_to_mesh(ga._h, mesh._h, -1, C.byref(h)), L.MPG_ERR_INVALID_ARG, "norm_type")
    # a grid without CORNER coordinates
    g = case["g"]
    bare = R.Grid(g.lon, g.lat)
    refused(L.regrid_store_conserve_to_mesh(bare._h, mesh._h, 0, C.byref(h)), L.MPG_ERR_INVALID_ARG, "CORNER")
    bare.destroy()
    # a mesh cut to a grid's window
    wmesh = R.Mesh.from_mpas(case["m"]["over"], window_grid=case["gb"])
    refused(L.regrid_store_conserve_to_mesh(case["gb"]._h, wmesh._h, 0, C.byref(h)), L.MPG_ERR_UNSUPPORTED, "window")
    wmesh.destroy()
    # maxEdges > 12
    m = case["m"]["coarse"]
    wide = synth.MpasMesh(m.latCell, m.lonCell, m.latVertex, m.lonVertex,
                          np.concatenate([m.verticesOnCell, np.zeros((m.nCells, 13 - m.maxEdges), np.int32)], axis=1))
    wm = R.Mesh.from_mpas(wide)
    refused(L.regrid_store_conserve_to_mesh(ga._h, wm._h, 0, C.byref(h)), L.MPG_ERR_UNSUPPORTED, "maxEdges")
    wm.destroy()
    # the old entry points keep refusing and name the new calls
    refused(L.regrid_store_to_mesh(ga._h, 0, mesh._h, 0, R.REGRIDMETHOD_CONSERVE, C.byref(h)), L.MPG_ERR_UNSUPPORTED, "mpg_regrid_store_conserve_to_mesh")
    # dst_frac on a handle that has none
    fwd = R.regrid_store(case["mesh"]["inside"], ga, R.REGRIDMETHOD_CONSERVE)
    buf = np.zeros(fwd.n_dst)
    refused(L.handle_get_dst_frac(fwd._h, buf.ctypes.data), L.MPG_ERR_INVALID_ARG, "fraction")
    refused(L.handle_get_dst_frac(None, buf.ctypes.data), L.MPG_ERR_INVALID_ARG)
    with pytest.raises(L.MpgError) as e:
        fwd.regrid_to_mesh(torch.zeros(fwd.n_src, dtype=torch.float64, device="cuda"))
    assert e.value.rc == L.MPG_ERR_UNSUPPORTED and "mpg_regrid_csr_to_mesh_dev" in str(e.value)
    fwd.release()
    # the apply
    rh = R.regrid_store_conserve_to_mesh(ga, mesh)
    refused(L.handle_get_dst_frac(rh._h, None), L.MPG_ERR_INVALID_ARG)
    src = torch.zeros(2 * rh.n_src, dtype=torch.float64, device="cuda")
    dst = torch.zeros(2 * rh.n_dst, dtype=torch.float64, device="cuda")
    args = lambda **kw: [kw.get("rh", rh._h), kw.get("src", src.data_ptr()), kw.get("st", 0), kw.get("ld", 0), kw.get("nlev", 2), kw.get("nf", 1),   # noqa: E731
                         kw.get("dst", dst.data_ptr()), kw.get("dt", 0), kw.get("layout", 1), 1.0, 0.0, None]
    refused(L.regrid_csr_to_mesh_dev(*args(st=2)), L.MPG_ERR_UNSUPPORTED, "big-endian")
    refused(L.regrid_csr_to_mesh_dev(*args(dt=3)), L.MPG_ERR_UNSUPPORTED, "big-endian")
    refused(L.regrid_csr_to_mesh_dev(*args(ld=rh.n_src - 1)), L.MPG_ERR_INVALID_ARG, "below the plane size")
    refused(L.regrid_csr_to_mesh_dev(*args(layout=2)), L.MPG_ERR_INVALID_ARG, "dst_layout")
    refused(L.regrid_csr_to_mesh_dev(*args(nlev=0)), L.MPG_ERR_INVALID_ARG, "nlev")
    refused(L.regrid_csr_to_mesh_dev(*args(nf=0)), L.MPG_ERR_INVALID_ARG, "nfields")
    refused(L.regrid_csr_to_mesh_dev(*args(rh=None)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(L.regrid_csr_to_mesh_dev(*args(src=None)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(L.regrid_csr_to_mesh_dev(*args(dst=None)), L.MPG_ERR_INVALID_ARG, "NULL")
    assert L.regrid_csr_to_mesh_dev(*args()) == 0 and L.regrid_csr_to_mesh_dev(*args(ld=rh.n_src)) == 0
    torch.cuda.synchronize()
    rh.release()
    # fixed handles: served by the other call
    fx = R.regrid_store_to_mesh(ga, mesh)
    with pytest.raises(L.MpgError) as e:
        fx.regrid_csr_to_mesh(torch.zeros(fx.n_src, dtype=torch.float64, device="cuda"))
    assert e.value.rc == L.MPG_ERR_UNSUPPORTED and "mpg_regrid_to_mesh_dev" in str(e.value)
    fx.release()


def test_cache_lifetime_and_source_window(gpu_lib):
    """Parked handles go with their mesh or grid; mpg_mesh_set_source_window passes the handle by; getters and re-indexing work."""
    from mpassit_amd import regrid as R, synth, target_grid as tg
    g = tg.define_target_grid_params("lambert", 41, 31, dx=30000.0, dy=30000.0, **LAMBERT)
    m = synth.regional_mesh_for_lambert(g.proj, 41, 31, 3001, margin=0.3, seed=3)
    grid, mesh = R.Grid.from_proj(g, fill_target=False), R.Mesh.from_mpas(m)
    a = R.regrid_store_conserve_to_mesh(grid, mesh)
    addr, w0 = a._h.value, a.csr()
    a.release()
    a = R.regrid_store_conserve_to_mesh(grid, mesh)
    assert a._h.value == addr, "a released handle stays parked"
    fwd = R.regrid_store(mesh, grid, R.REGRIDMETHOD_CONSERVE)
    first, end = fwd.source_range()
    assert first > 0 and end <= m.nCells
    mesh.set_source_window(first, end - first)
    fwd._refresh()
    a._refresh()
    assert fwd.n_src == end - first and a.n_src == g.nx * g.ny and a.n_dst == m.nCells
    for x, y in zip(w0, a.csr()):
        assert np.array_equal(x, y), "the to-mesh handle is untouched by the mesh's source window"
    b = R.regrid_store_conserve_to_mesh(grid, mesh, R.NORM_FRACAREA)           # a Store under the window: its sources are grid cells still
    assert b.n_src == g.nx * g.ny
    b.release()
    mesh.set_source_window(0, m.nCells)
    ids = a.unique_sources()
    assert ids.size > 0 and ids.max() < a.n_src
    f0, e0 = a.source_range()
    assert 0 <= f0 < e0 <= a.n_src
    fwd.release()
    a.release()
    # destroy the mesh with the handle parked, build the same pair again: a fresh Store, the same bytes
    mesh.destroy()
    mesh = R.Mesh.from_mpas(m)
    a = R.regrid_store_conserve_to_mesh(grid, mesh)
    for x, y in zip(w0, a.csr()):
        assert np.array_equal(x, y)
    a.release()
    mesh.destroy()
    grid.destroy()
