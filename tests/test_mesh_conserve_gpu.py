"""Conservative Mesh -> Mesh on the GPU at a few thousand cells: the Store (mpg_regrid_store_conserve_mesh) against the float64 numpy
reference of I(d, s) (tests/_mesh_conserve_ref.py, qualified on the CPU by tests/test_mesh_conserve_ref.py) on the four cell pairs of
tests/_mesh_to_mesh_cases.py and both normalisations, and its properties: dst fraction, row sums, conservation, src == dst, a renumbered
source, determinism from scratch, cache, source window, refusals.  The bar is the project's conservative one with h over BOTH meshes'
cells: max(1e-11, 64 eps / min h)."""
import ctypes as C

import numpy as np
import pytest

import _mesh_conserve_ref as MR
import _mesh_to_mesh_cases as MC
from _parity_helpers import assert_csr_equal

pytestmark = pytest.mark.gpu

NORMS = [MR.NORM_DSTAREA, MR.NORM_FRACAREA]
_NAMES = {"geo10_to_vor1500": ("geo10", "vor1500"), "vor2500_to_hex": ("vor2500", "hex_small"), "hex_to_geo10": ("hex_large", "geo10"),
          "varres3000_to_geo8": ("varres3000", "geo8")}


@pytest.fixture(scope="module")
def dev(gpu_lib):
    """Device meshes by name, created on first use, destroyed at the end of the module."""
    from mpassit_amd import regrid as R
    made = {}

    def get(name):
        if name not in made:
            made[name] = R.Mesh.from_mpas(MC.mesh(name))
        return made[name]

    yield get
    for m in made.values():
        m.destroy()


def _check_store(rh, a, norm, what):
    """Handle against the reference Answer `a`: shape, parity, ascending columns, frac, row sums; returns (rowptr, col, val, frac)."""
    n_src, n_dst = a.src.nCells, a.dst.nCells
    assert (rh.n_src, rh.n_dst, rh.nx_dst, rh.ny_dst, rh.nnz_per_row) == (n_src, n_dst, n_dst, 1, 0)
    rp, col, val = rh.csr()
    assert rp[0] == 0 and rp[-1] == rh.nnz == col.size and (np.diff(rp) >= 0).all()
    brp, bcol, bval, bfrac = a.rows(norm)
    common, only_r, only_g = assert_csr_equal(brp, bcol, bval, rp, col, val, n_src, tol=a.tol)
    rows_of = np.repeat(np.arange(n_dst), np.diff(rp))
    assert (np.diff(col.astype(np.int64))[rows_of[1:] == rows_of[:-1]] > 0).all(), "columns ascend strictly within every row"
    frac = rh.dst_frac()
    dfrac = np.abs(frac - bfrac).max()
    print("%s norm %d: %d entries, %d common, %d / %d on one side only, bar %.1e, frac %.1e from the reference" % (
        what, norm, col.size, common, only_r, only_g, a.tol, dfrac))
    assert common > 100 and dfrac < a.tol
    sums = np.bincount(rows_of, weights=val, minlength=n_dst)
    covered = np.diff(rp) > 0
    assert (frac[~covered] == 0.0).all()
    if norm == MR.NORM_FRACAREA:
        assert np.abs(sums[covered] - 1.0).max() < a.tol, "FRACAREA: covered rows sum to 1"
    else:
        assert np.abs(sums - frac).max() < a.tol, "DSTAREA: a row sums to the cell's covered fraction"
    return rp, col, val, frac


@pytest.mark.parametrize("norm", NORMS, ids=["dstarea", "fracarea"])
@pytest.mark.parametrize("name", MR.PAIRS)
def test_store_parity(dev, oracle, name, norm):
    from mpassit_amd import regrid as R
    a = MR.answer(oracle, name)
    src, dst = dev(_NAMES[name][0]), dev(_NAMES[name][1])
    rh = R.regrid_store_conserve_mesh(src, dst, norm)
    st = rh.store_stats
    print("%s: %d pairs clipped (reference caps: %d), %d vertex slots, tree %d us, Store %.2f ms" % (name, st[1], a.d.size, st[6], st[3], rh.store_ms))
    assert st[1] >= int((a.inter > 0.0).sum()) and st[2] == 0 and rh.store_ms > 0.0 and rh.store_path == 0
    assert st[6] == int(a.ps[1].max() + a.pd[1].max()) <= 24, "vertex slots = the two meshes' largest valences added"
    rp, col, val, frac = _check_store(rh, a, norm, name)
    if name == "hex_to_geo10":
        assert (np.diff(rp) == 0).sum() > 100 and ((frac > 1e-6) & (frac < 1.0 - 1e-6)).sum() > 10 and np.diff(rp).max() > 24
    else:
        assert np.abs(frac - 1.0).max() < a.tol, "a global source covers every destination cell"
    if name == "varres3000_to_geo8":
        assert np.diff(rp).max() >= 64
    rh.release()


@pytest.mark.parametrize("name", ["geo10_to_vor1500", "varres3000_to_geo8"])
def test_conservation_global_to_global(dev, oracle, name):
    """sum_d area(d) (B x)_d == sum_s area(s) x_s for an i.i.d. x, DSTAREA, within tol * sum area |x|."""
    from mpassit_amd import regrid as R
    a = MR.answer(oracle, name)
    assert abs(a.area_s.sum() - 4 * np.pi) < 1e-10 and abs(a.area_d.sum() - 4 * np.pi) < 1e-10
    rh = R.regrid_store_conserve_mesh(dev(_NAMES[name][0]), dev(_NAMES[name][1]))
    rp, col, val = rh.csr()
    x = np.random.default_rng(17).normal(size=a.src.nCells)
    bx = oracle.apply_csr(rp, col, val, x[None, :], 1)[0]
    lhs, rhs = float((a.area_d * bx).sum()), float((a.area_s * x).sum())
    bar = a.tol * float((a.area_s * np.abs(x)).sum())
    print("conservation %s: %.3e apart, bar %.3e" % (name, abs(lhs - rhs), bar))
    assert abs(lhs - rhs) <= bar
    rh.release()


@pytest.mark.parametrize("which", ["geo10", "vor1500"])
def test_identity_src_is_dst(dev, oracle, which):
    """src == dst: the diagonal within the bar of 1; an off-diagonal entry may exist (a neighbour's sliver above the 1e-14 rule on the
    device and below it in the reference, or the other way round) but only below SLIVER -- assert_csr_equal's one-sided rule."""
    from mpassit_amd import regrid as R
    a = MR.answer(oracle, which + "_self")
    m = dev(which)
    for norm in NORMS:
        rh = R.regrid_store_conserve_mesh(m, m, norm)
        rp, col, val, frac = _check_store(rh, a, norm, which + " onto itself")
        rows_of = np.repeat(np.arange(a.dst.nCells), np.diff(rp))
        diag = rows_of == col
        assert diag.sum() == a.dst.nCells and np.abs(val[diag] - 1.0).max() < a.tol
        assert (val[~diag] < MR.SLIVER).all()
        rh.release()


def test_renumbered_source_cells(gpu_lib, oracle):
    """The source cells shuffled: the same matrix under the permutation, within the bar (the clip of a pair does not depend on either
    cell's number; the candidate walk and the insertion order do, and must not matter)."""
    from mpassit_amd import regrid as R, synth
    src_m, dst_m, _ = MC.pair("varres3000_to_geo8")
    a = MR.answer(oracle, "varres3000_to_geo8")
    shuf = synth.shuffle_cells(src_m)
    perm = np.random.default_rng(synth.SEED + 7).permutation(src_m.nCells)          # new id i holds old cell perm[i]
    assert np.array_equal(shuf.latCell, src_m.latCell[perm]) and np.array_equal(shuf.verticesOnCell, src_m.verticesOnCell[perm])
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.size)
    src, dst = R.Mesh.from_mpas(shuf), R.Mesh.from_mpas(dst_m)
    for norm in NORMS:
        rh = R.regrid_store_conserve_mesh(src, dst, norm)
        rp, col, val = rh.csr()
        brp, bcol, bval, bfrac = a.rows(norm)
        common, only_r, only_g = assert_csr_equal(brp, inv[bcol], bval, rp, col, val, src_m.nCells, tol=a.tol)
        print("shuffled source, norm %d: %d common, %d / %d on one side only" % (norm, common, only_r, only_g))
        assert common > 1000 and np.abs(rh.dst_frac() - bfrac).max() < a.tol
        rows_of = np.repeat(np.arange(dst_m.nCells), np.diff(rp))
        assert (np.diff(col.astype(np.int64))[rows_of[1:] == rows_of[:-1]] > 0).all()
        rh.release()
    src.destroy()
    dst.destroy()


def test_determinism_from_scratch(gpu_lib):
    """Nothing of the first Store is left (both meshes destroyed: the cache entry, the tree): a second Store of the same pair on new
    meshes gives the same bytes."""
    from mpassit_amd import regrid as R
    src_m, dst_m, _ = MC.pair("hex_to_geo10")
    got = []
    for trial in range(2):
        src, dst = R.Mesh.from_mpas(src_m), R.Mesh.from_mpas(dst_m)
        for norm in NORMS:
            rh = R.regrid_store_conserve_mesh(src, dst, norm)
            assert rh.store_ms > 0.0 and (rh.store_stats[3] > 0) == (norm == NORMS[0]), "the first Store of a source mesh builds its cell tree"
            got.append(rh.csr() + (rh.dst_frac(),))
            rh.release()
        src.destroy()
        dst.destroy()
    for x, y in zip(got[0] + got[1], got[2] + got[3]):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), "rowptr, col, val and frac are byte-identical"


def test_cache(gpu_lib):
    from mpassit_amd import regrid as R
    src, dst = R.Mesh.from_mpas(MC.mesh("geo8")), R.Mesh.from_mpas(MC.mesh("vor1500"))
    a = R.regrid_store_conserve_mesh(src, dst)
    assert a.store_stats[3] > 0, "the first conservative Store of a source mesh builds its cell tree"
    b = R.regrid_store_conserve_mesh(src, dst)
    assert a._h.value == b._h.value, "a second Store with the same arguments returns the cached handle"
    f = R.regrid_store_conserve_mesh(src, dst, R.NORM_FRACAREA)
    assert f._h.value != a._h.value and f.store_stats[3] == 0, "the two norms are two handles; the tree is kept on the mesh"
    bil = R.regrid_store_mesh(src, dst)
    rev = R.regrid_store_conserve_mesh(dst, src)
    assert len({a._h.value, f._h.value, bil._h.value, rev._h.value}) == 4 and (rev.n_src, rev.n_dst) == (a.n_dst, a.n_src)
    for rh in (b, f, bil, rev):
        rh.release()
    # a released handle stays parked: the Store again returns it
    addr, wa = a._h.value, a.csr() + (a.dst_frac(),)
    a.release()
    a = R.regrid_store_conserve_mesh(src, dst)
    assert a._h.value == addr
    a.release()
    # destroying EITHER mesh drops the parked entry: a new mesh at whatever address stores anew (the same bytes)
    dst.destroy()
    dst2 = R.Mesh.from_mpas(MC.mesh("vor1500"))
    a2 = R.regrid_store_conserve_mesh(src, dst2)
    assert a2.store_ms > 0.0 and a2.store_stats[3] == 0 and all(np.array_equal(x, y) for x, y in zip(wa, a2.csr() + (a2.dst_frac(),)))
    a2.release()
    src.destroy()
    src2 = R.Mesh.from_mpas(MC.mesh("geo8"))
    a3 = R.regrid_store_conserve_mesh(src2, dst2)
    assert a3.store_stats[3] > 0, "a new source mesh builds a tree of its own: nothing of the destroyed one was found"
    assert all(np.array_equal(x, y) for x, y in zip(wa, a3.csr() + (a3.dst_frac(),)))
    a3.release()
    src2.destroy()
    dst2.destroy()


def test_source_window(gpu_lib):
    """A window on the SOURCE mesh rebases the columns, and the Regrid from the windowed slab has the bits of the Regrid from the whole
    slab; a window on the destination mesh does not touch the handle."""
    import torch
    from mpassit_amd import regrid as R
    src_m, dst_m, _ = MC.pair("vor2500_to_hex")
    src, dst = R.Mesh.from_mpas(src_m), R.Mesh.from_mpas(dst_m)
    rh = R.regrid_store_conserve_mesh(src, dst)
    first, end = rh.source_range()
    assert 0 < first < end < src_m.nCells, "the region references a band of the global mesh's cells"
    rp0, c0, v0 = rh.csr()
    nlev = 5
    field = torch.as_tensor(MC.smooth_field(src_m, nlev), device="cuda")
    whole = rh.regrid_csr_rows(field, nlev=nlev)
    dst.set_source_window(3, dst_m.nCells - 7)
    for x, y in zip((rp0, c0, v0), rh.csr()):
        assert np.array_equal(x, y), "a window on the destination mesh passes the handle by"
    dst.set_source_window(0, dst_m.nCells)
    src.set_source_window(first, end - first)
    rh._refresh()
    assert rh.n_src == end - first
    rp1, c1, v1 = rh.csr()
    assert np.array_equal(rp0, rp1) and np.array_equal(c0 - first, c1) and np.array_equal(v0, v1)
    assert rh.source_range() == (first, end), "back in global ids"
    windowed = rh.regrid_csr_rows(field[first:end].contiguous(), nlev=nlev)
    assert torch.equal(windowed.view(torch.int64), whole.view(torch.int64)), "the result bits are unchanged"
    late = R.regrid_store_conserve_mesh(src, dst, R.NORM_FRACAREA)       # a Store under the window is window-relative from the start
    assert late.n_src == end - first
    late.release()
    src.set_source_window(0, src_m.nCells)
    rh._refresh()
    assert rh.n_src == src_m.nCells and np.array_equal(rh.csr()[1], c0)
    rh.release()
    src.destroy()
    dst.destroy()


def test_refusals(dev, gpu_lib):
    from mpassit_amd import _lib as L, regrid as R, synth, target_grid as tg
    lib = L.load()

    def refused(rc, want, word=None):
        msg = lib.mpg_last_error().decode()
        assert rc == want and msg, (rc, want, msg)
        if word:
            assert word in msg, msg

    h = C.c_void_p()
    a, b = dev("geo8"), dev("geo10")
    refused(L.regrid_store_conserve_mesh(None, b._h, 0, C.byref(h)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(L.regrid_store_conserve_mesh(a._h, None, 0, C.byref(h)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(L.regrid_store_conserve_mesh(a._h, b._h, 0, None), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(L.regrid_store_conserve_mesh(a._h, b._h, 2, C.byref(h)), L.MPG_ERR_INVALID_ARG, "norm_type")
    refused(L.regrid_store_conserve_mesh(a._h, b._h, -1, C.byref(h)), L.MPG_ERR_INVALID_ARG, "norm_type")
    # either mesh cut to a grid's window
    g = tg.define_target_grid_params("lambert", 61, 41, dx=30000.0, dy=30000.0, **MC.LAMBERT)
    grid = R.Grid.from_proj(g, fill_target=False)
    wmesh = R.Mesh.from_mpas(MC.mesh("hex_small"), window_grid=grid)
    refused(L.regrid_store_conserve_mesh(wmesh._h, b._h, 0, C.byref(h)), L.MPG_ERR_UNSUPPORTED, "source mesh was cut")
    refused(L.regrid_store_conserve_mesh(a._h, wmesh._h, 0, C.byref(h)), L.MPG_ERR_UNSUPPORTED, "destination mesh was cut")
    assert "mpg_mesh_create" in lib.mpg_last_error().decode()
    wmesh.destroy()
    grid.destroy()
    # verticesOnCell wider than 12, on either side
    m = MC.mesh("geo8")
    voc13 = np.zeros((m.nCells, 13), m.verticesOnCell.dtype)
    voc13[:, :m.verticesOnCell.shape[1]] = m.verticesOnCell
    wide = R.Mesh.from_mpas(synth.MpasMesh(m.latCell, m.lonCell, m.latVertex, m.lonVertex, voc13))
    refused(L.regrid_store_conserve_mesh(wide._h, b._h, 0, C.byref(h)), L.MPG_ERR_UNSUPPORTED, "maxEdges 13 > 12")
    refused(L.regrid_store_conserve_mesh(a._h, wide._h, 0, C.byref(h)), L.MPG_ERR_UNSUPPORTED, "maxEdges 13 > 12")
    wide.destroy()
    # a handle without a dst fraction says which Stores keep one
    bil = R.regrid_store_mesh(a, b)
    frac = np.zeros(bil.n_dst)
    refused(L.handle_get_dst_frac(bil._h, frac.ctypes.data), L.MPG_ERR_INVALID_ARG, "mpg_regrid_store_conserve_mesh")
    assert "mpg_regrid_store_conserve_to_mesh stores one" in lib.mpg_last_error().decode()
    bil.release()


def test_symmetric_pair_is_right_or_refused(gpu_lib, oracle):
    """Two geodesic meshes of different frequency share the icosahedron's mirror planes: source edges run through destination vertices,
    and the in-place clip step can then see a polygon cross a plane four times (measured on the CPU: 2 of the 3882 candidate pairs of
    geo8 -> geo10, one of them covering 0.90 of its destination cell).  It reports such a polygon instead of storing a wrong one: the
    Store either matches the reference or fails with MPG_ERR_OVERFLOW -- never a silently wrong matrix."""
    from mpassit_amd import _lib as L, regrid as R
    src_m, dst_m = MC.mesh("geo8"), MC.mesh("geo10")
    src, dst = R.Mesh.from_mpas(src_m), R.Mesh.from_mpas(dst_m)
    try:
        rh = R.regrid_store_conserve_mesh(src, dst)
    except L.MpgError as e:
        print("geo8 -> geo10: refused, %s" % e)
        assert e.rc == L.MPG_ERR_OVERFLOW and "vertex slots" in str(e)
    else:
        _check_store(rh, MR.Answer(oracle, src_m, dst_m), MR.NORM_DSTAREA, "geo8 -> geo10")
        rh.release()
    src.destroy()
    dst.destroy()


def test_the_old_entry_point_still_refuses_conserve(dev, gpu_lib):
    from mpassit_amd import _lib as L, regrid as R
    lib = L.load()
    h = C.c_void_p()
    rc = L.regrid_store_mesh(dev("geo8")._h, 0, dev("geo10")._h, 0, R.REGRIDMETHOD_CONSERVE, C.byref(h))
    msg = lib.mpg_last_error().decode()
    assert rc == L.MPG_ERR_UNSUPPORTED and "conservative" in msg and "Voronoi cell against Voronoi cell is not built" in msg
    assert "mpg_regrid_store_conserve_to_mesh" in msg and "mpg_regrid_store_conserve_mesh" in msg, "the message names both ways out"
    with pytest.raises(L.MpgError) as e:
        R.regrid_store_mesh(dev("geo8"), dev("geo10"), R.REGRIDMETHOD_CONSERVE)
    assert e.value.rc == L.MPG_ERR_UNSUPPORTED
