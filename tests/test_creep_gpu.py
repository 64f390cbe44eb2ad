"""Creep-fill extrapolation on the GPU at small sizes (mpg_handle_creep): BYTE FOR BYTE against the numpy mirror target_grid.creep_rows fed
with the input handle's own pattern (rh.csr() / fixed_to_csr(rh.weights())) and creep_neighbours_grid / _mesh -- rowptr, col, the bits of
val, the levels through the row lengths, and store_stats -- on every geometry pairing with 1, 2, 5 and all levels, at the smallest
shapes, on long rows, with dst_skip, twice for determinism, chained, under every consumer, composed with the nearest fill, and the
refusals.

k_creep.hip has ONE path for rows of any length (a stable device-wide sort of the candidates, one lane per (row, column) run) and no
blocking knob, so there is no second path and no knob setting for the long-row case to reach: it checks that rows of 1320 entries from
3960 candidates come out right on the path every row takes.

The constant-field bound is test_creep_ref.py's row-sum bound, (longest row + last level) * 2^-52, from store_stats [6] and [2]."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import _contract_ref as cr
from conftest import LAMBERT

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
PAIRINGS = ("m2g bilinear", "m2g nearest", "m2g conserve", "g2m cells", "m2m cells", "g2g e1", "g2g e2", "pole none")
KIND = {"m2g bilinear": 3, "m2g nearest": 1, "m2g conserve": 0, "g2m cells": 4, "m2m cells": 3, "g2g e1": 4, "g2g e2": 4, "pole none": 0}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return all(np.array_equal(_raw(x), _raw(y)) for x, y in zip(a, b))


def _rows_of(rh):
    """(rowptr, col, val) of any handle without pole terms; a fixed one's slots in slot order, -1 entries dropped, a row whose slot 0 is
    -1 empty (the unmapped rule), a nearest handle's weights 1.0"""
    from mpassit_amd import target_grid as tg
    if rh.nnz_per_row == 0:
        return rh.csr()
    idx, w = rh.weights()
    idx = np.where(idx[:, :1] < 0, -1, idx)
    return tg.fixed_to_csr(idx, None if rh.nnz_per_row == 1 else w)


def _grid_nb(rh):
    from mpassit_amd import target_grid as tg
    return tg.creep_neighbours_grid(rh.nx_dst, rh.ny_dst)


def _expect(rh, nb, num_levels, skip=None):
    from mpassit_amd import target_grid as tg
    return tg.creep_rows(*_rows_of(rh), nb, num_levels, skip)


def _check(out, rh, want, what):
    """`out` = creep(rh, ...) against the mirror's (level, rowptr, col, val): shape, kind, bytes and statistics"""
    level, wptr, wcol, wval = want
    assert (out.n_src, out.n_dst, out.nx_dst, out.ny_dst) == (rh.n_src, rh.n_dst, rh.nx_dst, rh.ny_dst), what
    assert out.nnz_per_row == 0 and out.nnz == wcol.size, (what, out.nnz_per_row, out.nnz, wcol.size)
    gptr, gcol, gval = out.csr()
    assert np.array_equal(gptr, wptr), (what, "rowptr")
    assert np.array_equal(np.diff(gptr) > 0, level >= 0), (what, "the levels through the row lengths")
    assert np.array_equal(gcol, wcol), (what, "col")
    assert np.array_equal(_bits(gval), _bits(wval)), (what, "val bits", int((_bits(gval) != _bits(wval)).sum()))
    stats = out.store_stats
    longest = int(np.diff(wptr).max()) if level.size else 0
    assert (stats[1], stats[2], stats[3], stats[6]) == (int((level > 0).sum()), int(max(level.max(), 0)) if level.size else 0, int((level < 0).sum()), longest), (what, stats)
    assert out.store_ms > 0.0


def _nearest_outside_unmapped(R, o):
    """The nearest Mesh -> Grid handle (1 slot, no weight array).  The nearest Store maps every grid point, those outside the mesh too, so
    the points the bilinear Store leaves unmapped are unmapped here by mpg_handle_mask with a destination mask: the documented order, mask
    first, then creep."""
    bil = R.regrid_store(o["mesh_in"], o["grid"], R.REGRIDMETHOD_BILINEAR)
    near = R.regrid_store(o["mesh_in"], o["grid"], R.REGRIDMETHOD_NEAREST_STOD)
    out = R.mask_handle(near, dst_mask=bil.weights()[0][:, 0] < 0)
    assert out.nnz_per_row == 1
    for h in (bil, near):
        h.release()
    return out


@pytest.fixture(scope="module")
def world(gpu_lib):
    from mpassit_amd import regrid as R, synth, target_grid as tg
    g = tg.define_target_grid_params("lambert", 61, 41, dx=30000.0, dy=30000.0, **LAMBERT)
    m_in = synth.regional_mesh_for_lambert(g.proj, 61, 41, 5003, margin=-0.08, seed=12)
    m_over = synth.mesh_edges(synth.regional_mesh_for_lambert(g.proj, 61, 41, 6001, margin=0.05, seed=11))
    m_vor = synth.global_voronoi_mesh(1500)
    gp = tg.define_target_grid_params("lat-lon", nx=25, ny=13, stand_lon=0.0, is_regional=False)
    o = dict(grid=R.Grid.from_target(g), mesh_in=R.Mesh.from_mpas(m_in), mesh_over=R.Mesh.from_mpas(m_over), per=R.Grid.from_target(gp),
             vor=R.Mesh.from_mpas(m_vor))
    assert (m_in.nCells, m_over.nCells) == (5084, 6030)
    E, C_, E1, E2 = R.MESHLOC_ELEMENT, R.STAGGERLOC_CENTER, R.STAGGERLOC_EDGE1, R.STAGGERLOC_EDGE2
    BIL, NEAR = R.REGRIDMETHOD_BILINEAR, R.REGRIDMETHOD_NEAREST_STOD
    nb_over = tg.creep_neighbours_mesh(m_over.verticesOnCell, o["mesh_over"].triangles())
    nb_vor = tg.creep_neighbours_mesh(m_vor.verticesOnCell, o["vor"].triangles())
    # name -> (handle, src, src_loc, dst, dst_loc, the destination's neighbour table or None = the grid stagger's)
    pairs = {
        "m2g bilinear": (R.regrid_store(o["mesh_in"], o["grid"], BIL), o["mesh_in"], E, o["grid"], C_, None),
        "m2g nearest": (_nearest_outside_unmapped(R, o), o["mesh_in"], E, o["grid"], C_, None),
        "m2g conserve": (R.regrid_store(o["mesh_in"], o["grid"], R.REGRIDMETHOD_CONSERVE), o["mesh_in"], E, o["grid"], C_, None),
        "g2m cells": (R.regrid_store_to_mesh(o["grid"], o["mesh_over"], BIL), o["grid"], C_, o["mesh_over"], E, nb_over),
        "m2m cells": (R.regrid_store_mesh(o["mesh_in"], o["mesh_over"], BIL), o["mesh_in"], E, o["mesh_over"], E, nb_over),
        "g2g e1": (R.regrid_store_grid(o["grid"], E1), o["grid"], C_, o["grid"], E1, None),
        "g2g e2": (R.regrid_store_grid(o["grid"], E2), o["grid"], C_, o["grid"], E2, None),
        "pole none": (R.regrid_store_periodic_to_mesh(o["per"], o["vor"], pole_method=R.POLEMETHOD_NONE), o["per"], C_, o["vor"], E, nb_vor),
    }
    d = dict(g=g, obj=o, pairs=pairs, syn=dict(mesh_in=m_in, mesh_over=m_over), want={}, crept={})
    yield d
    for h in list(d["crept"].values()) + [p[0] for p in pairs.values()]:
        h.release()
    for x in o.values():
        x.destroy()


def _nb_of(world, name):
    rh, _, _, _, _, nb = world["pairs"][name]
    return _grid_nb(rh) if nb is None else nb


def _want(world, name, num_levels):
    """the mirror's answer for a pairing, computed once"""
    key = (name, num_levels)
    if key not in world["want"]:
        world["want"][key] = _expect(world["pairs"][name][0], _nb_of(world, name), num_levels)
    return world["want"][key]


def _crept(world, name, num_levels):
    from mpassit_amd import regrid as R
    key = (name, num_levels)
    if key not in world["crept"]:
        rh, _, _, dst, dloc, _ = world["pairs"][name]
        world["crept"][key] = R.creep(rh, dst, num_levels, dst_loc=dloc)
    return world["crept"][key]


# ---- 1. the pairings ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PAIRINGS)
def test_pairings(world, name):
    from mpassit_amd import regrid as R
    rh, _, _, dst, dloc, _ = world["pairs"][name]
    unmapped = np.diff(_rows_of(rh)[0]) == 0
    assert rh.nnz_per_row == KIND[name] and 0 < unmapped.sum() < rh.n_dst / 2, (name, rh.nnz_per_row, int(unmapped.sum()), rh.n_dst)
    for num_levels in (1, 2, 5, R.CREEP_ALL_LEVELS):
        want = _want(world, name, num_levels)
        out = _crept(world, name, num_levels)
        _check(out, rh, want, (name, num_levels))
        st = out.store_stats
        print("%s, %s levels: %d of %d rows unmapped, %d filled, last level %d, %d left, longest row %d, %d entries"
              % (name, "all" if num_levels == R.CREEP_ALL_LEVELS else num_levels, unmapped.sum(), rh.n_dst, st[1], st[2], st[3], st[6], out.nnz))
        assert st[1] > 0 and st[1] + st[3] == unmapped.sum()
    # determinism: a second call, the same bytes
    again = R.creep(rh, dst, R.CREEP_ALL_LEVELS, dst_loc=dloc)
    assert _same(again.csr(), _crept(world, name, R.CREEP_ALL_LEVELS).csr()), (name, "two calls")
    again.release()
    # a capped fill is a prefix of the full one: levels 1 and 2 are the same rows in every call
    l2, full = _want(world, name, 2), _want(world, name, R.CREEP_ALL_LEVELS)
    assert np.array_equal(np.where(full[0] <= 2, full[0], -1), l2[0])


# ---- 2. the smallest shapes ---------------------------------------------------------------------------------------------------------------
def _grid(R, nx, ny):
    lon, lat = np.meshgrid(-100.0 + 0.25 * np.arange(nx), 35.0 + 0.2 * np.arange(ny))
    return R.Grid(lon, lat)


def _weights_handle(R, rng, n_src, nx, ny, mapped, lens=(1, 4), distinct=False):
    """a from_weights handle of nx x ny rows: the rows `mapped` hold lens[0] .. lens[1] - 1 random entries, every other row none"""
    n = nx * ny
    k = np.zeros(n, np.int64)
    k[list(mapped)] = rng.integers(lens[0], lens[1], len(list(mapped)))
    row = np.repeat(np.arange(1, n + 1, dtype=np.int32), k)
    if distinct:
        col = np.concatenate([rng.choice(n_src, int(c), replace=False) for c in k if c] or [np.empty(0, np.int64)]).astype(np.int32) + 1
    else:
        col = rng.integers(1, n_src + 1, row.size).astype(np.int32)
    return R.RouteHandle.from_weights(n_src, nx, ny, row, col, rng.uniform(0.1, 1.0, row.size))


def _grid_case(R, nx, ny, mapped, num_levels, skip=None, seed=0, lens=(1, 4), n_src=50, distinct=False):
    """creep on a bare nx x ny grid from a from-weights handle against the mirror -> (level, the mirror's CSR, store_stats)"""
    rng = np.random.default_rng(seed)
    grid = _grid(R, nx, ny)
    rh = _weights_handle(R, rng, n_src, nx, ny, mapped, lens, distinct)
    try:
        want = _expect(rh, _grid_nb(rh), num_levels, skip)
        out = R.creep(rh, grid, num_levels, dst_skip=skip)
        _check(out, rh, want, (nx, ny, num_levels))
        stats = out.store_stats
        out.release()
    finally:
        rh.release()
        grid.destroy()
    return want[0], want[1:], stats


@pytest.mark.parametrize("shape", [(1, 1), (1, 63), (1, 64), (1, 65), (63, 1), (257, 1), (2, 2), (3, 3), (9, 7)])
def test_small_grids(gpu_lib, shape):
    """one point mapped and unmapped; strips that bracket a 64-lane wave and a 256-thread block with one end mapped; 2 x 2; 3 x 3 from its
    centre; 9 x 7 from a corner with all levels: the Chebyshev distances, 8 of them; rows of 1 to 3 entries as _weights_handle makes them"""
    from mpassit_amd import regrid as R
    nx, ny = shape
    n = nx * ny
    ALL = R.CREEP_ALL_LEVELS
    if shape == (1, 1):
        level, _, stats = _grid_case(R, 1, 1, [0], ALL)
        assert level.tolist() == [0] and stats[1:4] == [0, 0, 0]
        level, (ptr, _, _), stats = _grid_case(R, 1, 1, [], ALL)
        assert level.tolist() == [-1] and ptr.tolist() == [0, 0] and stats[1:4] == [0, 0, 1]
        return
    if shape == (2, 2):
        for p in range(4):
            level, _, stats = _grid_case(R, 2, 2, [p], ALL, seed=p)
            assert level.tolist() == [int(q != p) for q in range(4)] and stats[1:4] == [3, 1, 0]
        level, _, stats = _grid_case(R, 2, 2, [0, 3], ALL, seed=4)
        assert level.tolist() == [0, 1, 1, 0] and stats[1:4] == [2, 1, 0], "m = 2: the half-sum of two different rows"
        return
    if shape == (3, 3):
        level, _, stats = _grid_case(R, 3, 3, [4], ALL)
        assert level.tolist() == [1, 1, 1, 1, 0, 1, 1, 1, 1] and stats[1:4] == [8, 1, 0]
        return
    if shape == (9, 7):
        level, _, stats = _grid_case(R, 9, 7, [0], ALL)
        j, i = np.divmod(np.arange(63), 9)
        assert np.array_equal(level, np.maximum(i, j)) and stats[1:4] == [62, 8, 0]
        level, _, stats = _grid_case(R, 9, 7, [0], 3)
        assert stats[1:4] == [15, 3, 47]
        return
    for mapped, seed in (([0], 1), ([n - 1], 2), ([0, n - 1], 3)):
        level, (ptr, col, val), stats = _grid_case(R, nx, ny, mapped, ALL, seed=seed)
        pos = np.arange(n)
        assert np.array_equal(level, np.min([np.abs(pos - m) for m in mapped], axis=0)) and stats[1] == n - len(mapped) and stats[3] == 0
    level, _, stats = _grid_case(R, nx, ny, [0], 5, seed=4)
    assert stats[1:4] == [min(5, n - 1), min(5, n - 1), max(n - 6, 0)]
    level, _, stats = _grid_case(R, nx, ny, [], ALL)
    assert stats[1:4] == [0, 0, n], "everything unmapped: nothing to creep from"
    level, _, stats = _grid_case(R, nx, ny, range(n), 2)
    assert stats[1:4] == [0, 0, 0], "nothing unmapped: a copy of the pattern"


def test_bare_mesh_has_no_neighbours(gpu_lib):
    from mpassit_amd import regrid as R, target_grid as tg
    rng = np.random.default_rng(5)
    n = 70
    mesh = R.Mesh(np.deg2rad(30.0 + rng.uniform(0, 10, n)), np.deg2rad(-100.0 + rng.uniform(0, 10, n)), np.zeros(3), np.array([0.0, 0.1, 0.2]),
                  np.zeros((n, 3), np.int32))
    rh = _weights_handle(R, rng, 20, n, 1, range(0, n, 2))
    out = R.creep(rh, mesh, R.CREEP_ALL_LEVELS)
    want = tg.creep_rows(*_rows_of(rh), tg.creep_neighbours_mesh(np.zeros((n, 3), np.int32), mesh.triangles()))
    _check(out, rh, want, "bare centres")
    assert out.store_stats[1:4] == [0, 0, n // 2], "nothing is filled, and that is success"
    for x in (out, rh):
        x.release()
    mesh.destroy()


# ---- 3. long rows -------------------------------------------------------------------------------------------------------------------------
def test_long_rows(gpu_lib):
    """33 x 33, column 0 mapped by rows of 40 distinct columns each, all levels: the rows reach 33 * 40 = 1320 entries from 3 * 1320
    candidates (one path for every length: see the module's text)"""
    from mpassit_amd import regrid as R
    nx = ny = 33
    rng = np.random.default_rng(33)
    perm = rng.permutation(nx * 40)
    row = np.repeat(np.arange(ny, dtype=np.int32) * nx + 1, 40)
    col = (perm + 1).astype(np.int32)                              # row j holds columns perm[40 j .. 40 j + 40): all 1320 distinct, unsorted
    grid = _grid(R, nx, ny)
    rh = R.RouteHandle.from_weights(nx * 40, nx, ny, row, col, rng.uniform(0.1, 1.0, row.size))
    want = _expect(rh, _grid_nb(rh), R.CREEP_ALL_LEVELS)
    out = R.creep(rh, grid, R.CREEP_ALL_LEVELS)
    _check(out, rh, want, "long rows")
    stats = out.store_stats
    assert stats[1:4] == [nx * ny - ny, nx - 1, 0] and stats[6] == 1320
    lens = np.diff(want[1]).reshape(ny, nx)
    assert lens[16, 32] == 1320 and lens[0, 1] == 80 and lens[16, 1] == 120
    for x in (out, rh):
        x.release()
    grid.destroy()


# ---- 4. dst_skip, determinism, the chain identity -------------------------------------------------------------------------------------------
def test_dst_skip(world):
    from mpassit_amd import regrid as R
    nx, ny = 7, 5
    j, i = np.divmod(np.arange(nx * ny), nx)
    wall = i == 3
    level, _, stats = _grid_case(R, nx, ny, [jj * nx for jj in range(ny)], R.CREEP_ALL_LEVELS, skip=wall.astype(np.uint8), seed=7)
    assert np.array_equal(level, np.where(i < 3, i, -1)) and stats[1:4] == [10, 2, 20], "a wall stops the front"
    gap = wall & (j != 2)
    level, _, stats = _grid_case(R, nx, ny, [jj * nx for jj in range(ny)], R.CREEP_ALL_LEVELS, skip=gap, seed=7)
    assert level.max() == 6 and stats[1:4] == [26, 6, 4], "through the gap"
    # scattered bytes on a real pairing, any non-zero byte counts; a mapped row that is skipped keeps its row
    rh, _, _, dst, dloc, _ = world["pairs"]["m2g bilinear"]
    rng = np.random.default_rng(8)
    skip = (rng.uniform(size=rh.n_dst) < 0.2).astype(np.uint8) * rng.integers(1, 256, rh.n_dst).astype(np.uint8)
    want = _expect(rh, _grid_nb(rh), R.CREEP_ALL_LEVELS, skip)
    out = R.creep(rh, dst, R.CREEP_ALL_LEVELS, dst_skip=skip, dst_loc=dloc)
    _check(out, rh, want, "scattered skip")
    unmapped = np.diff(_rows_of(rh)[0]) == 0
    assert ((want[0] < 0) & ~unmapped).sum() == 0 and (want[0] < 0).sum() >= (unmapped & (skip != 0)).sum() > 0
    out.release()
    # both spellings of "no skip"
    none = R.creep(rh, dst, 2, dst_skip=None, dst_loc=dloc)
    zeros = R.creep(rh, dst, 2, dst_skip=np.zeros(rh.n_dst, bool), dst_loc=dloc)
    assert _same(none.csr(), zeros.csr()) and _same(none.csr(), _crept(world, "m2g bilinear", 2).csr())
    for x in (none, zeros):
        x.release()


@pytest.mark.parametrize("name", ["m2g bilinear", "m2g conserve", "g2m cells"])
def test_chain_identity(world, name):
    """creep(creep(h, 2), 3) has the bytes of creep(h, 5): on a fixed input (the first step turns it into CSR), a CSR one and a mesh"""
    from mpassit_amd import regrid as R
    rh, _, _, dst, dloc, _ = world["pairs"][name]
    two = _crept(world, name, 2)
    five = R.creep(two, dst, 3, dst_loc=dloc)
    assert _same(five.csr(), _crept(world, name, 5).csr()), name
    st2, st5 = two.store_stats, _crept(world, name, 5).store_stats
    assert five.store_stats[1] == st5[1] - st2[1] and five.store_stats[3] == st5[3]
    five.release()


# ---- 5. consumers ---------------------------------------------------------------------------------------------------------------------------
def _held(got, want, what):
    import torch
    g, w = got.contiguous().reshape(-1), want.contiguous().reshape(-1)
    assert g.dtype == w.dtype and g.numel() == w.numel(), (what, g.dtype, w.dtype)
    it = torch.int64 if g.dtype == torch.float64 else torch.int32
    bad = g.view(it) != w.view(it)
    assert not bool(bad.any()), (what, int(bad.sum()), bad.numel())


def _twin(R, rh, want):
    """RouteHandle.from_weights of the mirror's CSR"""
    _, ptr, col, val = want
    row = np.repeat(np.arange(1, rh.n_dst + 1, dtype=np.int32), np.diff(ptr))
    twin = R.RouteHandle.from_weights(rh.n_src, rh.nx_dst, rh.ny_dst, row, (col + 1).astype(np.int32), val)
    assert twin.nnz_per_row == 0
    return twin


def test_consumers(world, gpu_lib):
    """A crept handle under regrid_typed, regrid_masked with nothing missing, regrid_transpose, regrid_csr_to_mesh and regrid_csr_rows:
    bit for bit the same call on from_weights of the mirror's CSR; a constant field comes back constant at the filled points"""
    import torch
    from mpassit_amd import regrid as R
    nlev, nf = 5, 2
    rh = _crept(world, "m2g bilinear", 5)
    want = _want(world, "m2g bilinear", 5)
    twin = _twin(R, rh, want)
    for dt in (torch.float64, torch.float32):
        x = torch.from_numpy(cr.ordinary(rh.n_src, nlev, nf, 5)).cuda().to(dt)
        for layout, s in ((R.LAYOUT_CELL_FAST, x), (R.LAYOUT_LEV_FAST, x.transpose(1, 2).contiguous())):
            for odt in (torch.float64, torch.float32):
                _held(rh.regrid_typed(s.view(-1), nlev=nlev, nfields=nf, layout=layout, out_dtype=odt),
                      twin.regrid_typed(s.view(-1), nlev=nlev, nfields=nf, layout=layout, out_dtype=odt), ("typed", dt, layout, odt))
        _held(rh.regrid_masked(x.view(-1), nlev=nlev, nfields=nf), twin.regrid_masked(x.view(-1), nlev=nlev, nfields=nf), ("masked", dt))
        g = torch.from_numpy(cr.ordinary(rh.n_dst, nlev, nf, 9)).cuda().to(dt)
        _held(rh.regrid_transpose(g, nlev=nlev, nfields=nf, out_dtype=torch.float64), twin.regrid_transpose(g, nlev=nlev, nfields=nf, out_dtype=torch.float64),
              ("transpose", dt))
    # a constant field: the mapped bilinear rows give 1 within their own 3 roundings, the filled rows within the row-sum bound
    st = rh.store_stats
    one = rh.regrid_typed(torch.ones(rh.n_src, dtype=torch.float64, device="cuda")).reshape(-1).cpu().numpy()
    filled = want[0] > 0
    err = np.abs(one[filled] - 1.0).max()
    print("constant field: worst |y - 1| at %d filled points %.3g eps, bound (%d + %d) eps" % (filled.sum(), err / EPS, st[6], st[2]))
    assert filled.sum() == st[1] and err <= (st[6] + st[2]) * EPS
    assert (one[want[0] < 0] == 0.0).all() and (want[0] < 0).sum() == st[3]
    twin.release()
    # mesh-order consumers: grid planes onto the cells of a mesh, and MPAS rows onto MPAS rows
    rh = _crept(world, "g2m cells", R.CREEP_ALL_LEVELS)
    twin = _twin(R, rh, _want(world, "g2m cells", R.CREEP_ALL_LEVELS))
    x = torch.from_numpy(cr.ordinary(rh.n_src, nlev, nf, 6)).cuda()
    for layout in (R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST):
        _held(rh.regrid_csr_to_mesh(x, nlev=nlev, nfields=nf, layout=layout), twin.regrid_csr_to_mesh(x, nlev=nlev, nfields=nf, layout=layout),
              ("csr_to_mesh", layout))
    twin.release()
    rh = _crept(world, "m2m cells", 2)
    twin = _twin(R, rh, _want(world, "m2m cells", 2))
    x = torch.from_numpy(cr.ordinary(rh.n_src, nlev, nf, 7)).cuda().transpose(1, 2).contiguous()      # nfields slabs of (n_src, nlev)
    _held(rh.regrid_csr_rows(x, nlev=nlev, nfields=nf), twin.regrid_csr_rows(x, nlev=nlev, nfields=nf), "csr_rows")
    twin.release()


# ---- 6. creep, then the nearest source for what is left (ESMF_EXTRAPMETHOD_CREEP_NRST_D) ----------------------------------------------------
@pytest.mark.parametrize("name", ["m2g bilinear", "g2m cells"])
def test_creep_nearest(world, name):
    from mpassit_amd import regrid as R, target_grid as tg
    rh, src, sloc, dst, dloc, _ = world["pairs"][name]
    sx, dx = src.xyz(sloc), dst.xyz(dloc)

    def expected(want, rows, ids):
        """the crept CSR with row rows[u] = one entry (ids[u], 1.0) where ids[u] >= 0"""
        level, ptr, col, val = want
        lens = np.diff(ptr).copy()
        lens[rows[ids >= 0]] = 1
        optr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        ocol, oval = np.empty(optr[-1], np.int32), np.empty(optr[-1])
        keep = np.repeat(np.diff(ptr) > 0, lens)
        ocol[keep], oval[keep] = col, val
        ocol[optr[rows[ids >= 0]]], oval[optr[rows[ids >= 0]]] = ids[ids >= 0], 1.0
        return optr, ocol, oval

    # no masks
    want = _want(world, name, 2)
    left = np.flatnonzero(want[0] < 0)
    assert left.size > 0, "two levels leave rows for the nearest fill"
    _, ids, _ = tg.extrapolate_rows(sx, dx, left, tg.EXTRAPMETHOD_NEAREST_STOD)
    out = R.creep_nearest(rh, src, dst, 2, src_loc=sloc, dst_loc=dloc)
    assert _same(out.csr(), expected(want, left, ids[:, 0])), name
    assert (np.diff(out.csr()[0]) > 0).all(), "no row is left unmapped"
    out.release()
    # a source mask and skipped destinations: the nearest UNMASKED source, the skipped rows left alone by both steps
    rng = np.random.default_rng(11)
    smask = rng.uniform(size=rh.n_src) < 0.3
    skip = rng.uniform(size=rh.n_dst) < 0.1
    want = _expect(rh, _nb_of(world, name), 2, skip)
    left = np.flatnonzero((want[0] < 0) & ~skip)
    _, ids, _ = tg.extrapolate_rows_masked(sx, dx, left, smask, tg.EXTRAPMETHOD_NEAREST_STOD)
    out = R.creep_nearest(rh, src, dst, 2, src_mask=smask, dst_skip=skip, src_loc=sloc, dst_loc=dloc)
    assert _same(out.csr(), expected(want, left, ids[:, 0])), (name, "masked")
    unmapped = np.diff(_rows_of(rh)[0]) == 0
    assert np.array_equal(np.diff(out.csr()[0]) == 0, unmapped & skip) and (unmapped & skip).sum() > 0
    out.release()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(world, gpu_lib):
    from mpassit_amd import _lib as L, regrid as R, synth, target_grid as tg
    lib = L.load()
    o = world["obj"]
    m2g = world["pairs"]["m2g bilinear"][0]
    who = "mpg_handle_creep"
    h = C.c_void_p()

    def pts(obj, loc=0):
        return R._points(obj, loc, "x")

    def call(rh=m2g, dst=None, levels=3, out=h, skip=None):
        pd = pts(o["grid"]) if dst is None else dst
        opts = L.CreepOpts(num_levels=levels, dst_skip_dev=skip)
        return L.handle_creep(rh._h if rh is not None else None, C.byref(pd), C.byref(opts), C.byref(out) if out is not None else None)

    def refused(rc, want, *words):
        msg = lib.mpg_last_error().decode()
        assert rc == want and who in msg, (rc, want, msg)
        for word in words:
            assert word in msg, msg

    INV, UNS = L.MPG_ERR_INVALID_ARG, L.MPG_ERR_UNSUPPORTED
    assert call() == 0
    L.check(lib.mpg_handle_release(h))
    h = C.c_void_p()
    refused(call(rh=None), INV, "NULL")
    refused(call(out=None), INV, "NULL")
    opts = L.CreepOpts(num_levels=1, dst_skip_dev=None)
    pd = pts(o["grid"])
    refused(L.handle_creep(m2g._h, None, C.byref(opts), C.byref(h)), INV, "NULL")
    refused(L.handle_creep(m2g._h, C.byref(pd), None, C.byref(h)), INV, "NULL")
    refused(call(dst=L.Points(mesh=o["mesh_in"]._h, meshloc=0, grid=o["grid"]._h, staggerloc=0)), INV, "exactly one", "both")
    refused(call(dst=L.Points(mesh=None, meshloc=0, grid=None, staggerloc=0)), INV, "exactly one", "neither")
    refused(call(dst=pts(o["grid"], 7)), INV, "stagger location 7")
    refused(call(dst=pts(o["mesh_over"], 9)), INV, "mesh location 9")
    refused(call(levels=0), INV, "num_levels = 0", ">= 1", "MPG_CREEP_ALL_LEVELS")
    refused(call(levels=-3), INV, "num_levels = -3")
    refused(call(dst=pts(o["grid"], R.STAGGERLOC_EDGE1)), INV, "n_dst = 2400", "2440", "60 x 40", "61 x 40")
    refused(call(dst=pts(o["mesh_over"])), INV, "n_dst = 2400", "6030")
    bare = R.Grid(np.array([[0.0, 1.0]]), np.array([[0.0, 0.0]]))
    refused(call(dst=pts(bare, R.STAGGERLOC_EDGE1)), INV, "no coordinates")
    bare.destroy()
    # vertices and edges: no ring is defined there
    g2m = world["pairs"]["g2m cells"][0]
    refused(call(rh=g2m, dst=pts(o["mesh_over"], R.MESHLOC_NODE)), UNS, "MPG_MESHLOC_ELEMENT", "mpg_handle_extrapolate")
    refused(call(rh=g2m, dst=pts(o["mesh_over"], R.MESHLOC_EDGE)), UNS, "MPG_MESHLOC_ELEMENT")
    # a mesh cut to a grid, maxEdges > 12
    rng = np.random.default_rng(13)
    m_over = world["syn"]["mesh_over"]
    onto_over = _weights_handle(R, rng, 20, m_over.nCells, 1, range(0, m_over.nCells, 3))
    cut = R.Mesh.from_mpas(m_over, window_grid=o["grid"])
    refused(call(rh=onto_over, dst=pts(cut)), UNS, "mpg_mesh_create_window", "whole mesh")
    cut.destroy()
    wide = R.Mesh.from_mpas(dataclasses.replace(m_over, verticesOnCell=np.pad(m_over.verticesOnCell, ((0, 0), (0, 13 - m_over.verticesOnCell.shape[1])))))
    refused(call(rh=onto_over, dst=pts(wide)), UNS, "maxEdges 13 > 12")
    wide.destroy()
    assert call(rh=onto_over, dst=pts(o["mesh_over"])) == 0, "the same handle onto the whole mesh"
    L.check(lib.mpg_handle_release(h))
    h = C.c_void_p()
    # a periodic destination, pole terms
    onto_per = _weights_handle(R, rng, 20, 25, 13, range(0, 325, 2))
    refused(call(rh=onto_per, dst=pts(o["per"])), UNS, "MPG_GRID_PERIODIC_I", "seam")
    pole = R.regrid_store_grid(o["per"], R.STAGGERLOC_EDGE2)
    assert pole.pole()[0].size > 0
    refused(call(rh=pole, dst=pts(o["per"], R.STAGGERLOC_EDGE2)), UNS, "mpg_handle_pole_count > 0", "MPG_POLEMETHOD_NONE")
    # a localized handle, a source window
    rowptr, col, val = _rows_of(m2g)
    loc = R.RouteHandle.from_weights(m2g.n_src, m2g.nx_dst, m2g.ny_dst, np.repeat(np.arange(1, m2g.n_dst + 1, dtype=np.int32), np.diff(rowptr)),
                                     (col + 1).astype(np.int32), val)
    loc.localize()
    refused(call(rh=loc), UNS, "localized or rebased")
    g2 = tg.define_target_grid_params("lambert", 41, 31, dx=30000.0, dy=30000.0, **LAMBERT)
    m2 = R.Mesh.from_mpas(synth.regional_mesh_for_lambert(g2.proj, 41, 31, 3001, margin=0.3, seed=3))
    grid2 = R.Grid.from_target(g2)
    win = R.regrid_store(m2, grid2, R.REGRIDMETHOD_BILINEAR)
    first, end = win.source_range()
    assert 0 < first < end <= m2.nCells
    assert call(rh=win, dst=pts(grid2)) == 0, "the same call without a window"
    L.check(lib.mpg_handle_release(h))
    h = C.c_void_p()
    m2.set_source_window(first, end - first)
    refused(call(rh=win, dst=pts(grid2)), UNS, "source window", "mpg_mesh_set_source_window")
    m2.set_source_window(0, m2.nCells)
    assert h.value is None, "a refused call leaves *out alone"
    # the wrappers' own checks, and the library still works afterwards
    with pytest.raises(ValueError):
        R.creep(m2g, "grid")
    with pytest.raises(ValueError):
        R.creep(m2g, o["grid"], dst_skip=np.zeros(5, bool))
    again = R.creep(m2g, o["grid"], 2)
    assert _same(again.csr(), _crept(world, "m2g bilinear", 2).csr())
    for x in (again, onto_over, onto_per, pole, loc, win):
        x.release()
    m2.destroy()
    grid2.destroy()
