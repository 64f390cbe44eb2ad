"""The float64 device entry point (mpg_regrid_pitched_dev: Handle.regrid on float64 CUDA tensors) against the typed one
(mpg_regrid_typed_pitched_dev, float64 both sides, scale 1, offset 0), and the bits that only the float64 entry promises: it
stores the result as it stands, without the affine epilogue -- a nearest-neighbour Regrid is a copy of every bit pattern, and a
3-point sum that comes out as -0.0 stays -0.0 (fma(x, 1, 0) would make it +0.0).  Every input is a CUDA tensor, so no call goes
through the host pipeline, and every comparison is on int64 views: -0.0 == 0.0 and nan != nan say nothing about bits.

Shapes: a mesh with an unmapped rim, the tiny workload, and that mesh under a 19 x 11 grid (narrower than a tile); 1, 2, 9 and
65 levels (one level: the cell-fast kernels serve both layouts; 2: the shortest row the row gather takes; 9: an odd count at
or above the staging threshold of 8; 65: a second 64-level chunk), two fields.

The sign-of-zero test prints, per case, how many mapped points carry three non-negative weights (at least 99 % must)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NLEVS = (1, 2, 9, 65)
NF = 2
A3 = (-1, -2, 0, 1, 2)           # "a3_staged": per handle, lane gather, the three staged shapes
LFV = (-1, 0, 1, 2)              # "lf_variant": per handle, row gather, staged level-fast, grid-row tiles
NEG_ZERO = -2 ** 63              # the bits of -0.0 as int64
CASES = ("regional", "tiny", "narrow")


def _bits(torch, t):
    return t.view(torch.int64)


def _layouts(R, cf):
    """(layout, source) for a [nfields][nlev][n_src] tensor: as it is, and in file order [nfields][n_src][nlev]"""
    return ((R.LAYOUT_CELL_FAST, cf), (R.LAYOUT_LEV_FAST, cf.transpose(1, 2).contiguous()))


_random = {}


def _random_sources(torch, R, n_src, nlev):
    """normal data shifted away from zero: fma(x, 1, 0) == x for every non-zero finite x"""
    if (n_src, nlev) not in _random:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(1000 * nlev + 7)
        _random[n_src, nlev] = _layouts(R, torch.randn((NF, nlev, n_src), dtype=torch.float64, device="cuda", generator=gen) * 30 + 280)
    return _random[n_src, nlev]


@pytest.fixture(scope="module")
def cases(gpu_lib, regional_case):
    from mpassit_amd import regrid as R, target_grid as T, workloads
    mt, gt, _, _ = workloads.workload("tiny")
    gn = T.define_target_grid_params("lambert", 19, 11, dx=300000.0, dy=300000.0, ref_lat=38.5, ref_lon=-97.5, truelat1=38.5,
                                     truelat2=38.5, stand_lon=-97.5)
    out = {}
    for name, (m, g) in (("regional", regional_case), ("tiny", (mt, gt)), ("narrow", (mt, gn))):
        mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
        out[name] = dict(mesh=mesh, grid=grid,
                         bilinear=R.regrid_store(mesh, grid, R.REGRIDMETHOD_BILINEAR),
                         nearest=R.regrid_store(mesh, grid, R.REGRIDMETHOD_NEAREST_STOD),
                         conserve=R.regrid_store(mesh, grid, R.REGRIDMETHOD_CONSERVE))
    yield out
    _random.clear()
    for c in out.values():
        for k in ("bilinear", "nearest", "conserve"):
            c[k].release()
        c["mesh"].destroy()
        c["grid"].destroy()


def _entries_agree(torch, R, gpu_lib, rh, what):
    def typed(src, nlev, layout, out=None):
        return rh.regrid_typed(src.view(-1), nlev=nlev, nfields=NF, layout=layout, out_dtype=torch.float64, scale=1.0, offset=0.0, out=out)
    try:
        for a3 in A3:
            gpu_lib.tune("a3_staged", a3)
            for lfv in LFV:
                gpu_lib.tune("lf_variant", lfv)
                for nlev in NLEVS:
                    for layout, src in _random_sources(torch, R, rh.n_src, nlev):
                        a = rh.regrid(src.view(-1), nlev=nlev, nfields=NF, layout=layout)
                        b = typed(src, nlev, layout)
                        assert torch.equal(_bits(torch, a), _bits(torch, b)), (what, a3, lfv, nlev, layout)
                        assert bool((_bits(torch, a) != 0).any()), (what, "an all-zero result shows nothing")
    finally:
        gpu_lib.tune("a3_staged", -1)
        gpu_lib.tune("lf_variant", -1)
    # a pitched destination (planes level_stride apart): both entries again, and the dense result's bits in every plane
    nlev = 9
    for layout, src in _random_sources(torch, R, rh.n_src, nlev):
        dense = rh.regrid(src.view(-1), nlev=nlev, nfields=NF, layout=layout)
        a, b = rh.empty_pitched(nlev, NF, torch.float64), rh.empty_pitched(nlev, NF, torch.float64)
        assert a.stride(1) == rh.level_stride(torch.float64)
        rh.regrid(src.view(-1), nlev=nlev, nfields=NF, layout=layout, out=a)
        typed(src, nlev, layout, out=b)
        assert torch.equal(_bits(torch, a), _bits(torch, dense)) and torch.equal(_bits(torch, b), _bits(torch, dense)), (what, "pitched", layout)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("method", ["bilinear", "nearest", "conserve"])
def test_entry_points_agree_mesh_to_grid(gpu_lib, cases, case, method):
    import torch
    from mpassit_amd import regrid as R
    _entries_agree(torch, R, gpu_lib, cases[case][method], (case, method))


def test_entry_points_agree_destagger_and_csr(gpu_lib, cases, regional_case):
    """CENTER -> EDGE1 on a regional grid and on a periodic lat-lon grid (pole caps: EDGE1 carries the cap list, EDGE2 the cap
    weights), and the conservative weights of the regional case brought back through from_weights as a CSR handle."""
    import torch
    from mpassit_amd import regrid as R, target_grid as T
    gl = R.Grid.from_target(T.define_target_grid_params("lat-lon", nx=73, ny=37, stand_lon=0.0, is_regional=False))
    m, g = regional_case
    row, col, S = cases["regional"]["conserve"].to_esmf_weights()
    order = np.argsort(row, kind="stable")
    handles = [("regional EDGE1", R.regrid_store_grid(cases["regional"]["grid"], R.STAGGERLOC_EDGE1)),
               ("periodic EDGE1", R.regrid_store_grid(gl, R.STAGGERLOC_EDGE1)),
               ("periodic EDGE2", R.regrid_store_grid(gl, R.STAGGERLOC_EDGE2)),
               ("from_weights CSR", R.RouteHandle.from_weights(m.nCells, g.nx, g.ny, row[order], col[order], S[order]))]
    assert handles[0][1].nnz_per_row == 4 and len(handles[1][1].pole()[0]) > 0 and handles[3][1].nnz_per_row == 0
    for what, rh in handles:
        _entries_agree(torch, R, gpu_lib, rh, what)
        rh.release()
    gl.destroy()


@pytest.mark.parametrize("case", CASES)
def test_nearest_is_a_copy_of_every_bit_pattern(gpu_lib, cases, case):
    import torch
    from mpassit_amd import regrid as R
    rh = cases[case]["nearest"]
    idx = torch.as_tensor(rh.weights()[0][:, 0].astype(np.int64), device="cuda")
    mapped = idx >= 0
    assert bool(mapped.any())
    for nlev in NLEVS:
        n = NF * nlev * rh.n_src
        i = torch.arange(n, dtype=torch.int64, device="cuda")
        bits = 0x7ff8000000000000 | (i + 1)                                     # quiet NaNs, every payload different
        bits = torch.where(i % 4 == 1, torch.full_like(i, NEG_ZERO), bits)                       # -0.0
        bits = torch.where(i % 4 == 2, torch.full_like(i, 0x7ff0000000000000), bits)             # +inf
        bits = torch.where(i % 4 == 3, torch.full_like(i, 0x7ff0000000000000 + NEG_ZERO), bits)  # -inf
        cf = bits.view(NF, nlev, rh.n_src)
        want = torch.where(mapped, cf[:, :, idx.clamp(min=0)], torch.zeros((), dtype=torch.int64, device="cuda"))
        for layout, src in _layouts(R, cf):
            got = rh.regrid(src.view(torch.float64).view(-1), nlev=nlev, nfields=NF, layout=layout)
            assert torch.equal(_bits(torch, got).view(NF, nlev, -1), want), (case, nlev, layout)


@pytest.mark.parametrize("case", CASES)
def test_three_point_sum_keeps_the_sign_of_zero(gpu_lib, cases, case):
    """Every source value is -0.0: w0 * -0.0 is -0.0 for w0 >= 0, and fma(w, -0.0, -0.0) stays -0.0 for w >= 0, so a mapped point
    with three non-negative weights must come out as -0.0 from every 3-point kernel; an unmapped point is +0.0.  (A point within
    the inside tolerance of a triangle edge may carry a weight below zero: +0.0 enters its sum, it is left out here.)"""
    import torch
    from mpassit_amd import regrid as R
    rh = cases[case]["bilinear"]
    idx, w = rh.weights()
    mapped = idx[:, 0] >= 0
    qual = mapped & ~np.signbit(w).any(axis=1)
    print("sign of zero, %s: %d points, %d mapped, %d with three non-negative weights" % (case, rh.n_dst, mapped.sum(), qual.sum()))
    assert mapped.sum() > 0 and qual.sum() >= 0.99 * mapped.sum(), "badly constructed case: too few points qualify"
    qual_d, unmapped_d = torch.as_tensor(qual, device="cuda"), torch.as_tensor(~mapped, device="cuda")
    try:
        for knob, values, layout in (("a3_staged", (-2, 0, 1, 2), R.LAYOUT_CELL_FAST), ("lf_variant", (0, 1, 2), R.LAYOUT_LEV_FAST)):
            for v in values:
                gpu_lib.tune(knob, v)
                for nlev in NLEVS:
                    src = torch.full((NF * nlev * rh.n_src,), -0.0, dtype=torch.float64, device="cuda")   # all -0.0: the same in both layouts
                    got = _bits(torch, rh.regrid(src, nlev=nlev, nfields=NF, layout=layout)).view(NF * nlev, -1)
                    assert bool((got[:, qual_d] == NEG_ZERO).all()), (case, knob, v, nlev, "a -0.0 sum lost its sign")
                    assert bool((got[:, unmapped_d] == 0).all()), (case, knob, v, nlev, "an unmapped point is not +0.0")
            gpu_lib.tune(knob, -1)
    finally:
        gpu_lib.tune("a3_staged", -1)
        gpu_lib.tune("lf_variant", -1)
