"""Pitched destinations (mpg_*_pitched_dev, Handle.empty_pitched) on the 181 x 107 Lambert grid: 180 x 106 = 19 080 mass points per
level, so a dense float32 plane k starts k * 32 bytes (float64: k * 64) into a 128-byte line while the pitched planes all start on
one.  Every plane of a pitched result must be the dense result BIT FOR BIT (compared as integers: the sign of zero counts) and every
pad element must still hold the NaN it was filled with -- for every kernel that stores Regrid results, the pole caps, the wind chain,
a captured graph, and the pitched file write."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAN64, NAN32 = np.float64("nan").view(np.int64), np.float32("nan").view(np.int32)


def _int(torch, t):
    return t.view({8: torch.int64, 4: torch.int32}[t.element_size()])


def _pitched(torch, lead, ny, nx, dtype, ld):
    """NaN-filled storage of prod(lead) planes ld apart, and the (lead..., ny, nx) view on it."""
    nplanes = int(np.prod(lead))
    raw = torch.full((nplanes * ld,), float("nan"), dtype=dtype, device="cuda")
    st, acc = [], ld
    for s in reversed(lead):
        st.insert(0, acc)
        acc *= s
    return raw, raw.as_strided(tuple(lead) + (ny, nx), tuple(st) + (nx, 1))


def _assert_pitched(torch, raw, dense, ld, what):
    """raw: the pitched storage, dense: the dense result (any shape, planes of P = ny * nx points)."""
    torch.cuda.synchronize()
    P = dense.shape[-1] * dense.shape[-2]
    nplanes = dense.numel() // P
    planes = _int(torch, raw.view(nplanes, ld))
    want = _int(torch, dense.contiguous().view(nplanes, P))
    assert torch.equal(planes[:, :P], want), "%s: a pitched plane differs from the dense result" % what
    if ld > P:
        pad = planes[:, P:]
        sentinel = int(_int(torch, torch.tensor([float("nan")], dtype=raw.dtype))[0])
        assert bool((pad == sentinel).all()), "%s: the pad was written" % what
    assert bool((want != 0).any()), "%s: an all-zero result shows nothing" % what


def _both(torch, rh, call, lead, dtype, what):
    """call(out) on a dense result and on a pitched one (level_stride of the handle); compares them."""
    dense = torch.empty(tuple(lead) + (rh.ny_dst, rh.nx_dst), dtype=dtype, device="cuda")
    call(dense)
    ld = rh.level_stride(dtype)
    assert ld > rh.n_dst, "the test grid must have planes off a line"
    raw, view = _pitched(torch, lead, rh.ny_dst, rh.nx_dst, dtype, ld)
    call(view)
    _assert_pitched(torch, raw, dense, ld, what)
    return dense


@pytest.fixture(scope="module")
def case(gpu_lib, global_mesh, conus_grid_30km):
    import torch
    from mpassit_amd import regrid as R
    m, g = global_mesh, conus_grid_30km
    assert (g.nx, g.ny) == (180, 106)
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
    rng = np.random.default_rng(19080)
    nlev, nf = 9, 2
    s64 = torch.as_tensor(rng.normal(size=(nf, nlev, m.nCells)) * 40.0, device="cuda")
    yield dict(torch=torch, R=R, m=m, g=g, mesh=mesh, grid=grid, nlev=nlev, nf=nf, s64=s64,
               lf64=s64.transpose(1, 2).contiguous(), rng=rng)
    grid.destroy()
    mesh.destroy()


def _be(torch, t):
    """the big-endian bytes of a float32 tensor (as a NetCDF classic variable holds them), as float32 storage"""
    return torch.as_tensor(t.cpu().numpy().astype(">f4").view(np.float32).copy(), device="cuda")


def test_bilinear_cell_fast_f64_staged_and_lane_gather(case, gpu_lib):
    torch, R = case["torch"], case["R"]
    rh = R.regrid_store(case["mesh"], case["grid"], R.REGRIDMETHOD_BILINEAR)
    src, nlev, nf = case["s64"], case["nlev"], case["nf"]
    try:
        for staged in (-1, -2, 0):           # the default choice (staged on this grid), the lane gather, staged variant 0
            gpu_lib.tune("a3_staged", staged)
            _both(torch, rh, lambda o: rh.regrid(src.view(-1), nlev=nlev, nfields=nf, out=o), (nf, nlev), torch.float64,
                  "cell-fast f64 a3_staged %d" % staged)
            _both(torch, rh, lambda o: rh.regrid_typed(src.view(-1), nlev=nlev, nfields=nf, out_dtype=torch.float32, offset=-300.0, out=o),
                  (nf, nlev), torch.float32, "cell-fast f64->f32 a3_staged %d" % staged)
    finally:
        gpu_lib.tune("a3_staged", -1)
    rh.release()


@pytest.mark.parametrize("be", [False, True])
def test_file_order_f32_every_kernel(case, gpu_lib, be):
    torch, R = case["torch"], case["R"]
    rh = R.regrid_store(case["mesh"], case["grid"], R.REGRIDMETHOD_BILINEAR)
    nlev, nf = case["nlev"], case["nf"]
    src = case["lf64"].to(torch.float32)
    src = _be(torch, src) if be else src
    try:
        for lfv in (0, 2, 1):                # k_apply3_lf_rows, k_apply3_lf, the staged k_apply3_lfu
            gpu_lib.tune("lf_variant", lfv)
            _both(torch, rh, lambda o: rh.regrid_typed(src.view(-1), nlev=nlev, nfields=nf, layout=R.LAYOUT_LEV_FAST, out_dtype=torch.float32,
                                                       src_be=be, dst_be=be, out=o), (nf, nlev), torch.float32, "file order f32 be=%s lf_variant %d" % (be, lfv))
            _both(torch, rh, lambda o: rh.regrid_typed(src.view(-1), nlev=nlev, nfields=nf, layout=R.LAYOUT_LEV_FAST, out_dtype=torch.float64,
                                                       src_be=be, out=o), (nf, nlev), torch.float64, "file order f32->f64 be=%s lf_variant %d" % (be, lfv))
            _both(torch, rh, lambda o: rh.regrid(case["lf64"].view(-1), nlev=nlev, nfields=nf, layout=R.LAYOUT_LEV_FAST, out=o), (nf, nlev),
                  torch.float64, "file order f64 lf_variant %d" % lfv)
    finally:
        gpu_lib.tune("lf_variant", -1)
    rh.release()


def test_f32_to_f64_cell_fast(case, gpu_lib):
    torch, R = case["torch"], case["R"]
    rh = R.regrid_store(case["mesh"], case["grid"], R.REGRIDMETHOD_BILINEAR)
    src = case["s64"].to(torch.float32)
    _both(torch, rh, lambda o: rh.regrid_typed(src.view(-1), nlev=case["nlev"], nfields=case["nf"], out_dtype=torch.float64, out=o),
          (case["nf"], case["nlev"]), torch.float64, "cell-fast f32->f64")
    rh.release()


@pytest.mark.parametrize("method", ["nearest", "conserve", "edge1", "edge2"])
def test_nearest_conservative_and_destagger_handles(case, gpu_lib, method):
    torch, R = case["torch"], case["R"]
    nlev, nf = case["nlev"], case["nf"]
    if method in ("edge1", "edge2"):
        rh = R.regrid_store_grid(case["grid"], R.STAGGERLOC_EDGE1 if method == "edge1" else R.STAGGERLOC_EDGE2)
        src = torch.as_tensor(case["rng"].normal(size=(nf, nlev, case["g"].ny * case["g"].nx)), device="cuda")
    else:
        rh = R.regrid_store(case["mesh"], case["grid"], R.REGRIDMETHOD_NEAREST_STOD if method == "nearest" else R.REGRIDMETHOD_CONSERVE)
        src = case["s64"]
    lf = src.transpose(1, 2).contiguous()
    for layout, s in ((R.LAYOUT_CELL_FAST, src), (R.LAYOUT_LEV_FAST, lf)):
        _both(torch, rh, lambda o: rh.regrid(s.view(-1), nlev=nlev, nfields=nf, layout=layout, out=o), (nf, nlev), torch.float64,
              "%s f64 layout %d" % (method, layout))
        s32 = _be(torch, s.to(torch.float32))
        _both(torch, rh, lambda o: rh.regrid_typed(s32.view(-1), nlev=nlev, nfields=nf, layout=layout, out_dtype=torch.float32, src_be=True,
                                                   dst_be=True, out=o), (nf, nlev), torch.float32, "%s f32-BE layout %d" % (method, layout))
    rh.release()


def test_periodic_grid_pole_caps_fields_and_bundle(gpu_lib):
    import torch
    from mpassit_amd import regrid as R, target_grid as T
    t = T.define_target_grid_params("lat-lon", nx=73, ny=37, stand_lon=0.0, is_regional=False)   # 72 x 36, pole caps on EDGE2
    grid = R.Grid.from_target(t)
    rh = R.regrid_store_grid(grid, R.STAGGERLOC_EDGE2)
    assert rh.pole()[0].size > 0
    nlev, nf = 4, 3
    rng = np.random.default_rng(37)
    src = torch.as_tensor(rng.normal(size=(nf, nlev, t.nx * t.ny)) + 280.0, device="cuda")
    for layout, s in ((R.LAYOUT_CELL_FAST, src), (R.LAYOUT_LEV_FAST, src.transpose(1, 2).contiguous())):
        _both(torch, rh, lambda o: rh.regrid(s.view(-1), nlev=nlev, nfields=nf, layout=layout, out=o), (nf, nlev), torch.float64,
              "pole caps f64 layout %d" % layout)
        _both(torch, rh, lambda o: rh.regrid_typed(s.view(-1), nlev=nlev, nfields=nf, layout=layout, out_dtype=torch.float32, offset=-300.0,
                                                   out=o), (nf, nlev), torch.float32, "pole caps f32 layout %d" % layout)
    # the bundle call: separate arrays, per-field offsets
    srcs = [src[f].contiguous() for f in range(nf)]
    offs = [0.0, -300.0, 9.81]
    for dt in (torch.float64, torch.float32):
        dense = rh.regrid_bundle(srcs, nlev=nlev, out_dtype=dt, offsets=offs)
        ld = rh.level_stride(dt)
        pitched = [_pitched(torch, (nlev,), rh.ny_dst, rh.nx_dst, dt, ld) for _ in range(nf)]
        rh.regrid_bundle(srcs, nlev=nlev, out_dtype=dt, offsets=offs, outs=[v for _, v in pitched])
        for f in range(nf):
            _assert_pitched(torch, pitched[f][0], dense[f], ld, "bundle field %d %s" % (f, dt))
    rh.release()
    grid.destroy()


@pytest.mark.parametrize("out", ["f64", "f32be"])
def test_wind_destagger_pitched(gpu_lib, conus_grid_30km, out):
    import torch
    from mpassit_amd import regrid as R
    t = conus_grid_30km
    grid = R.Grid.from_target(t)
    rh_u, rh_v = R.regrid_store_grid(grid, R.STAGGERLOC_EDGE1), R.regrid_store_grid(grid, R.STAGGERLOC_EDGE2)
    nlev = 7
    rng = np.random.default_rng(7)
    um = torch.as_tensor(rng.normal(size=(nlev, t.ny, t.nx)) * 10.0, device="cuda")
    vm = torch.as_tensor(rng.normal(size=(nlev, t.ny, t.nx)) * 10.0, device="cuda")
    cosa = torch.as_tensor(np.ascontiguousarray(t.cosa), device="cuda")
    sina = torch.as_tensor(np.ascontiguousarray(t.sina), device="cuda")
    dt, be = (torch.float64, False) if out == "f64" else (torch.float32, True)
    u, v, _, _ = R.wind_destagger(rh_u, rh_v, cosa, sina, um, vm, nlev, out_dtype=dt, dst_be=be)
    ld = max(rh_u.level_stride(dt), rh_v.level_stride(dt))
    assert ld > max(rh_u.n_dst, rh_v.n_dst)
    ru, pu = _pitched(torch, (nlev,), rh_u.ny_dst, rh_u.nx_dst, dt, ld)
    rv, pv = _pitched(torch, (nlev,), rh_v.ny_dst, rh_v.nx_dst, dt, ld)
    R.wind_destagger(rh_u, rh_v, cosa, sina, um, vm, nlev, out_dtype=dt, dst_be=be, outs=(pu, pv))
    _assert_pitched(torch, ru, u, ld, "wind U %s" % out)
    _assert_pitched(torch, rv, v, ld, "wind V %s" % out)
    # one stride for both: U's own stride is below V's plane on this grid?  Either way a stride below the larger plane is refused
    from mpassit_amd import _lib as L
    lib = L.load()
    small = min(rh_u.n_dst, rh_v.n_dst)
    if small < max(rh_u.n_dst, rh_v.n_dst):
        rc = lib.mpg_wind_destagger_pitched_dev(rh_u._h, rh_v._h, C.c_void_p(cosa.data_ptr()), C.c_void_p(sina.data_ptr()), C.c_void_p(um.data_ptr()),
                                                C.c_void_p(vm.data_ptr()), C.c_int(nlev), C.c_void_p(ru.data_ptr()), C.c_void_p(rv.data_ptr()),
                                                C.c_int(int(dt == torch.float32) | (2 if be else 0)), None, None, C.c_int64(small), None)
        assert rc == L.MPG_ERR_INVALID_ARG
    rh_u.release()
    rh_v.release()
    grid.destroy()


def test_stride_equal_to_the_plane_is_the_dense_call_and_below_is_refused(case, gpu_lib):
    torch, R = case["torch"], case["R"]
    from mpassit_amd import _lib as L
    rh = R.regrid_store(case["mesh"], case["grid"], R.REGRIDMETHOD_BILINEAR)
    nlev, nf, src = case["nlev"], case["nf"], case["s64"]
    dense = rh.regrid(src.view(-1), nlev=nlev, nfields=nf)
    out = torch.full_like(dense, float("nan"))
    lib = L.load()
    rc = lib.mpg_regrid_pitched_dev(rh._h, C.c_void_p(src.data_ptr()), C.c_int(0), C.c_int(nlev), C.c_int(nf), C.c_void_p(out.data_ptr()),
                                    C.c_int64(rh.n_dst), None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(_int(torch, out), _int(torch, dense))
    for bad in (rh.n_dst - 1, 1, -rh.n_dst):
        rc = lib.mpg_regrid_pitched_dev(rh._h, C.c_void_p(src.data_ptr()), C.c_int(0), C.c_int(nlev), C.c_int(nf), C.c_void_p(out.data_ptr()),
                                        C.c_int64(bad), None)
        assert rc == L.MPG_ERR_INVALID_ARG
        rc = lib.mpg_regrid_typed_pitched_dev(rh._h, C.c_void_p(src.data_ptr()), C.c_int(0), C.c_int(0), C.c_int(nlev), C.c_int(nf),
                                              C.c_void_p(out.data_ptr()), C.c_int(0), C.c_double(1.0), C.c_double(0.0), C.c_int64(bad), None)
        assert rc == L.MPG_ERR_INVALID_ARG
    # a stride whose planes cannot be addressed: refused, never wrapped
    rc = lib.mpg_regrid_pitched_dev(rh._h, C.c_void_p(src.data_ptr()), C.c_int(0), C.c_int(nlev), C.c_int(nf), C.c_void_p(out.data_ptr()),
                                    C.c_int64(2 ** 62), None)
    assert rc == L.MPG_ERR_INVALID_ARG
    rh.release()


def test_python_out_views(case, gpu_lib):
    torch, R = case["torch"], case["R"]
    rh = R.regrid_store(case["mesh"], case["grid"], R.REGRIDMETHOD_BILINEAR)
    nlev, nf, src = case["nlev"], case["nf"], case["s64"]
    dense = rh.regrid(src.view(-1), nlev=nlev, nfields=nf)
    out = rh.empty_pitched(nlev, nfields=nf, dtype=torch.float64)
    ld = rh.level_stride(torch.float64)
    assert out.shape == (nf, nlev, rh.ny_dst, rh.nx_dst) and out.stride() == (nlev * ld, ld, rh.nx_dst, 1)
    got = rh.regrid(src.view(-1), nlev=nlev, nfields=nf, out=out)
    torch.cuda.synchronize()
    assert got is out and torch.equal(_int(torch, out.contiguous()), _int(torch, dense))
    out32 = rh.empty_pitched(nlev, nfields=nf, dtype=torch.float32)
    rh.regrid_typed(src.view(-1), nlev=nlev, nfields=nf, out_dtype=torch.float32, out=out32)
    want32 = rh.regrid_typed(src.view(-1), nlev=nlev, nfields=nf, out_dtype=torch.float32)
    torch.cuda.synchronize()
    assert torch.equal(_int(torch, out32.contiguous()), _int(torch, want32))
    # layouts that are not plane-pitched are refused
    full = torch.empty((nf, nlev, rh.nx_dst, rh.ny_dst), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        rh.regrid(src.view(-1), nlev=nlev, nfields=nf, out=full.transpose(2, 3))                  # transposed planes
    wide = torch.empty((nf, nlev, rh.ny_dst, rh.nx_dst + 3), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        rh.regrid(src.view(-1), nlev=nlev, nfields=nf, out=wide[..., :rh.nx_dst])                 # a row pitch
    big = torch.empty((nf * nlev + 1) * ld, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        rh.regrid(src.view(-1), nlev=nlev, nfields=nf, out=big.as_strided(out.shape, ((nlev + 1) * ld, ld, rh.nx_dst, 1)))   # field stride != nlev * ld
    rh.release()


def test_pitched_sequence_in_a_captured_graph(case, gpu_lib):
    torch, R = case["torch"], case["R"]
    rh = R.regrid_store(case["mesh"], case["grid"], R.REGRIDMETHOD_BILINEAR)
    rh_u = R.regrid_store_grid(case["grid"], R.STAGGERLOC_EDGE1)
    nlev, nf = case["nlev"], case["nf"]
    src = case["s64"].clone()
    src_lf32 = case["lf64"].to(torch.float32)
    mass = torch.as_tensor(case["rng"].normal(size=(nlev, case["g"].ny * case["g"].nx)), device="cuda")
    o1 = rh.empty_pitched(nlev, nfields=nf, dtype=torch.float64)
    o2 = rh.empty_pitched(nlev, nfields=nf, dtype=torch.float32)
    o3 = rh_u.empty_pitched(nlev, dtype=torch.float64)

    def step():
        rh.regrid(src.view(-1), nlev=nlev, nfields=nf, out=o1)
        rh.regrid_typed(src_lf32.view(-1), nlev=nlev, nfields=nf, layout=R.LAYOUT_LEV_FAST, out_dtype=torch.float32, dst_be=True, out=o2)
        rh_u.regrid(mass.view(-1), nlev=nlev, out=o3)

    step()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            step()
    for _ in range(2):
        src.mul_(-0.75)
        src_lf32.add_(1.5)
        mass.mul_(2.0)
        graph.replay()
        torch.cuda.synchronize()
        got = [_int(torch, t.contiguous()).clone() for t in (o1, o2, o3)]
        step()
        torch.cuda.synchronize()
        for a, b in zip(got, (o1, o2, o3)):
            assert torch.equal(a, _int(torch, b.contiguous()))
    for h in (rh, rh_u):
        h.release()


@pytest.mark.parametrize("plane_mb,nplanes", [(1, 5), (40, 2)])
def test_dev_to_file_planes(gpu_lib, tmp_path, plane_mb, nplanes):
    """planes below and above the 32 MB staging chunk: the file holds the dense bytes, in one call"""
    import torch
    from mpassit_amd import _lib as L
    plane = plane_mb * (1 << 20) + 12                  # not a multiple of a line, nor of the chunk
    pitch = plane + 116
    dev = torch.randint(0, 256, (nplanes * pitch,), dtype=torch.uint8, device="cuda")
    want = dev.view(-1)[: nplanes * pitch].cpu().numpy().reshape(nplanes, pitch)[:, :plane].tobytes()
    path = str(tmp_path / "planes.bin")
    off = 1000
    with open(path, "wb") as f:
        f.truncate(off + len(want) + 500)
    rc = L.load().mpg_dev_to_file_planes(path.encode(), C.c_int64(off), C.c_int64(plane), C.c_int64(nplanes), C.c_void_p(dev.data_ptr()),
                                         C.c_int64(pitch), None)
    assert rc == 0, L.load().mpg_last_error()
    data = open(path, "rb").read()
    assert data[off:off + len(want)] == want
    assert data[:off] == b"\0" * off and data[off + len(want):] == b"\0" * 500
    assert L.load().mpg_dev_to_file_planes(path.encode(), C.c_int64(0), C.c_int64(plane), C.c_int64(1), C.c_void_p(dev.data_ptr()),
                                           C.c_int64(plane - 1), None) == L.MPG_ERR_INVALID_ARG
    os.remove(path)
    rc = L.load().mpg_dev_to_file_planes(path.encode(), C.c_int64(0), C.c_int64(plane), C.c_int64(1), C.c_void_p(dev.data_ptr()),
                                         C.c_int64(pitch), None)       # the file is gone: the error names this call
    assert rc != 0 and L.load().mpg_last_error().decode().startswith("mpg_dev_to_file_planes:")
