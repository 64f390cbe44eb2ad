"""The rows Regrid (mpg_regrid_rows_dev: [cell][lev] in, [cell][lev] out) held to its contract by identity: element [p][k] has the bits of
element [k][p] of mpg_regrid_typed_dev(MPG_LAYOUT_LEV_FAST) on the same handle -- for a 3-slot Mesh -> Mesh handle, a nearest handle and a
4-slot Grid -> Mesh handle, all four type pairs, an affine epilogue, inputs with -0.0, one and three fields, and level counts of one
lane, an odd row, a full wavefront, a wavefront plus one and more than two (1, 3, 55, 64, 65, 130).  Destinations of 1002, 162 and an
odd number of points: the last 64-point block holds 42, 34, ... points.  Results go into NaN-filled buffers between canary bands that
start one element into a 128-byte line (tests/_oracle_compare.py).  Also: the oracle's apply, unmapped points, refusals, graph capture
of the first-ever call, and the adjoint identity through the autograd op."""
import numpy as np
import pytest

import _mesh_to_mesh_cases as MC
from _oracle_compare import Banded, assert_all_finite, assert_close

pytestmark = pytest.mark.gpu

NLEVS = [1, 3, 55, 64, 65, 130]
APPLY_BAR = 2.4e-16          # the project's float64 apply bar, of max |field| (tests/test_odd_grid_oracle_gpu.py)


@pytest.fixture(scope="module")
def handles(gpu_lib):
    """bil: vor1500 -> geo10 (3 slots, 1002 points); bil_un: hex_large -> geo10 (3 slots, most points unmapped); near: geo10 -> geodesic(4)
    (1 slot, 162 points); grid4: a 40 x 30 Lambert grid -> a hex mesh that overhangs it (4 slots, unmapped rim, odd count)."""
    from mpassit_amd import regrid as R, synth, target_grid as tg
    g = tg.define_target_grid_params("lambert", 41, 31, dx=30000.0, dy=30000.0, **MC.LAMBERT)
    objs = dict(vor1500=R.Mesh.from_mpas(MC.mesh("vor1500")), geo10=R.Mesh.from_mpas(MC.mesh("geo10")),
                hex_large=R.Mesh.from_mpas(MC.mesh("hex_large")), geo4=R.Mesh.from_mpas(synth.geodesic_mesh(4)),
                over=R.Mesh.from_mpas(synth.regional_mesh_for_lambert(g.proj, 41, 31, 1501, margin=0.06, seed=17)),
                grid=R.Grid.from_proj(g, fill_target=False))
    h = dict(bil=R.regrid_store_mesh(objs["vor1500"], objs["geo10"]),
             bil_un=R.regrid_store_mesh(objs["hex_large"], objs["geo10"]),
             near=R.regrid_store_mesh(objs["geo10"], objs["geo4"], R.REGRIDMETHOD_NEAREST_STOD),
             grid4=R.regrid_store_to_mesh(objs["grid"], objs["over"]))
    assert (h["bil"].nnz_per_row, h["near"].nnz_per_row, h["grid4"].nnz_per_row) == (3, 1, 4)
    assert (h["bil"].n_dst % 64, h["near"].n_dst % 64) == (42, 34) and h["grid4"].n_dst % 64 != 0
    yield h
    for rh in h.values():
        rh.release()
    for k in ("vor1500", "geo10", "hex_large", "geo4", "over", "grid"):
        objs[k].destroy()


def _bytes_equal(a, b):
    import torch
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    bits = torch.int64 if a.dtype == torch.float64 else torch.int32       # compared as integers: -0.0 is not +0.0, NaN equals itself
    return torch.equal(a.reshape(-1).view(bits), b.reshape(-1).view(bits))


def _source(torch, rh, nfields, nlev, sdt, seed, span=80.0):
    """nfields slabs of [n_src][nlev], i.i.d. in [-span / 2, span / 2), a sprinkling of -0.0 and +0.0."""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    src = (torch.rand((nfields, rh.n_src, nlev), dtype=torch.float64, device="cuda", generator=gen) - 0.5) * span
    z = torch.rand(src.shape, device="cuda", generator=gen)
    src = torch.where(z < 0.02, torch.full_like(src, -0.0), src)
    src = torch.where(z > 0.99, torch.zeros_like(src), src)
    return src.to(sdt)


def _rows_banded(torch, rh, src, nlev, nfields, ddt, scale, offset):
    """regrid_rows into a NaN-filled, canary-banded buffer that starts one element into a line; every element must have been written."""
    n = nfields * rh.n_dst * nlev
    band = Banded(torch, n, ddt, shift=1)
    got = rh.regrid_rows(src, nlev=nlev, nfields=nfields, out_dtype=ddt, scale=scale, offset=offset, out=band.res)
    assert got.data_ptr() == band.ptr()
    band.assert_canaries("regrid_rows")
    assert_all_finite(band.res, "regrid_rows (an unwritten element?)")
    return band.res.clone().reshape(nfields, rh.n_dst, nlev)


@pytest.mark.parametrize("nlev", NLEVS)
@pytest.mark.parametrize("types", ["f64f64", "f32f32", "f32f64", "f64f32"])
@pytest.mark.parametrize("which", ["bil", "bil_un", "near", "grid4"])
def test_rows_is_the_typed_regrid_transposed(handles, which, types, nlev):
    import torch
    from mpassit_amd import regrid as R
    dt = {"f64": torch.float64, "f32": torch.float32}
    sdt, ddt = dt[types[:3]], dt[types[3:]]
    rh = handles[which]
    for nfields, scale, offset in ((1, 1.0, 0.0), (3, 9.81, -300.0)):
        src = _source(torch, rh, nfields, nlev, sdt, 1000 + 10 * nlev + nfields)
        want = rh.regrid_typed(src.reshape(-1), nlev=nlev, nfields=nfields, layout=R.LAYOUT_LEV_FAST, out_dtype=ddt, scale=scale,
                               offset=offset).reshape(nfields, nlev, rh.n_dst)
        got = _rows_banded(torch, rh, src, nlev, nfields, ddt, scale, offset)
        assert _bytes_equal(got, want.transpose(1, 2).contiguous()), "regrid_rows [p][k] is not regrid_typed(LEV_FAST) [k][p]"
        assert _bytes_equal(rh.regrid_rows(src, nlev=nlev, nfields=nfields, out_dtype=ddt, scale=scale, offset=offset), got), "a second call differs"
        if nfields > 1:
            for f in range(nfields):
                one = rh.regrid_rows(src[f].contiguous(), nlev=nlev, out_dtype=ddt, scale=scale, offset=offset)
                assert _bytes_equal(one[0], got[f]), "field %d of a batch differs from its single call" % f


@pytest.mark.parametrize("which", ["bil", "bil_un", "near", "grid4"])
def test_rows_against_the_oracle(handles, oracle, which):
    """float64 in and out against orc_apply_fixed on the handle's own weights, source in [cell][lev] order, transposed.

    The bar is relative to max|field| and comes from tests/test_odd_grid_oracle_gpu.py, whose sources are i.i.d. in [-30, 30): results
    there lie in binades up to [16, 32), where 2.4e-16 x 30 is two units in the last place -- the most the kernel's fma chain (geom.h
    wsum3) and the oracle's separate multiplies and adds were seen apart.  So the sources here are drawn the same way.  (With sources
    in [-40, 40) -- results up to the binade [32, 64), whose unit is 1.8e-16 x 40 -- the same kernel measured 2.665e-16 of max|field| on
    the 3-slot handle at 55 levels: 1.5 units of that binade, beyond a bar that leaves room for 1.35.)"""
    import torch
    rh = handles[which]
    gi, gw = rh.weights()
    for nlev in (3, 55):
        src = _source(torch, rh, 1, nlev, torch.float64, 7 + nlev, span=60.0)
        ref = torch.as_tensor(oracle.apply_fixed(gi, gw, src.cpu().numpy().reshape(-1), nlev, lev_fast=True), device="cuda").t().contiguous()
        got = _rows_banded(torch, rh, src, nlev, 1, torch.float64, 1.0, 0.0)[0]
        e = assert_close(got, ref, APPLY_BAR, float(src.abs().max()), "regrid_rows vs the oracle (%s, %d levels)" % (which, nlev))
        print("%s nlev %d: largest difference %.3g of max|field|" % (which, nlev, e))


@pytest.mark.parametrize("which", ["bil_un", "grid4"])
def test_unmapped_points_get_the_epilogue_of_zero(handles, which):
    import torch
    rh = handles[which]
    un = torch.as_tensor(rh.weights()[0][:, 0] < 0, device="cuda")
    assert 0 < int(un.sum()) < rh.n_dst
    nlev = 5
    for sdt, ddt in ((torch.float64, torch.float64), (torch.float32, torch.float32), (torch.float64, torch.float32)):
        src = _source(torch, rh, 2, nlev, sdt, 3)
        for scale, offset in ((1.0, 0.0), (9.81, -300.0), (-2.0, 0.1)):
            got = _rows_banded(torch, rh, src, nlev, 2, ddt, scale, offset)
            want = torch.tensor(0.0 * scale + offset, dtype=torch.float64).to(ddt)          # (dst type)(0.0 * scale + offset)
            v = got[:, un, :].contiguous()
            assert _bytes_equal(v, want.to("cuda").expand(v.shape).contiguous()), (which, scale, offset)
            assert bool((got[:, ~un, :] != want.item()).any())


def test_refusals(handles, gpu_lib):
    import torch
    from mpassit_amd import _lib as L, regrid as R, target_grid as tg
    lib = L.load()

    def refused(rc, want, word=None):
        msg = lib.mpg_last_error().decode()
        assert rc == want and msg, (rc, want, msg)
        if word:
            assert word in msg, msg

    rh = handles["bil"]
    src = torch.zeros(2 * rh.n_src, dtype=torch.float64, device="cuda")
    dst = torch.zeros(2 * rh.n_dst, dtype=torch.float64, device="cuda")
    args = lambda **kw: [kw.get("rh", rh._h), kw.get("src", src.data_ptr()), kw.get("st", 0), kw.get("nlev", 2), kw.get("nf", 1),   # noqa: E731
                         kw.get("dst", dst.data_ptr()), kw.get("dt", 0), 1.0, 0.0, None]
    refused(L.regrid_rows_dev(*args(st=2)), L.MPG_ERR_UNSUPPORTED, "big-endian")
    refused(L.regrid_rows_dev(*args(dt=3)), L.MPG_ERR_UNSUPPORTED, "big-endian")
    refused(L.regrid_rows_dev(*args(st=4)), L.MPG_ERR_INVALID_ARG, "src_type")
    refused(L.regrid_rows_dev(*args(nlev=0)), L.MPG_ERR_INVALID_ARG, "nlev")
    refused(L.regrid_rows_dev(*args(nf=0)), L.MPG_ERR_INVALID_ARG, "nfields")
    refused(L.regrid_rows_dev(*args(rh=None)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(L.regrid_rows_dev(*args(src=None)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(L.regrid_rows_dev(*args(dst=None)), L.MPG_ERR_INVALID_ARG, "NULL")
    assert L.regrid_rows_dev(*args()) == 0
    torch.cuda.synchronize()
    # CSR handles
    rw = R.RouteHandle.from_weights(4, 2, 1, [1, 2], [1, 3], [1.0, 1.0])
    with pytest.raises(L.MpgError) as e:
        rw.regrid_rows(torch.zeros(4, dtype=torch.float64, device="cuda"))
    assert e.value.rc == L.MPG_ERR_UNSUPPORTED and "CSR" in str(e.value)
    rw.release()
    # pole caps: a Grid -> Grid handle of a periodic grid
    gl = tg.define_target_grid_params("lat-lon", nx=73, ny=37, stand_lon=0.0, is_regional=False)
    gp = R.Grid.from_target(gl)
    rp = R.regrid_store_grid(gp, R.STAGGERLOC_EDGE2)
    assert rp.pole()[0].size > 0
    with pytest.raises(L.MpgError) as e:
        rp.regrid_rows(torch.zeros(rp.n_src, dtype=torch.float64, device="cuda"))
    assert e.value.rc == L.MPG_ERR_UNSUPPORTED and "pole" in str(e.value)
    rp.release()
    gp.destroy()
    # the Python face: shapes and dtypes
    with pytest.raises(ValueError):
        rh.regrid_rows(torch.zeros(rh.n_src * 2 + 1, dtype=torch.float64, device="cuda"), nlev=2)
    with pytest.raises(ValueError):
        rh.regrid_rows(torch.zeros(rh.n_src * 2, dtype=torch.float16, device="cuda"), nlev=2)
    with pytest.raises(ValueError):
        rh.regrid_rows(torch.zeros(rh.n_src * 2, dtype=torch.float64, device="cuda"), nlev=0)
    with pytest.raises(ValueError):
        rh.regrid_rows(torch.zeros(rh.n_src * 2, dtype=torch.float64, device="cuda"), nlev=2, out=torch.zeros(3, dtype=torch.float64, device="cuda"))


def test_graph_capture_of_the_first_ever_call(gpu_lib):
    """A fresh handle's first-ever regrid_rows is recorded in a graph (after mpg_warmup_wait) and replayed: the bytes of the eager call."""
    import torch
    from mpassit_amd import regrid as R, synth
    src_mesh, dst_mesh = R.Mesh.from_mpas(synth.geodesic_mesh(7)), R.Mesh.from_mpas(synth.geodesic_mesh(9))
    rh = R.regrid_store_mesh(src_mesh, dst_mesh)
    assert gpu_lib.load().mpg_warmup_wait() == 0
    nlev = 55
    src = torch.rand((rh.n_src, nlev), dtype=torch.float32, device="cuda")
    out32 = torch.full((1, rh.n_dst, nlev), float("nan"), dtype=torch.float32, device="cuda")
    out64 = torch.full((1, rh.n_dst, nlev), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):        # one stream: a chain, no parallel branches
            rh.regrid_rows(src, nlev=nlev, out=out32, scale=2.0, offset=1.0)
            rh.regrid_rows(src, nlev=nlev, out=out64)
    for trial in range(2):
        src.mul_(-0.5).add_(0.25)
        graph.replay()
        torch.cuda.synchronize()
        got32, got64 = out32.clone(), out64.clone()
        assert _bytes_equal(got32, rh.regrid_rows(src, nlev=nlev, scale=2.0, offset=1.0))
        assert _bytes_equal(got64, rh.regrid_rows(src, nlev=nlev, out_dtype=torch.float64))
    rh.release()
    src_mesh.destroy()
    dst_mesh.destroy()


@pytest.mark.parametrize("which", ["bil", "bil_un", "near", "grid4"])
def test_adjoint_through_autograd(handles, which):
    """<A x, y> == <x, A^T y> within 1e-12 relative on random float64 x and y, A^T y taken from the backward of regrid_rows_autograd."""
    import torch
    from mpassit_amd import regrid as R
    rh = handles[which]
    rng = np.random.default_rng(13)
    for nlev, nfields in ((1, 1), (5, 2)):
        x = torch.as_tensor(rng.normal(size=(nfields, rh.n_src, nlev)), device="cuda").requires_grad_(True)
        y = torch.as_tensor(rng.normal(size=(nfields, rh.n_dst, nlev)), device="cuda")
        ax = R.regrid_rows_autograd(rh, x, nlev=nlev, nfields=nfields)
        assert _bytes_equal(ax.detach(), rh.regrid_rows(x.detach(), nlev=nlev, nfields=nfields))
        ax.backward(y)
        assert x.grad.shape == x.shape
        want = rh.regrid_transpose(y.transpose(1, 2).contiguous(), nlev=nlev, nfields=nfields, layout=R.LAYOUT_LEV_FAST)
        assert torch.equal(x.grad, want.reshape(x.shape)), "the backward is regrid_transpose(layout=LAYOUT_LEV_FAST) of the same handle"
        lhs, rhs = float((ax.detach() * y).sum()), float((x.detach() * x.grad).sum())
        print("%s nlev %d: <Ax, y> %.17g  <x, ATy> %.17g" % (which, nlev, lhs, rhs))
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))
        # float32 goes through the same op
        x32 = x.detach().to(torch.float32).requires_grad_(True)
        out = R.regrid_rows_autograd(rh, x32, nlev=nlev, nfields=nfields)
        out.backward(y.to(torch.float32))
        assert x32.grad.dtype == torch.float32 and x32.grad.shape == x32.shape
