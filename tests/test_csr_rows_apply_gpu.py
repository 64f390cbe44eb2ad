"""The CSR rows Regrid (mpg_regrid_csr_rows_dev: [cell][lev] in, [cell][lev] out, any CSR handle) held to its contract by identity:
element [p][k] has the bits of element [k][p] of mpg_regrid_typed_dev(MPG_LAYOUT_LEV_FAST) on the same handle -- all four type pairs, an
affine epilogue, one and three fields, level counts of one lane, an odd row, 55, a full wavefront and a wavefront plus six (1, 3, 55, 64,
70).  Handles: two conservative Mesh -> Mesh ones (hex_to_geo10: empty rows, 1002 = 15 * 64 + 42 rows; varres3000_to_geo8: 97-entry rows,
642 = 10 * 64 + 2 rows) and a synthetic one of mpg_handle_from_weights whose 200 rows of 0 .. 3000 entries make a 64-row run cross the
kernel's 1024-entry LDS chunks inside a row and exactly at a row's end.  Results go into NaN-filled buffers between canary bands that
start one element into a 128-byte line.  Also: empty rows, the oracle's apply, stability, graph capture of the first-ever call,
refusals, gradcheck of the autograd op."""
import numpy as np
import pytest

import _mesh_to_mesh_cases as MC
from _oracle_compare import Banded, assert_all_finite, assert_close

pytestmark = pytest.mark.gpu

NLEVS = [1, 3, 55, 64, 70]
LDS_CHUNK = 1024                                   # entries of a 64-row run resident in LDS (apply_mesh.h AM_CHUNK)
SYN_LENGTHS = [1, 1023, 0, 1024, 2, 1025, 3000]    # row lengths of the synthetic handle, repeated: 1 + 1023 ends a row ON a chunk boundary
SYN_ROWS, SYN_NSRC = 200, 4001


def _synthetic(R):
    rng = np.random.default_rng(29)
    lens = np.array([SYN_LENGTHS[p % len(SYN_LENGTHS)] for p in range(SYN_ROWS)])
    row = np.repeat(np.arange(1, SYN_ROWS + 1), lens)
    col = rng.integers(1, SYN_NSRC + 1, size=row.size)
    S = rng.normal(size=row.size) / np.sqrt(np.maximum(np.repeat(lens, lens), 1))
    return R.RouteHandle.from_weights(SYN_NSRC, SYN_ROWS, 1, row, col, S), lens


@pytest.fixture(scope="module")
def handles(gpu_lib):
    from mpassit_amd import regrid as R
    objs = {k: R.Mesh.from_mpas(MC.mesh(k)) for k in ("hex_large", "geo10", "varres3000", "geo8")}
    syn, lens = _synthetic(R)
    h = dict(hex=R.regrid_store_conserve_mesh(objs["hex_large"], objs["geo10"]),
             varres=R.regrid_store_conserve_mesh(objs["varres3000"], objs["geo8"], R.NORM_FRACAREA), syn=syn)
    for rh in h.values():
        assert rh.nnz_per_row == 0
    assert (h["hex"].n_dst, h["varres"].n_dst) == (15 * 64 + 42, 10 * 64 + 2)
    rp = h["hex"].csr()[0]
    assert (np.diff(rp) == 0).sum() > 100, "hex_to_geo10 has empty rows"
    assert np.diff(h["varres"].csr()[0]).max() >= 64, "varres3000_to_geo8 has rows of 97 entries"
    # the synthetic handle's first 64-row run: a row ends exactly on a chunk boundary, another one straddles one
    rp = h["syn"].csr()[0]
    assert np.array_equal(np.diff(rp), lens)
    ends, bounds = rp[1:65] - rp[0], np.arange(LDS_CHUNK, rp[64] - rp[0], LDS_CHUNK)
    assert np.isin(bounds, ends).any() and (~np.isin(bounds, ends)).any() and bounds.size > 10
    yield h
    for rh in h.values():
        rh.release()
    for m in objs.values():
        m.destroy()


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
    """regrid_csr_rows into a NaN-filled, canary-banded buffer that starts one element into a line; every element must have been written."""
    n = nfields * rh.n_dst * nlev
    band = Banded(torch, n, ddt, shift=1)
    got = rh.regrid_csr_rows(src, nlev=nlev, nfields=nfields, out_dtype=ddt, scale=scale, offset=offset, out=band.res)
    assert got.data_ptr() == band.ptr()
    band.assert_canaries("regrid_csr_rows")
    assert_all_finite(band.res, "regrid_csr_rows (an unwritten element?)")
    return band.res.clone().reshape(nfields, rh.n_dst, nlev)


@pytest.mark.parametrize("nlev", NLEVS)
@pytest.mark.parametrize("types", ["f64f64", "f32f32", "f32f64", "f64f32"])
@pytest.mark.parametrize("which", ["hex", "varres", "syn"])
def test_csr_rows_is_the_typed_regrid_transposed(handles, which, types, nlev):
    import torch
    from mpassit_amd import regrid as R
    dt = {"f64": torch.float64, "f32": torch.float32}
    sdt, ddt = dt[types[:3]], dt[types[3:]]
    rh = handles[which]
    for nfields, scale, offset in ((1, 1.0, 0.0), (3, 9.81, -300.0)):
        src = _source(torch, rh, nfields, nlev, sdt, 2000 + 10 * nlev + nfields)
        want = rh.regrid_typed(src.reshape(-1), nlev=nlev, nfields=nfields, layout=R.LAYOUT_LEV_FAST, out_dtype=ddt, scale=scale,
                               offset=offset).reshape(nfields, nlev, rh.n_dst)
        got = _rows_banded(torch, rh, src, nlev, nfields, ddt, scale, offset)
        assert _bytes_equal(got, want.transpose(1, 2).contiguous()), "regrid_csr_rows [p][k] is not regrid_typed(LEV_FAST) [k][p]"
        # stability: the same bits from a second call, and from every field of the batch on its own
        assert _bytes_equal(rh.regrid_csr_rows(src, nlev=nlev, nfields=nfields, out_dtype=ddt, scale=scale, offset=offset), got), "a second call differs"
        if nfields > 1:
            for f in range(nfields):
                one = rh.regrid_csr_rows(src[f].contiguous(), nlev=nlev, out_dtype=ddt, scale=scale, offset=offset)
                assert _bytes_equal(one[0], got[f]), "field %d of a batch differs from its single call" % f


@pytest.mark.parametrize("which", ["hex", "syn"])
def test_empty_rows_get_the_epilogue_of_zero(handles, which):
    import torch
    rh = handles[which]
    empty = torch.as_tensor(np.diff(rh.csr()[0]) == 0, device="cuda")
    assert 0 < int(empty.sum()) < rh.n_dst
    nlev = 5
    for sdt, ddt in ((torch.float64, torch.float64), (torch.float32, torch.float32), (torch.float64, torch.float32)):
        src = _source(torch, rh, 2, nlev, sdt, 3)
        for scale, offset in ((1.0, 0.0), (9.81, -300.0), (-2.0, 0.1)):
            got = _rows_banded(torch, rh, src, nlev, 2, ddt, scale, offset)
            want = torch.tensor(0.0 * scale + offset, dtype=torch.float64).to(ddt)          # (dst type)(0.0 * scale + offset)
            v = got[:, empty, :].contiguous()
            assert _bytes_equal(v, want.to("cuda").expand(v.shape).contiguous()), (which, scale, offset)
            assert bool((got[:, ~empty, :] != want.item()).any())


@pytest.mark.parametrize("which", ["hex", "varres", "syn"])
def test_csr_rows_against_the_oracle(handles, oracle, which):
    """float64 in and out against orc_apply_csr on the handle's own matrix, source in [cell][lev] order.  The kernel's row is an fma chain,
    the oracle's separate multiplies and adds: two evaluations of a dot product of n terms, each within (n + 1) / 2 * eps * sum |w| |x| of
    the exact value to first order -- so they lie within (n + 1) * eps * sum |w| * max |x| of each other, row by row."""
    import torch
    rh = handles[which]
    rp, col, val = rh.csr()
    n = np.diff(rp)
    sumw = np.bincount(np.repeat(np.arange(rh.n_dst), n), weights=np.abs(val), minlength=rh.n_dst)
    bar = torch.as_tensor((n + 1) * np.finfo(np.float64).eps * sumw, device="cuda")
    for nlev in (3, 55):
        src = _source(torch, rh, 1, nlev, torch.float64, 7 + nlev, span=60.0)
        ref = torch.as_tensor(oracle.apply_csr(rp, col, val, src.cpu().numpy().reshape(-1), nlev, lev_fast=True), device="cuda")   # [nlev][n_dst]
        got = _rows_banded(torch, rh, src, nlev, 1, torch.float64, 1.0, 0.0)[0].t().contiguous()
        scale = float(src.abs().max())
        worst = float(((got - ref).abs() / (bar * scale).clamp_min(1e-300)).max())
        print("%s nlev %d: largest difference %.3g of its row's bar (row lengths up to %d)" % (which, nlev, worst, n.max()))
        assert_close(got, ref, bar, scale, "regrid_csr_rows vs the oracle (%s, %d levels)" % (which, nlev))


def test_graph_capture_of_the_first_ever_call(gpu_lib):
    """A fresh handle's first-ever regrid_csr_rows is recorded in a graph (after mpg_warmup_wait) and replayed: the bytes of the eager call."""
    import torch
    from mpassit_amd import regrid as R
    src_mesh, dst_mesh = R.Mesh.from_mpas(MC.mesh("geo8")), R.Mesh.from_mpas(MC.mesh("vor1500"))
    rh = R.regrid_store_conserve_mesh(src_mesh, dst_mesh)
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
            rh.regrid_csr_rows(src, nlev=nlev, out=out32, scale=2.0, offset=1.0)
            rh.regrid_csr_rows(src, nlev=nlev, out=out64)
    for trial in range(2):
        src.mul_(-0.5).add_(0.25)
        graph.replay()
        torch.cuda.synchronize()
        got32, got64 = out32.clone(), out64.clone()
        assert _bytes_equal(got32, rh.regrid_csr_rows(src, nlev=nlev, scale=2.0, offset=1.0))
        assert _bytes_equal(got64, rh.regrid_csr_rows(src, nlev=nlev, out_dtype=torch.float64))
    rh.release()
    src_mesh.destroy()
    dst_mesh.destroy()


def test_refusals(handles, gpu_lib):
    import torch
    from mpassit_amd import _lib as L, regrid as R
    lib = L.load()

    def refused(rc, want, word=None):
        msg = lib.mpg_last_error().decode()
        assert rc == want and msg, (rc, want, msg)
        if word:
            assert word in msg, msg

    rh = handles["hex"]
    src = torch.zeros(2 * rh.n_src, dtype=torch.float64, device="cuda")
    dst = torch.zeros(2 * rh.n_dst, dtype=torch.float64, device="cuda")
    args = lambda **kw: [kw.get("rh", rh._h), kw.get("src", src.data_ptr()), kw.get("st", 0), kw.get("nlev", 2), kw.get("nf", 1),   # noqa: E731
                         kw.get("dst", dst.data_ptr()), kw.get("dt", 0), 1.0, 0.0, None]
    refused(L.regrid_csr_rows_dev(*args(st=2)), L.MPG_ERR_UNSUPPORTED, "big-endian")
    refused(L.regrid_csr_rows_dev(*args(dt=3)), L.MPG_ERR_UNSUPPORTED, "big-endian")
    refused(L.regrid_csr_rows_dev(*args(st=4)), L.MPG_ERR_INVALID_ARG, "src_type")
    refused(L.regrid_csr_rows_dev(*args(nlev=0)), L.MPG_ERR_INVALID_ARG, "nlev")
    refused(L.regrid_csr_rows_dev(*args(nf=0)), L.MPG_ERR_INVALID_ARG, "nfields")
    refused(L.regrid_csr_rows_dev(*args(rh=None)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(L.regrid_csr_rows_dev(*args(src=None)), L.MPG_ERR_INVALID_ARG, "NULL")
    refused(L.regrid_csr_rows_dev(*args(dst=None)), L.MPG_ERR_INVALID_ARG, "NULL")
    assert L.regrid_csr_rows_dev(*args()) == 0
    torch.cuda.synchronize()
    # the rows Regrid of fixed handles still refuses CSR handles, and names this call
    refused(L.regrid_rows_dev(*args()), L.MPG_ERR_UNSUPPORTED, "CSR")
    assert "mpg_regrid_csr_rows_dev" in lib.mpg_last_error().decode()
    with pytest.raises(L.MpgError) as e:
        rh.regrid_rows(src, nlev=2)
    assert e.value.rc == L.MPG_ERR_UNSUPPORTED and "CSR" in str(e.value)
    # fixed handles: the message names mpg_regrid_rows_dev
    a, b = R.Mesh.from_mpas(MC.mesh("geo8")), R.Mesh.from_mpas(MC.mesh("geo10"))
    for method in (R.REGRIDMETHOD_BILINEAR, R.REGRIDMETHOD_NEAREST_STOD):
        fx = R.regrid_store_mesh(a, b, method)
        with pytest.raises(L.MpgError) as e:
            fx.regrid_csr_rows(torch.zeros(fx.n_src, dtype=torch.float64, device="cuda"))
        assert e.value.rc == L.MPG_ERR_UNSUPPORTED and "mpg_regrid_rows_dev" in str(e.value)
        fx.release()
    a.destroy()
    b.destroy()
    # the Python face: shapes and dtypes
    with pytest.raises(ValueError):
        rh.regrid_csr_rows(torch.zeros(rh.n_src * 2 + 1, dtype=torch.float64, device="cuda"), nlev=2)
    with pytest.raises(ValueError):
        rh.regrid_csr_rows(torch.zeros(rh.n_src * 2, dtype=torch.float16, device="cuda"), nlev=2)
    with pytest.raises(ValueError):
        rh.regrid_csr_rows(torch.zeros(rh.n_src * 2, dtype=torch.float64, device="cuda"), nlev=0)
    with pytest.raises(ValueError):
        rh.regrid_csr_rows(torch.zeros(rh.n_src * 2, dtype=torch.float64, device="cuda"), nlev=2, out=torch.zeros(3, dtype=torch.float64, device="cuda"))


def test_autograd_gradcheck(gpu_lib):
    """gradcheck of regrid_csr_rows_autograd on a 40-row handle with two levels; the backward is regrid_transpose(layout=LAYOUT_LEV_FAST) of
    the same handle."""
    import torch
    from mpassit_amd import regrid as R
    rng = np.random.default_rng(5)
    n_src, n_dst, nlev = 31, 40, 2
    lens = rng.integers(0, 6, size=n_dst)
    lens[:3] = (0, 1, 5)
    row = np.repeat(np.arange(1, n_dst + 1), lens)
    rh = R.RouteHandle.from_weights(n_src, n_dst, 1, row, rng.integers(1, n_src + 1, size=row.size), rng.normal(size=row.size))
    assert rh.nnz_per_row == 0
    x = torch.as_tensor(rng.normal(size=(1, n_src, nlev)), device="cuda").requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: R.regrid_csr_rows_autograd(rh, t, nlev=nlev), (x,), eps=1e-6, atol=1e-7, rtol=1e-7)
    y = torch.as_tensor(rng.normal(size=(1, n_dst, nlev)), device="cuda")
    ax = R.regrid_csr_rows_autograd(rh, x, nlev=nlev)
    assert _bytes_equal(ax.detach(), rh.regrid_csr_rows(x.detach(), nlev=nlev))
    ax.backward(y)
    want = rh.regrid_transpose(y.transpose(1, 2).contiguous(), nlev=nlev, layout=R.LAYOUT_LEV_FAST)
    assert torch.equal(x.grad, want.reshape(x.shape)), "the backward is regrid_transpose(layout=LAYOUT_LEV_FAST) of the same handle"
    rh.release()
