"""Output epilogues (write_data.F90:1339-1475 as device kernels) against the oracle's numpy restatement: bit-exact,
every operation is a single correctly rounded float64 op followed by the float64 -> float32 conversion."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_cast_layer_mean_ptop_bit_exact(oracle, gpu_lib):
    import torch

    from mpassit_amd import post
    rng = np.random.default_rng(11)
    for shape in ((5, 37, 41), (3, 1, 7), (56, 64, 129)):
        x = rng.normal(300.0, 40.0, shape) * 10.0 ** rng.integers(-3, 4, shape)
        assert np.array_equal(post.cast_f32(x), oracle.post_cast(x))
        assert np.array_equal(post.cast_f32(x, offset=-300.0), oracle.post_cast(x, offset=-300.0))
        assert np.array_equal(post.cast_f32(x, scale=9.81), oracle.post_cast(x, scale=9.81))
        assert np.array_equal(post.layer_mean_f32(x), oracle.post_layer_mean(x))
        xt = torch.as_tensor(x, device="cuda")
        odd = xt.reshape(-1)[1:]                                      # 8-byte aligned only: scalar path
        assert np.array_equal(post.cast_f32(odd).cpu().numpy(), oracle.post_cast(x.reshape(-1)[1:]))
        assert post.cast_f32(xt).dtype == torch.float32 and post.cast_f32(xt).is_cuda
        # big-endian results (the bytes nf90_put_var stores in a classic file): the oracle's values, byte-reversed
        for got, want in ((post.cast_f32(xt, scale=9.81, offset=-300.0, be=True), oracle.post_cast(x, scale=9.81, offset=-300.0)),
                          (post.cast_f32(odd, be=True), oracle.post_cast(x.reshape(-1)[1:])),
                          (post.layer_mean_f32(xt, be=True), oracle.post_layer_mean(x))):
            assert got.mpg_be and got.cpu().numpy().tobytes() == want.astype(">f4").tobytes()
    p = np.abs(rng.normal(5.0e4, 2.0e4, (55, 30, 40)))
    p[-1] = rng.uniform(0.0, 6000.0, (30, 40))
    p[-1, :3] = 0.0                                                   # unmapped columns (regrid leaves 0.0) are skipped
    assert post.p_top(p) == oracle.post_ptop(p)
    p[-1] = 5.0                                                       # no column reaches 10: maxval of the whole field
    assert post.p_top(p) == oracle.post_ptop(p) == np.float32(p.max())
    neg = -np.abs(p)
    assert post.p_top(neg) == oracle.post_ptop(neg)                   # ordered-key reduction handles negative values


def test_output_fields_follow_the_writer(oracle, gpu_lib):
    """post.output_fields on a tiny wrf_mod_vars run: names, order and values of what write_target_data would write."""
    import torch

    from mpassit_amd import interp as I, post, regrid as R, workloads
    m, g, nz, _ = workloads.workload("tiny")
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
    rng = np.random.default_rng(3)
    hist_2d = [("xland", "XLAND"), ("skintemp", "TSK"), ("snow", "SNOW")]
    hist_3d = [("zgrid", "PHB"), ("theta", "T"), ("uReconstructZonal", "U"), ("uReconstructMeridional", "V"), ("pressure", "P_HYD"),
               ("rho", "MUB")]
    inp = I.InputData(nz=nz, nzp1=nz + 1, nsoil=0, hgt=rng.uniform(0, 3000, m.nCells))
    inp.hist = {"xland": np.floor(rng.uniform(1, 3, m.nCells)), "skintemp": rng.uniform(250, 320, m.nCells),
                "snow": rng.uniform(0, 50, m.nCells), "zgrid": np.sort(rng.uniform(0, 2.0e4, (nz + 1, m.nCells)), axis=0),
                "theta": rng.uniform(280, 500, (nz, m.nCells)), "uReconstructZonal": rng.normal(0, 10, (nz, m.nCells)),
                "uReconstructMeridional": rng.normal(0, 10, (nz, m.nCells)),
                "pressure": -np.sort(-rng.uniform(2.0e3, 1.0e5, (nz, m.nCells)), axis=0), "rho": rng.uniform(0.1, 1.2, (nz, m.nCells))}
    cfg = I.InterpConfig(interp_diag=False, wrf_mod_vars=True, hist_2d=hist_2d, hist_3d=hist_3d)
    out = I.interp_data(mesh, grid, g, inp, cfg)
    res = post.output_fields(out, cfg)
    assert list(res) == ["HGT", "U", "V", "SNOW", "TSK", "XLAND", "T", "P_HYD", "P_TOP", "PB", "MUB", "MU", "Z_C", "PHB", "PH", "P"]
    assert all(v.dtype == np.float32 for k, v in res.items() if k != "P_TOP")
    assert np.array_equal(res["T"], oracle.post_cast(out["T"], offset=-300.0))
    assert np.array_equal(res["PHB"], oracle.post_cast(out["PHB"], scale=9.81))
    assert np.array_equal(res["Z_C"], oracle.post_layer_mean(out["PHB"])) and res["Z_C"].shape == (nz, g.ny, g.nx)
    assert res["P_TOP"] == oracle.post_ptop(out["P_HYD"]) and np.array_equal(res["PB"], res["P_HYD"])
    assert res["U"].shape == (nz, g.ny, g.nx + 1) and res["V"].shape == (nz, g.ny + 1, g.nx)
    for z in ("MU", "PH", "P"):
        assert not res[z].any()
    assert res["PH"].shape == (nz + 1, g.ny, g.nx) and res["P"].shape == (nz, g.ny, g.nx)
    # the device-resident route returns CUDA float32 tensors with the same bits
    out_t = {k: torch.as_tensor(v, device="cuda") for k, v in out.items()}
    res_t = post.output_fields(out_t, cfg)
    for k in res:
        if k != "P_TOP":
            assert res_t[k].is_cuda and np.array_equal(res_t[k].cpu().numpy(), res[k])
    mesh.destroy()
    grid.destroy()


# ---- paths the cases above never reach ---------------------------------------------------------------------------------------------------
PTOP_SHAPE = (5, 421, 500)          # 1 052 500 elements: k_post_ptop's launch covers 1 048 576, its grid-stride loop runs a second round
PTOP_PASS = 4096 * 256


def _ptop_field(rng):
    p = rng.uniform(2.0e4, 9.0e4, PTOP_SHAPE)
    p[-1] = rng.uniform(2000.0, 6000.0, PTOP_SHAPE[1:])
    return p


def test_ptop_beyond_the_first_pass_of_the_grid_stride_loop(oracle, gpu_lib):
    """P_HYD of 1 052 500 elements, its top plane from flat index 842 000 on: the element that decides P_TOP sits once just before and
    once just after flat index 1 048 576, where the second round of the loop begins -- the smallest candidate 0.8 * top, and the maximum
    (which decides only where no top value reaches 10: an all-negative field)"""
    from mpassit_amd import post
    rng = np.random.default_rng(21)
    n = int(np.prod(PTOP_SHAPE))
    top0 = n - PTOP_SHAPE[1] * PTOP_SHAPE[2]
    assert top0 == 842000 and top0 < PTOP_PASS < n
    base = _ptop_field(rng)
    for at in (PTOP_PASS - 7, PTOP_PASS - 1, PTOP_PASS, PTOP_PASS + 5, n - 1):
        p = base.copy()
        p.reshape(-1)[at] = 100.0 + at % 13                                   # the one candidate below every other: P_TOP = 0.8 * it
        want = oracle.post_ptop(p)
        assert want == np.float32(0.8 * (100.0 + at % 13)) and post.p_top(p) == want, at
        neg = -base
        neg.reshape(-1)[at] = -3.0 - at % 7                                   # no candidate at all: P_TOP is the maximum
        want = oracle.post_ptop(neg)
        assert want == np.float32(-3.0 - at % 7) and post.p_top(neg) == want, at
    low = base.copy()
    low[-1] = 5.0                                                             # a positive field without candidates, the maximum in either round
    for at in (500000, PTOP_PASS - 7, PTOP_PASS + 5):
        p = low.copy()
        p.reshape(-1)[at] = 2.5e5 if at < top0 else 9.5
        if at >= top0:
            p[:-1] = rng.uniform(1.0, 9.0, (PTOP_SHAPE[0] - 1,) + PTOP_SHAPE[1:])
        want = oracle.post_ptop(p)
        assert want == np.float32(p.reshape(-1)[at]) and post.p_top(p) == want, at


def test_ptop_parts_combine_to_the_whole(oracle, gpu_lib):
    """mpg_post_ptop_parts_dev on row blocks of one field: max of the vmax, min of the candmin over the blocks that have a candidate is
    P_TOP of the whole field, for every split; a block whose top values all stay below 10 reports has_cand == 0"""
    import ctypes as C
    import torch
    from mpassit_amd import _lib as L, post
    lib = L.load()
    rng = np.random.default_rng(22)
    p = _ptop_field(rng)
    p[-1, 0:1], p[-1, 400:] = 5.0, rng.uniform(0.0, 9.9, (21, PTOP_SHAPE[2]))          # rows without a candidate
    p[2, 300, 17] = 1.0e5                                                                # the maximum, far from the smallest candidate
    p[-1, 37, 499] = 40.0
    whole = post.p_top(p)
    assert whole == oracle.post_ptop(p) == np.float32(32.0)
    splits = {1: (421,), 2: (200, 221), 3: (100, 300, 21), 7: (1, 50, 99, 3, 150, 100, 18)}
    without = {1: (), 2: (), 3: (2,), 7: (0, 6)}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for nblk, rows in splits.items():
        assert len(rows) == nblk and sum(rows) == PTOP_SHAPE[1] and len(set(rows)) == nblk
        r0, vmaxs, cands = 0, [], []
        for b, nr in enumerate(rows):
            blk = torch.from_numpy(np.ascontiguousarray(p[:, r0:r0 + nr, :])).cuda()
            vmax, cand, has = C.c_double(np.nan), C.c_double(np.nan), C.c_int(-1)
            L.check(lib.mpg_post_ptop_parts_dev(C.c_void_p(blk.data_ptr()), C.c_int(PTOP_SHAPE[0]), C.c_int64(nr * PTOP_SHAPE[2]), C.byref(vmax),
                                                C.byref(cand), C.byref(has), stream))
            assert has.value == (0 if b in without[nblk] else 1), (nblk, b, has.value)
            assert vmax.value == p[:, r0:r0 + nr, :].max(), (nblk, b)
            vmaxs.append(vmax.value)
            if has.value:
                top = p[-1, r0:r0 + nr, :]
                assert cand.value == (top[top >= 10.0] * 0.80).min(), (nblk, b)
                cands.append(cand.value)
            r0 += nr
        got = np.float32(min(max(vmaxs), min(cands)))
        assert got == whole == oracle.post_ptop(p), (nblk, got, whole)


def test_layer_mean_of_two_levels(oracle, gpu_lib):
    from mpassit_amd import post
    x = np.random.default_rng(23).normal(3000.0, 900.0, (2, 7, 9))
    got = post.layer_mean_f32(x)
    assert got.shape == (1, 7, 9) and np.array_equal(got, oracle.post_layer_mean(x))


@pytest.mark.parametrize("n", (1, 2, 3))
def test_cast_of_one_two_three_elements_at_every_alignment(oracle, gpu_lib, n):
    """mpg_post_cast_dev on 1, 2 and 3 elements, the source 16-byte aligned or 8 bytes off, the destination 8-byte aligned or 4 bytes
    off (the vector path needs both aligned; its last thread holds one element when n is odd), written between canary bands"""
    import ctypes as C
    import torch
    from _oracle_compare import Banded
    from mpassit_amd import _lib as L
    lib = L.load()
    x = np.random.default_rng(24 + n).normal(300.0, 40.0, n)
    buf = torch.full((n + 3,), 7.0e9, dtype=torch.float64, device="cuda")
    lead = (-buf.data_ptr() % 16) // 8
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for src_off in (0, 1):
        src = buf[lead + src_off:lead + src_off + n]
        src.copy_(torch.from_numpy(x))
        assert src.data_ptr() % 16 == 8 * src_off
        for dst_off in (0, 1):
            for scale, offset, be in ((1.0, 0.0, False), (9.81, 0.0, False), (1.0, -300.0, False), (1.0, -300.0, True)):
                out = Banded(torch, n, torch.float32, shift=dst_off)
                assert out.ptr() % 8 == 4 * dst_off
                L.check(lib.mpg_post_cast_dev(C.c_void_p(src.data_ptr()), C.c_int64(n), C.c_double(scale), C.c_double(offset), C.c_void_p(out.ptr()),
                                              C.c_int(int(be)), stream))
                torch.cuda.synchronize()
                want = oracle.post_cast(x, scale=scale, offset=offset)
                assert out.res.cpu().numpy().tobytes() == want.astype(">f4" if be else "<f4").tobytes(), (n, src_off, dst_off, scale, offset, be)
                out.assert_canaries(str((n, src_off, dst_off)))
