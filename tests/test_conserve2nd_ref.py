"""The numpy mirror of mpg_handle_conserve2nd (target_grid.conserve2nd_rows) alone, on the CPU: the cell pairs of
tests/_mesh_to_mesh_cases.py with the first-order pattern of the numpy reference (tests/_mesh_conserve_ref.py).  The two identities that
make the rule the right one -- column sums sum_j area_j c_(j,e) = A_e and first-order row sums -- within the project's conservative bar,
applied as test_conservation_global_to_global applies it; every stencil forced to fail gives the first-order weights of the same areas
exactly; the re-clip agrees with the reference's intersections; and the accuracy claim.

Accuracy, measured here (RMS over all 1500 destination cells of vor1500, the field of test_patch_gpu.py, means by a fan-subdivision
quadrature of 256 triangles per fan triangle): geodesic_mesh(8): first order 1.92e-2, second order 1.47e-3; geodesic_mesh(16): first order
3.32e-3, second order 1.16e-4.  From frequency 8 to 16 the first-order error falls by 5.8, the second-order error by 12.7; the bar is
2^1.5 = 2.83 (theory: 4 against 2)."""
import numpy as np
import pytest

import _conserve2nd_cases as CC
import _mesh_conserve_ref as MR
import _mesh_to_mesh_cases as MC

NORMS = [MR.NORM_DSTAREA, MR.NORM_FRACAREA]


def _rows(rp):
    return np.repeat(np.arange(rp.size - 1), np.diff(rp))


@pytest.mark.parametrize("name", MR.PAIRS)
def test_identities(oracle, name):
    a = MR.answer(oracle, name)
    rp1, col1, val1, _ = a.rows(MR.NORM_DSTAREA)
    rp, col, val, info = CC.mirror(oracle, name, MR.NORM_DSTAREA)
    n_dst, n_src = a.dst.nCells, a.src.nCells
    rows, rows1 = _rows(rp), _rows(rp1)
    # the re-clip is the reference's clip with another triangle area: the same pieces within the bar
    w = info["Aq"] / a.area_d[rows1]
    print("%s: re-clip worst %.3e, bar %.3e" % (name, np.abs(w - val1).max(), a.tol))
    assert np.abs(w - val1).max() <= a.tol and np.abs(info["area_d"] - a.area_d).max() <= a.tol
    # conservation, as test_conservation_global_to_global applies the bar
    x = np.random.default_rng(17).normal(size=n_src)
    lhs = float((a.area_d * np.bincount(rows, weights=val * x[col], minlength=n_dst)).sum())
    rhs, bar = float((info["Ai"] * x).sum()), a.tol * float((a.area_s * np.abs(x)).sum())
    print("conservation %s: %.3e apart, bar %.3e" % (name, abs(lhs - rhs), bar))
    assert abs(lhs - rhs) <= bar
    cs = np.bincount(col, weights=val * a.area_d[rows], minlength=n_src)
    assert np.abs(cs - info["Ai"]).max() <= a.tol * a.area_s.max(), "column sums: sum_j area_j c_je = A_e"
    if name in ("geo10_to_vor1500", "varres3000_to_geo8"):                       # a global destination covers every source cell
        assert np.abs(info["Ai"] - a.area_s).max() <= a.tol * a.area_s.max(), "a covered source cell keeps its whole area"
    # row sums equal the first-order row sums, under both norms
    for norm in NORMS:
        r1, c1, v1, _ = a.rows(norm)
        r2, c2, v2, _ = CC.mirror(oracle, name, norm)
        d = np.abs(np.bincount(_rows(r2), weights=v2, minlength=n_dst) - np.bincount(_rows(r1), weights=v1, minlength=n_dst)).max()
        print("row sums %s norm %d: worst %.3e" % (name, norm, d))
        assert d <= a.tol
        assert np.array_equal(np.diff(r2) == 0, np.diff(r1) == 0), "an empty input row stays empty"
    st = info["stats"]
    assert st[0] == col1.size and st[1] + st[2] == n_src and st[1] > 0.9 * n_src and st[3] == info["scol"].size and st[4] == np.diff(rp).max()
    assert val.min() < 0.0, "weights can be negative: there is no limiter"


@pytest.mark.parametrize("norm", NORMS, ids=["dstarea", "fracarea"])
@pytest.mark.parametrize("name", ["geo10_to_vor1500", "hex_to_geo10"])
def test_failing_stencils_give_first_order(oracle, name, norm):
    from mpassit_amd import target_grid as tg
    a = MR.answer(oracle, name)
    rp1, col1, _, _ = a.rows(norm)
    rp, col, val, info = CC.mirror(oracle, name, norm, first_order=True)
    assert np.array_equal(rp, rp1) and np.array_equal(col, col1), "the first-order pattern"
    rows = _rows(rp1)
    div = info["area_d"][rows] if norm == MR.NORM_DSTAREA else tg._c2_seq_sum(info["Aq"], rows, a.dst.nCells)[rows]
    assert np.array_equal(val.view(np.int64), (info["Aq"] / div).view(np.int64)), "the first-order weights of the same areas, exactly"
    assert info["stats"][1] == 0 and info["stats"][3] == a.src.nCells


def test_masked_cells_take_no_part(oracle):
    from mpassit_amd import target_grid as tg
    a = MR.answer(oracle, "geo10_to_vor1500")
    rp1, col1, _, _ = a.rows(MR.NORM_DSTAREA)
    sm = np.zeros(a.src.nCells, bool)
    sm[::17] = True
    keep = ~sm[col1]                                                            # the ENTRY rule's pattern
    rpm = np.concatenate([[0], np.cumsum(np.bincount(_rows(rp1)[keep], minlength=a.dst.nCells))])
    args = (rpm, col1[keep], (a.ps[0], a.ps[1], MC.cell_xyz(oracle, a.src)), a.pd, CC.neighbours_of(oracle, a.src), MR.NORM_DSTAREA)
    rp, col, val, info = tg._conserve2nd_rows(*args, src_mask=sm)
    owner = np.repeat(np.arange(a.src.nCells), np.diff(info["sptr"]))
    assert not sm[col].any() and not sm[info["scol"][~sm[owner]]].any(), "no stencil of an unmasked cell holds a masked id"
    assert (np.diff(info["sptr"])[sm] == 1).all() and not info["pass"][sm].any(), "a masked cell keeps the single entry of a failed stencil"
    zero = tg.conserve2nd_rows(*args, src_mask=np.zeros(a.src.nCells, np.uint8))
    none = tg.conserve2nd_rows(*args)
    assert all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(zero, none))


def test_accuracy(oracle):
    """RMS error over the destination cells whose sources are all fully covered: second order below first order at both resolutions, and
    falling by more than 2^1.5 from frequency 8 to 16 (the figures are in this module's docstring and in profiles/r30_conserve2nd.md)."""
    from mpassit_amd import target_grid as tg
    err = {}
    for freq in CC.ACCURACY_FREQS:
        a, xs, xd = CC.accuracy_case(oracle, freq)
        rp1, col1, val1, _ = a.rows(MR.NORM_DSTAREA)
        rp, col, val = tg.conserve2nd_rows(rp1, col1, (a.ps[0], a.ps[1], MC.cell_xyz(oracle, a.src)), a.pd, CC.neighbours_of(oracle, a.src),
                                           MR.NORM_DSTAREA)
        e1, e2, n = CC.rms_errors(rp1, col1, val1, rp, col, val, (a.area_s, a.area_d), xs, xd)
        print("geodesic_mesh(%d) -> vor1500: %d cells, RMS first order %.4e, second order %.4e" % (freq, n, e1, e2))
        assert n > 1000 and e2 < e1
        err[freq] = (e1, e2)
    r1, r2 = err[8][0] / err[16][0], err[8][1] / err[16][1]
    print("ratio from 8 to 16: first order %.2f, second order %.2f (bar 2^1.5 = %.2f)" % (r1, r2, 2 ** 1.5))
    assert r2 > 2 ** 1.5
