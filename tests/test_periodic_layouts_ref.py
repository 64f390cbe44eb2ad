"""The periodic Grid -> Mesh reference (tests/_periodic_to_mesh_ref.py) on the grid layouts of tests/_periodic_layouts.py, on the CPU, checked
against the FIELD being interpolated rather than against a restatement of the rule: rows numbered north to south, Gaussian rows, rows on
the poles, a seam away from longitude 0.

A cap that takes its pole from the row NUMBER passes every other test of the reference on a grid numbered north to south -- rows sum to 1,
nothing is NaN, a constant is reproduced -- and hands Arctic points the values of the Antarctic end row (an error of 1.99 on sin(lat)).
The mutant "caps_by_row_index" is that rule; test_the_row_index_rule_fails_the_analytic_check shows these checks see it."""
import numpy as np
import pytest

import _periodic_layouts as PL
import _periodic_to_mesh_ref as PR
from _parity_helpers import assert_csr_equal

TIE_CAP = 1e-4            # tests/test_to_mesh_gpu.py
CASES = [(name, 0) for name in PL.LAYOUTS] + [(name, 1) for name in PL.WITH_VERTICES]


@pytest.fixture(scope="module")
def refs(oracle, global_mesh):
    """get(name, loc) -> (reference dict, mesh points [n][3]); each computed once and left unchanged."""
    m = global_mesh
    pts = {0: oracle.lonlat_deg_to_xyz(*oracle.mesh_coords_deg(m.lonCell, m.latCell)),
           1: oracle.lonlat_deg_to_xyz(*oracle.mesh_coords_deg(m.lonVertex, m.latVertex))}
    cache = {}

    def get(name, loc, mutate=None):
        key = (name, loc, mutate)
        if key not in cache:
            cache[key] = PR.periodic_to_mesh(oracle, PL.centers(oracle, name), pts[loc], mutate=mutate)
        return cache[key], pts[loc]
    get.oracle = oracle
    return get


def _errors(refs, name, loc, mutate=None):
    r, pts = refs(name, loc, mutate)
    src = PL.fields(PL.centers(refs.oracle, name).reshape(-1, 3))
    out = {f: PL.apply_csr(r["rowptr"], r["col"], r["val"], src[f]) for f in PL.FIELDS}
    return PL.field_errors(out, PL.fields(pts), r["kind"] == PR.KIND_CAP)


@pytest.mark.parametrize("name,loc", CASES)
def test_counts(refs, name, loc):
    r, _ = refs(name, loc)
    ncap, nseam = int((r["kind"] == PR.KIND_CAP).sum()), int(PR.seam_rows(r).size)
    share = PR.edge_share(r)
    print("%s loc %d: %d cap points, %d seam-quad points, share within 1e-9 of an edge %.3g" % (name, loc, ncap, nseam, share))
    assert not (r["kind"] == PR.KIND_NONE).any(), "no point may be unmapped"
    assert (ncap, nseam) == PL.COUNTS[(name, loc)]
    assert share <= TIE_CAP and share == 0.0
    lens = np.diff(r["rowptr"])
    rows = np.repeat(np.arange(lens.size), lens)
    assert np.isfinite(r["val"]).all() and r["val"].min() > -1e-9
    assert np.abs(np.bincount(rows, weights=r["val"], minlength=lens.size) - 1.0).max() < 1e-12


@pytest.mark.parametrize("name,loc", CASES)
def test_analytic_fields(refs, name, loc):
    """|interpolated - field| at the mesh points, for z, x and 1 + z + x y, over all rows and over the cap rows: a south-to-north layout
    within 1.05 x the recorded error of bilinear interpolation on that grid, a north-to-south one within its twin's error (x 1.01 + 1e-12)."""
    err = _errors(refs, name, loc)
    print("%s loc %d: %s" % (name, loc, ", ".join("%s %s %.4g" % (f, w, e) for (f, w), e in err.items() if e is not None)))
    if name in PL.TWIN:
        bound = PL.twin_bounds(_errors(refs, PL.TWIN[name], loc))
        assert set(k for k, v in bound.items() if v is not None) == set(k for k, v in err.items() if v is not None)
        for k, b in bound.items():
            if b is not None:
                assert err[k] <= b, (k, err[k], b)
    else:
        want = PL.S2N_ERRORS[name]
        for f in PL.FIELDS:
            assert err[(f, "all")] <= 1.05 * want[f], (f, err[(f, "all")], want[f])
        if want["cap z"] is None:
            assert err[("z", "cap")] is None
        else:
            assert err[("z", "cap")] <= 1.05 * want["cap z"], (err[("z", "cap")], want["cap z"])


@pytest.mark.parametrize("name,loc", [c for c in CASES if c[0] in PL.TWIN])
def test_row_flip_identity(refs, name, loc):
    """Reversing the rows of the same physical grid does not change the interpolation: with every column mapped by j -> ny - 1 - j the
    handle has its twin's row kinds, lengths and column sets, and its values within 1e-11."""
    r, _ = refs(name, loc)
    t, _ = refs(PL.TWIN[name], loc)
    nx, ny = r["nx"], r["ny"]
    rp, col, val = PL.flip_rows(r["rowptr"], r["col"], r["val"], nx, ny)
    assert np.array_equal(r["kind"], t["kind"]) and np.array_equal(rp, t["rowptr"])
    assert np.array_equal(col, t["col"]), "the column sets differ"
    common, only_a, only_b = assert_csr_equal(t["rowptr"], t["col"], t["val"], rp, col, val, nx * ny, tol=1e-11)
    assert only_a == 0 and only_b == 0 and common == col.size
    d = np.abs(val - t["val"])
    cap = np.repeat(r["kind"] == PR.KIND_CAP, np.diff(rp))
    print("%s loc %d: largest row-flip difference %.3g on quad rows, %.3g on cap rows" % (
        name, loc, d[~cap].max(), d[cap].max() if cap.any() else 0.0))


def test_the_row_index_rule_fails_the_analytic_check(refs):
    """The rule before this one -- row 0 always takes the pole (0, 0, -1) -- on `n2s`: Arctic points get the Antarctic end row."""
    bound = PL.twin_bounds(_errors(refs, "s2n", 0))
    err = _errors(refs, "n2s", 0, mutate="caps_by_row_index")
    print("caps_by_row_index on n2s: z error %.4g over the cap rows against a bound of %.4g" % (err[("z", "cap")], bound[("z", "cap")]))
    assert err[("z", "all")] > 1.0 and err[("z", "cap")] > 1.0 and bound[("z", "all")] < 0.0094
    assert err[("z", "all")] > bound[("z", "all")]
    # on its twin the old rule and the new one are the same rule
    a, _ = refs("s2n", 0)
    b, _ = refs("s2n", 0, mutate="caps_by_row_index")
    assert all(np.array_equal(a[k], b[k]) for k in ("rowptr", "col", "val"))
