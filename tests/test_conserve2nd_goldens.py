"""The numpy mirror of mpg_handle_conserve2nd (target_grid._conserve2nd_rows) on the CPU, against the 50-digit goldens of
tests/golden/make_conserve2nd_goldens.py (mpmath, brute force, straight from the header's steps 1 to 6, the exact 2 atan2 triangle area,
N1 from verticesOnCell alone: nothing of the mirror): rowptr, col, the pass flags and the statistics identical, val within BAR absolute,
the pieces' and cells' areas within BAR times the largest cell area.  Mesh -> Mesh, Mesh -> Grid and Grid -> Mesh all run here.

The bar, 1e-12, one for all cases.  The weights are O(1).  delta_q is a difference of two near-equal vectors of size h (the cell's angular
width) carrying eps each, b is of size 1 / h, so a value carries about eps / h: 2.2e-16 / 0.016 = 1.4e-14 on the 100-km hex cells, which
is what is measured.  Measured on the stored inputs, each figure against the golden (conserve2nd_hp.json "_measured" holds them, the tests
below reproduce them): worst |mirror - golden|, and worst |mirror on inputs moved by a random last-bit change of every unit vector -
golden|:

    geo6 to vor             3.3e-16   8.3e-16        hex to grid9x7          2.4e-15   3.6e-15
    geo6 to vor masked      3.9e-16   8.3e-16        grid7x5 to hex          1.1e-14   1.5e-14
    hex to geo6 dstarea     1.1e-16   1.8e-16        grid2x2 to hex          5.8e-15   4.8e-15
    hex to geo6 fracarea    1.3e-15   6.9e-15        grid1x5 to hex          9.0e-15   1.5e-14
    geo6 to hex dstarea     1.4e-14   1.9e-14        reversed hex to geo6    1.1e-16   1.8e-16
    geo6 to hex fracarea    7.4e-15   1.8e-14

The larger of the two worsts is 1.9e-14 (the mirror's own worst change under that move is 2.0e-14); 1e-12 is the round number 53 x above
it, the margin for other seeds' rounding.  It is the bar of the GPU test too: the device has the mirror's bits on its own unit vectors,
which differ from the stored ones in last bits only, and that is what the second figure measures.  The five mutants of the rule that the
generator evaluates at the same 50 digits must each miss the bar by at least 100 x on their case; they miss it by 3.4e-4 (the stencil about
the cell centre), 1.5e-1 (delta_q about G_i), 1.4e-3 (b_i = 0), 4.8e-2 (masked cells left in the stencils) and 8.8e-7 (planar triangles)."""
import numpy as np
import pytest

import _conserve2nd_golden_cases as GC

BAR = 1e-12
CASES = ("geo6 to vor", "geo6 to vor masked", "hex to geo6 dstarea", "hex to geo6 fracarea", "geo6 to hex dstarea", "geo6 to hex fracarea",
         "hex to grid9x7", "grid7x5 to hex", "grid2x2 to hex", "grid1x5 to hex", "reversed hex to geo6")


@pytest.fixture(scope="module")
def golden():
    return GC.load()


def test_cases_reach_every_branch(golden):
    doc, cases = golden
    assert tuple(sorted(cases)) == tuple(sorted(CASES))
    r = {name: c["meta"]["reached"] for name, c in cases.items()}
    meta = {name: c["meta"] for name, c in cases.items()}
    assert 5 in r["geo6 to vor"]["source_polygon_sizes"] and r["geo6 to vor"]["sources_fully_covered"] == meta["geo6 to vor"]["n_src"] == 362
    m = r["geo6 to vor masked"]
    assert m["masked_sources"] == 22 and m["stencils_that_lost_a_masked_neighbour"] > 100 and meta["geo6 to vor masked"]["stats"][2] == 22
    for name in ("geo6 to hex dstarea", "geo6 to hex fracarea"):
        assert r[name]["sources_partly_covered"] > 0 and r[name]["sources_without_a_piece"] > 300
    assert r["hex to geo6 dstarea"]["empty_rows"] > 300 and meta["hex to geo6 dstarea"]["stats"][4] > 100, "empty rows, long rows"
    a, b = cases["hex to geo6 dstarea"], cases["hex to geo6 fracarea"]
    assert np.array_equal(a["col"], b["col"]) and np.abs(a["val"] - b["val"]).max() > 1e-3, "FRACAREA differs from DSTAREA"
    assert r["hex to grid9x7"]["rim_rows"] > 0 and r["hex to grid9x7"]["empty_rows"] > 0
    assert r["grid7x5 to hex"]["shifted_windows"] == 20 and r["grid7x5 to hex"]["stencil_sizes"] == [8]
    assert r["grid2x2 to hex"]["stencil_sizes"] == [3] and meta["grid2x2 to hex"]["stats"][1:3] == [4, 0]
    assert r["grid1x5 to hex"]["stencil_sizes"] == [0] and meta["grid1x5 to hex"]["stats"][1:3] == [0, 5], "the collinear stencils fail"
    rev = r["reversed hex to geo6"]
    assert rev["reversed_sources"] > 50 and rev["reversed_destinations"] > 100
    assert not any(r[n]["reversed_sources"] or r[n]["reversed_destinations"] for n in r if n != "reversed hex to geo6")
    # the rule turns a reversed listing back: the expectation of the reversed pair is the unreversed pair's, up to area(d)'s last bits (its
    # fan starts at the other end of the listing, and the stored vectors are unit vectors to an ulp only)
    assert np.abs(cases["reversed hex to geo6"]["val"] - cases["hex to geo6 dstarea"]["val"]).max() < 1e-16
    assert np.array_equal(cases["reversed hex to geo6"]["G"], cases["hex to geo6 dstarea"]["G"])
    assert not np.array_equal(cases["reversed hex to geo6"]["src"]["voc"], cases["hex to geo6 dstarea"]["src"]["voc"])


def test_margins_hold(golden):
    """The conditions under which the golden's discrete decisions are float64's decisions too."""
    doc, _ = golden
    assert len(doc["_margins"]) == 8
    for pair, m in doc["_margins"].items():
        assert m["inside_smallest_above_1e-15"] > 1e-12 and m["inside_largest_at_or_below_1e-15"] < 1e-18, pair
        assert m["side_squared_smallest"] > 1e-21, pair
        assert m["det_ratio_smallest_passing"] is None or m["det_ratio_smallest_passing"] > 4 * 2.0 ** -26, pair
        assert m["det_ratio_largest_failing"] < 2.0 ** -26 / 4, pair
        assert m["piece_area_smallest_positive"] >= 1e-20, pair
    assert 0 < doc["_margins"]["grid1x5 -> hex"]["det_ratio_largest_failing"] < 1e-12, "the 1 x 5 grid falls far below 2^-26"


@pytest.mark.parametrize("name", CASES)
def test_mirror_against_the_goldens(golden, oracle, name):
    from mpassit_amd import target_grid as tg
    c = golden[1][name]
    rowptr, col, val, info = GC.run_mirror(oracle, tg, c)
    assert np.array_equal(rowptr, c["rowptr"]) and np.array_equal(col, c["col"]), "the pattern is the golden's"
    assert np.array_equal(info["pass"], c["pass"] != 0), "the pass flags are the golden's"
    assert np.array_equal(info["sptr"], c["sptr"]) and np.array_equal(info["scol"], c["scol"]), "the stencils' members are the golden's"
    assert info["stats"] == c["meta"]["stats"], (info["stats"], c["meta"]["stats"])
    worst = float(np.abs(val - c["val"]).max())
    scale = c["meta"]["largest_cell_area"]
    areas = {k: float(np.abs(info[k] - c[k]).max()) for k in ("Aq", "Ai", "area_d")}
    print("%s: %d entries, worst |mirror - golden| %.3g (bar %.0e); areas %s (bar %.3g)" % (name, col.size, worst, BAR, areas, BAR * scale))
    assert np.abs(c["val"]).max() < 10.0 and np.abs(val).max() < 10.0, "the weights are O(1)"
    assert worst <= BAR
    assert max(areas.values()) <= BAR * scale


@pytest.mark.parametrize("name", CASES)
def test_sensitivity_to_input_rounding(golden, oracle, name):
    """Every stored unit vector moved by a random last-bit change and renormalised: the pattern stays, val stays within the bar of the
    golden, and both measured figures are the json's and lie 16 x inside the bar."""
    from mpassit_amd import target_grid as tg
    doc, cases = golden
    got = GC.measure(oracle, tg, cases[name])
    print("%s: %s" % (name, got))
    assert max(got["mirror_minus_golden"], got["one_ulp_minus_golden"]) <= BAR / 16
    assert got == pytest.approx(doc["_measured"][name], rel=1e-6, abs=1e-18), "the json's figures are these"


def test_the_bar_and_the_mutants(golden):
    doc, cases = golden
    largest = max(max(m["mirror_minus_golden"], m["one_ulp_minus_golden"]) for m in doc["_measured"].values())
    print("the larger of the two worst figures %.3g; bar %.0e = %.0f x above" % (largest, BAR, BAR / largest))
    assert sorted(doc["_measured"]) == sorted(CASES) and BAR >= 16 * largest
    assert sorted(doc["_mutants"]) == ["1", "2", "3", "4", "5"]
    for k, m in sorted(doc["_mutants"].items()):
        c = cases[m["case"]]
        miss, _, one_sided = GC.union_difference(m["rows"], (c["rowptr"], c["col"], c["val"]))
        print("mutant %s (%s) on %s: misses by %.3g = %.0f x the bar; %d entries on one side only" % (k, m["what"], m["case"], miss, miss / BAR, one_sided))
        assert miss >= 100 * BAR and miss == pytest.approx(m["worst_difference_from_the_golden"], rel=1e-9)
    assert doc["_mutants"]["2"]["case"].startswith("geo6 to hex") and doc["_mutants"]["4"]["case"] == "geo6 to vor masked"


def test_generator_and_fixture_stay_together(golden, oracle):
    """A few rows of one case evaluated again by the generator: the stored bytes."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("make_conserve2nd_goldens", os.path.join(GC.HERE, "golden", "make_conserve2nd_goldens.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    doc, cases = golden
    name, n = doc["recheck"]["case"], doc["recheck"]["rows"]
    assert (name, n) == gen.RECHECK and [c[0] for c in gen.case_list()] == list(CASES)
    c = cases[name]
    problem = gen.Problem(oracle)
    rp, col, sm = problem.inputs(name)
    assert np.array_equal(rp, c["in_rowptr"]) and np.array_equal(col, c["in_col"]) and sm is None, "the reference's pattern is the stored one"
    for side, spec_ in ((c["src"], doc["sides"][c["meta"]["src_side"]]), (c["dst"], doc["sides"][c["meta"]["dst_side"]])):
        again = problem.arrays(spec_)
        assert all(np.array_equal(again[k].view(np.uint8), side[k].view(np.uint8)) for k in again), "the stored inputs are the generator's"
    which = gen.recheck_rows(rp, n)
    rowptr, ocol, val = problem.rule(name).rows(which)
    want_col = np.concatenate([c["col"][c["rowptr"][j]:c["rowptr"][j + 1]] for j in which])
    want_val = np.concatenate([c["val"][c["rowptr"][j]:c["rowptr"][j + 1]] for j in which])
    assert len(which) == n and val.size > 100
    assert np.array_equal(ocol, want_col) and np.array_equal(val.view(np.int64), want_val.view(np.int64))
