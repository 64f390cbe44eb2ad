"""CPU qualification of the conservative Mesh -> Mesh reference (tests/_mesh_conserve_ref.py) and of the GPU test's inputs: the
reference against the oracle's Mesh -> Grid conservative matrix (destination polygons = the cells of a small Lambert grid), its own
properties (I symmetric under a swap of roles, frac = 1 under a global source), and the conditions the four mesh pairs must meet for
tests/test_mesh_conserve_gpu.py and tests/test_csr_rows_apply_gpu.py to reach what they are meant to reach."""
import numpy as np
import pytest

import _mesh_conserve_ref as MR
import _mesh_to_mesh_cases as MC
from _parity_helpers import assert_csr_equal, conserve_tol
from conftest import LAMBERT, mesh_xyz

GLOBAL_SOURCE = ("geo10_to_vor1500", "vor2500_to_hex", "varres3000_to_geo8")
# pair -> (entries, longest row, largest valence src / dst) of the reference: counts, so they are pinned exactly.  The covered share of a
# source cell was measured at most 1 + 2.4e-15 / 1.1e-15 / 1.4e-14 / 8.9e-15 on the four pairs (the issue's draft: 3e-15 / 2e-15 / 1e-14 /
# 2e-14); its bar is derived in test_input_conditions.
TABLE = {"geo10_to_vor1500": (5269, 7, 6, 8), "vor2500_to_hex": (1522, 3, 8, 6), "hex_to_geo10": (3046, 40, 6, 6),
         "varres3000_to_geo8": (5803, 97, 10, 6)}


def test_reference_against_the_oracle(oracle):
    """Destination polygons = the CORNER quads of a 31 x 21 Lambert grid of 120 km, source = the 2500-cell global Voronoi mesh:
    I_ref / area(g) is the oracle's conservative matrix as a set of entries, within the oracle's own bar for that grid."""
    from mpassit_amd import target_grid as tg
    g = tg.define_target_grid_params("lambert", 31, 21, dx=120000.0, dy=120000.0, **LAMBERT)
    m = MC.mesh("vor2500")
    _, vxyz = mesh_xyz(oracle, m)
    kxyz = oracle.lonlat_deg_to_xyz(g.lon_c, g.lat_c)
    orp, ocol, oval = oracle.conserve(m.verticesOnCell, vxyz, g.nx, g.ny, kxyz)[:3]
    dst, src = MR.polygons_of_grid(kxyz, g.nx, g.ny), MR.polygons_of_mesh(m.verticesOnCell, vxyz)
    area_g = np.abs(MR.fan_areas(*dst))
    d, s, inter = MR.intersections(dst, src)
    rp, col, val, frac = MR.rows(d, s, inter, area_g, MR.NORM_DSTAREA)
    tol = conserve_tol(oracle, g)
    common, only_o, only_r = assert_csr_equal(orp, ocol, oval, rp, col, val, m.nCells, tol=tol, sliver=MR.SLIVER)
    print("reference vs oracle: %d common entries, %d / %d on one side only, bar %.1e" % (common, only_o, only_r, tol))
    assert common > 1000
    assert np.abs(frac - 1.0).max() < tol, "a global mesh covers every grid cell"


@pytest.mark.parametrize("name", MR.PAIRS)
def test_reference_properties(oracle, name):
    a = MR.answer(oracle, name)
    # I(d, s) == I(s, d): the same region, the roles of subject and clip polygon swapped
    rng = np.random.default_rng(41)
    live = np.nonzero(a.inter > 0.0)[0]
    pick = rng.choice(live, size=min(300, live.size), replace=False)
    d, s = a.d[pick], a.s[pick]
    _, _, swapped = MR.intersections(a.ps, a.pd, pairs=(s, d))
    err = np.abs(swapped - a.inter[pick]) / (a.area_d[d] + a.area_s[s])
    print("%s: I under a swap of roles, %d pairs, worst %.1e of the two cells' areas, bar %.1e" % (name, pick.size, err.max(), a.tol))
    assert err.max() < a.tol
    frac = a.rows(MR.NORM_DSTAREA)[3]
    if name in GLOBAL_SOURCE:
        print("%s: |frac - 1| max %.1e" % (name, np.abs(frac - 1.0).max()))
        assert np.abs(frac - 1.0).max() < a.tol, "a global source covers every destination cell"


@pytest.mark.parametrize("name", MR.PAIRS)
def test_input_conditions(oracle, name):
    a = MR.answer(oracle, name)
    entries, longest, val_s, val_d = TABLE[name]
    rp, col, val, frac = a.rows(MR.NORM_DSTAREA)
    rows = np.diff(rp)
    cover_s = np.bincount(a.s, weights=a.inter, minlength=a.area_s.size) / a.area_s
    slivers = int((val < MR.SLIVER).sum()) + int((a.rows(MR.NORM_FRACAREA)[2] < MR.SLIVER).sum())
    print("%s: %d entries, a source cell covered at most 1 + %.1e, longest row %d, valence %d / %d, %d weights below %.0e" % (
        name, col.size, cover_s.max() - 1.0, rows.max(), a.ps[1].max(), a.pd[1].max(), slivers, MR.SLIVER))
    assert col.size == entries and rows.max() == longest and (a.ps[1].max(), a.pd[1].max()) == (val_s, val_d)
    # Two destination cells meet along a side that each of them walks in its own direction: the two clip planes are rounded apart by a few
    # eps radians, so the pieces of a source cell overlap (or gape) by a strip of that width along the side -- (eps x diameter) / area =
    # eps / h of the cell.  With the 64 of the project's conservative bar, and no floor: a source counted twice would show as 1e-3 or more.
    over = 64 * np.finfo(np.float64).eps / MR.thin(a.src.verticesOnCell, a.vs).min()
    print("%s: bar on the covered share of a source cell 1 + %.1e" % (name, over))
    assert cover_s.max() <= 1.0 + over, "no part of a source cell is counted twice"
    assert slivers <= MR.SLIVER_CAP * 2 * col.size, "the reference itself holds sliver-sized weights: change the seeds"
    assert a.dst.nCells % 64 != 0, "the last block of the rows Regrid is a partial one"
    if name == "hex_to_geo10":
        empty, full = int((rows == 0).sum()), int((np.abs(frac - 1.0) < a.tol).sum())
        partial = int(((frac > 1e-6) & (frac < 1.0 - 1e-6)).sum())
        print("hex_to_geo10: %d empty, %d partial, %d full rows" % (empty, partial, full))
        assert empty > 100 and partial > 10 and full > 10 and rows.max() > 24
    if name == "varres3000_to_geo8":
        assert rows.max() >= 64 and a.ps[1].max() == 10


@pytest.mark.parametrize("which", ["geo10", "vor1500"])
def test_identity_pair(oracle, which):
    """src == dst: the diagonal is 1, and what neighbours contribute stays below the 1e-14 rule in the reference (the GPU test does
    not require an exactly diagonal pattern: it allows one-sided entries below SLIVER)."""
    a = MR.answer(oracle, which + "_self")
    own = a.d == a.s
    w = a.inter / a.area_d[a.d]
    print("%s onto itself: diagonal within %.1e of 1, largest off-diagonal weight %.1e" % (which, np.abs(w[own] - 1.0).max(), w[~own].max()))
    assert own.sum() == a.dst.nCells and np.abs(w[own] - 1.0).max() < a.tol
    assert w[~own].max() < MR.SLIVER
    rp, col, val, frac = a.rows(MR.NORM_DSTAREA)
    assert np.array_equal(col, np.arange(a.dst.nCells)) and np.abs(frac - 1.0).max() < a.tol
