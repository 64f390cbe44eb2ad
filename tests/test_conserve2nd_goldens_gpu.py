"""The whole library path of second-order conservative regridding -- the first-order Store, mpg_handle_mask where the case is masked,
mpg_handle_conserve2nd -- against the 50-digit goldens of tests/golden/make_conserve2nd_goldens.py, NOT against the numpy mirror
(tests/test_conserve2nd_gpu.py holds the device to the mirror bit for bit; tests/test_conserve2nd_goldens.py holds the mirror to these
goldens on the CPU).  Every case's mesh or grid is rebuilt from the generator parameters the fixture records, and the regenerated float64
unit vectors are the stored ones bit for bit.

The comparison is of sparse matrices over the union of their entries, absolute, a missing entry counting as 0: the device's Store may
keep or drop a sliver pair that the reference pattern has the other way round, and such a pair carries a weight of rounding size.  The bar
is the CPU test's 1e-12 (its docstring derives it: the device has the mirror's bits on its own unit vectors, which differ from the stored
ones in last bits only, and the sensitivity measured there covers that).  Entries on one side only are each below the bar and number at
most 1 % of the golden's; mpg_handle_store_stats [2] and [3] are the golden's pass and fail counts.  The figures measured on an MI355X are
in profiles/r32_conserve2nd_goldens.md."""
import numpy as np
import pytest

import _conserve2nd_golden_cases as GC
from test_conserve2nd_goldens import BAR, CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return GC.load()


@pytest.fixture(scope="module")
def device(gpu_lib, golden, oracle):
    """The device object of a side of the fixture, made on first use from its generator parameters; all destroyed at the end."""
    from mpassit_amd import regrid as R
    doc, _ = golden
    made = {}

    def get(side):
        if side not in made:
            spec = doc["sides"][side]
            made[side] = R.Mesh.from_mpas(GC.mesh_of(spec)) if "mesh" in spec else R.Grid.from_target(GC.grid_of(spec))
        return made[side]

    yield get
    for x in made.values():
        x.destroy()


def _first_order(R, src, dst, norm):
    if isinstance(src, R.Mesh) and isinstance(dst, R.Grid):
        assert norm == GC.NORM_DSTAREA
        return R.regrid_store(src, dst, R.REGRIDMETHOD_CONSERVE)
    if isinstance(src, R.Grid):
        return R.regrid_store_conserve_to_mesh(src, dst, norm)
    return R.regrid_store_conserve_mesh(src, dst, norm)


@pytest.mark.parametrize("name", CASES)
def test_library_against_the_goldens(golden, device, oracle, name):
    from mpassit_amd import regrid as R
    doc, cases = golden
    c = cases[name]
    meta = c["meta"]
    for side, stored in ((meta["src_side"], c["src"]), (meta["dst_side"], c["dst"])):
        again = GC.side_arrays(oracle, doc["sides"][side])
        assert sorted(again) == sorted(stored)
        for k in again:
            assert np.array_equal(np.ascontiguousarray(again[k]).view(np.uint8), np.ascontiguousarray(stored[k]).view(np.uint8)), (side, k)
    src, dst = device(meta["src_side"]), device(meta["dst_side"])      # (Mesh.from_mpas takes cells listed clockwise: the reversed case runs)
    norm, sm = meta["norm"], c.get("src_mask")
    handles = [_first_order(R, src, dst, norm)]
    try:
        if meta["masked"]:
            handles.append(R.mask_handle(handles[0], src_mask=sm != 0, rule=R.MASKRULE_ENTRY, norm_type=norm))
        out = R.conserve_2nd(handles[-1], src, dst, norm, src_mask=None if sm is None else sm != 0)
        handles.append(out)
        got = out.csr()
        stats, shape = out.store_stats, (out.n_src, out.n_dst)
        first_nnz = handles[-2].nnz
    finally:
        for h in handles:
            h.release()
    worst, one_sided_worst, one_sided = GC.union_difference(got, (c["rowptr"], c["col"], c["val"]))
    print("%s: %d entries (golden %d), first-order pairs %d (reference %d), worst |device - golden| %.3g, %d entries on one side only "
          "(worst %.3g), bar %.0e" % (name, got[1].size, meta["nnz"], first_nnz, meta["nnz_in"], worst, one_sided, one_sided_worst, BAR))
    assert shape == (meta["n_src"], meta["n_dst"])
    assert worst <= BAR
    assert one_sided_worst < BAR and one_sided <= 0.01 * meta["nnz"]
    assert [stats[2], stats[3]] == meta["stats"][1:3], (stats[1:7], meta["stats"])
