"""The apply kernels held to the header's arithmetic, bit for bit: every comparison here is between a library call on the GPU and the exact
host restatement of include/mpassit_amd.h (tests/c/contract_ref.c through tests/_contract_ref.py), on integer views of the results --
equal bits, or NaN on both sides (payloads are not part of the contract).  No call is compared with another library call and there is no
tolerance, except the one derived bound for the pole-cap points of a periodic Grid -> Grid handle (test_pole_caps).

Handles (built once per module, all small): Mesh -> Grid bilinear (3 slots, unmapped rim), nearest (1 slot) and conservative (CSR) on the
regional case and on the tiny mesh under a 19 x 11 grid narrower than a 64-point tile; Grid -> Grid CENTER -> EDGE1 (4 slots); the periodic
72 x 36 grid CENTER -> EDGE2 (4 slots and pole caps); Grid -> Mesh bilinear (4 slots) and nearest from EDGE1, EDGE2 and CENTER of the 30-km
CONUS grid onto the cells and the edges of the global mesh (most points lie outside the grid); the periodic 72 x 36 grid onto that mesh's
cells and edges (CSR, rows of 72 entries beside rows of 4); and a from_weights CSR handle of 210 rows (_contract_ref.from_weights_case).

Levels 1, 2, 17 and 65, two fields.  Sources: ordinary N(280, 30) data and the same with about 1 % special values (NaN, infinities, -0.0,
subnormals of both types, values whose sums overflow or whose float32 cast does), each as float64 and as float32.  Epilogues (1, 0),
(9.81, -300) and (9.81, -2700): the last one is where a multiply-then-add epilogue shows in nearly every result (_contract_ref.recipe_shares).

The transpose (mpg_regrid_transpose_dev) on ten of those handles, on one from mpg_reconstruct_store, one from mpg_handle_compose and a
synthetic from_weights handle whose transposed segments bracket every kernel's thresholds (_contract_ref.synthetic_transpose_case), with
ordinary and special grid values (a NaN at destination point 0, the row the padded slots load), dense and pitched with NaN in the pad;
the rotation (mpg_rotate_winds_dev and mpg_rotate_winds) with cos(alpha) entries of 0.0 and -0.0; the Grid -> Grid wind chain
(mpg_wind_destagger_dev, _pitched_dev and the host mpg_wind_destagger) on mass grids of 19 x 11, 65 x 17 and 203 x 35 points.  Two derived
bounds besides test_pole_caps': the cap-row sources of the periodic handle's transpose (_transpose_ref.transpose_ref's), and the pole
rows of V in the wind chain on the periodic grid (test_pole_caps' own).  The only arithmetic the header does not pin, and so the only
values not held by bits here, are those two pole terms: the summation order of a cap's row mean and of the transpose's cap reduction.

Every input is a CUDA tensor: nothing goes through the host pipeline."""
import numpy as np
import pytest

import _contract_ref as cr
import _wind_reconstruct_helpers as H

pytestmark = pytest.mark.gpu

NLEVS = (1, 2, 17, 65)
NF = 2
A3 = (-1, -2, 0, 1, 2)           # "a3_staged": per handle, lane gather, the three staged shapes
LFV = (-1, 0, 1, 2)              # "lf_variant": per handle, row gather, staged level-fast, grid-row tiles
EPIS = ((1.0, 0.0), cr.EPI, cr.EPI_SHARP)
F64, F32 = np.float64, np.float32
TYPE_PAIRS = ((F64, F64), (F64, F32), (F32, F64), (F32, F32))
KINDS = ("ordinary", "special")
LAMBERT = dict(ref_lat=38.5, ref_lon=-97.5, truelat1=38.5, truelat2=38.5, stand_lon=-97.5)


class Case:
    def __init__(self):
        self.rh, self.pat, self.obj, self._src = {}, {}, [], {}

    def add(self, name, rh):
        self.rh[name], self.pat[name] = rh, cr.Pattern.of(rh)
        return rh

    def source(self, name, kind, nlev, sdt, seed=0):
        """{'np': (NF, nlev, n_src) of sdt on the host, 'cf': the same on the GPU, 'lf': (NF, n_src, nlev) on the GPU, 'where': {kind: mask}}"""
        import torch
        key = (name, kind, nlev, sdt, seed)
        if key not in self._src:
            pat = self.pat[name]
            if kind == "ordinary":
                x, where = cr.ordinary(pat.n_src, nlev, NF, seed), {}
            else:
                x, where = cr.special(pat, nlev, NF, seed, with_nan=kind != "special without NaN")
            x = cr.to_f32(x) if sdt == F32 else x
            if kind != "ordinary":      # every special source any test uses: each kind reaches an output of each field, >= 90 % finite
                kinds = [k for k, _ in cr.SPECIALS if kind == "special" or k != "nan"]
                cr.special_is_informative(pat, x, where, nlev, NF, kinds)
            cf = torch.from_numpy(x).cuda()
            self._src[key] = dict(np=x, cf=cf, lf=cf.transpose(1, 2).contiguous(), where=where)
        return self._src[key]

    def grid_values(self, name, kind, nlev, sdt):
        """grid values for the transpose of a handle: {'np': (NF, nlev, n_dst) of sdt, 'cf': the same on the GPU, 'pitched': a view
        (NF, nlev, ny_dst, nx_dst) of it whose planes lie a padded stride apart in a NaN-filled buffer}"""
        import torch
        key = (name, "g " + kind, nlev, sdt, 0)
        if key not in self._src:
            pat, rh = self.pat[name], self.rh[name]
            if kind == "ordinary":
                x = cr.ordinary(pat.n_dst, nlev, NF)
            else:
                x, where, pt = cr.special_g(pat, nlev, NF)
            x = cr.to_f32(x) if sdt == F32 else x
            if kind != "ordinary":      # every kind reaches an output of each field, >= 90 % of the referenced outputs finite
                cr.special_is_informative(pt, x, where, nlev, NF)
            cf = torch.from_numpy(x).cuda()
            ld = (pat.n_dst + 15) // 16 * 16 + 16
            buf = torch.full((NF * nlev * ld,), float("nan"), dtype=cf.dtype, device="cuda")
            view = buf.as_strided((NF, nlev, rh.ny_dst, rh.nx_dst), (nlev * ld, ld, rh.nx_dst, 1))
            view.copy_(cf.reshape(NF, nlev, rh.ny_dst, rh.nx_dst))
            self._src[key] = dict(np=x, cf=cf, pitched=view)
        return self._src[key]

    def drop_sources(self):
        self._src.clear()


@pytest.fixture(scope="module")
def case(gpu_lib, regional_case, global_mesh, conus_grid_30km):
    from mpassit_amd import regrid as R, synth, target_grid as T, workloads
    c = Case()
    m, g = regional_case
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
    c.add("m2g 3", R.regrid_store(mesh, grid, R.REGRIDMETHOD_BILINEAR))
    c.add("m2g 1", R.regrid_store(mesh, grid, R.REGRIDMETHOD_NEAREST_STOD))
    c.add("m2g csr", R.regrid_store(mesh, grid, R.REGRIDMETHOD_CONSERVE))
    c.add("g2g 4", R.regrid_store_grid(grid, R.STAGGERLOC_EDGE1))
    mt = workloads.workload("tiny")[0]
    gn = T.define_target_grid_params("lambert", 19, 11, dx=300000.0, dy=300000.0, **LAMBERT)
    mesh_t, grid_n = R.Mesh.from_mpas(mt), R.Grid.from_target(gn)
    c.add("narrow 3", R.regrid_store(mesh_t, grid_n, R.REGRIDMETHOD_BILINEAR))
    c.add("narrow 1", R.regrid_store(mesh_t, grid_n, R.REGRIDMETHOD_NEAREST_STOD))
    c.add("narrow csr", R.regrid_store(mesh_t, grid_n, R.REGRIDMETHOD_CONSERVE))
    gp = R.Grid.from_target(T.define_target_grid_params("lat-lon", nx=73, ny=37, stand_lon=0.0, is_regional=False))
    c.add("pole 4", R.regrid_store_grid(gp, R.STAGGERLOC_EDGE2))
    c.add("periodic E1", R.regrid_store_grid(gp, R.STAGGERLOC_EDGE1))
    gm = synth.mesh_edges(global_mesh)
    mesh_g, grid_c = R.Mesh.from_mpas(gm), R.Grid.from_target(conus_grid_30km)
    c.mesh_g, c.grid_c = mesh_g, grid_c
    for loc, lname in ((R.MESHLOC_ELEMENT, "cells"), (R.MESHLOC_EDGE, "edges")):
        for stag, sname in ((R.STAGGERLOC_EDGE1, "E1"), (R.STAGGERLOC_EDGE2, "E2"), (R.STAGGERLOC_CENTER, "C")):
            c.add("g2m 4 %s %s" % (sname, lname), R.regrid_store_to_mesh(grid_c, mesh_g, R.REGRIDMETHOD_BILINEAR, staggerloc=stag, meshloc=loc))
            c.add("g2m 1 %s %s" % (sname, lname), R.regrid_store_to_mesh(grid_c, mesh_g, R.REGRIDMETHOD_NEAREST_STOD, staggerloc=stag, meshloc=loc))
        c.add("p2m csr " + lname, R.regrid_store_periodic_to_mesh(gp, mesh_g, meshloc=loc, pole_method=R.POLEMETHOD_ALLAVG))
    (row, col, S), fw = cr.from_weights_case()
    c.add("fw csr", R.RouteHandle.from_weights(cr.FW_N_SRC, cr.FW_NX, cr.FW_NY, row, col, S))
    c.fw = fw
    (row, col, S), c.syn = cr.synthetic_transpose_case()
    c.add("syn csr", R.RouteHandle.from_weights(cr.SYN_N_SRC, cr.SYN_NX, cr.SYN_NY, row, col, S))
    mc = H.mesh_case(synth.icosahedral_mesh(3))
    rec = c.add("rec csr", R.reconstruct_store(mc["n_on"], mc["eoc"], mc["m"].nEdges))
    rng = np.random.default_rng(31)            # 300 points that each take one cell of their own, with a weight: 300 rows of that cell's edges
    c.pick_i = R.RouteHandle.from_weights(rec.n_dst, 300, 1, np.arange(1, 301, dtype=np.int32), (rng.permutation(rec.n_dst)[:300] + 1).astype(np.int32),
                                          rng.uniform(0.5, 1.5, 300))
    c.add("comp csr", R.compose(c.pick_i, rec))
    c.obj = [mesh, grid, mesh_t, grid_n, gp, mesh_g, grid_c]
    yield c
    c.drop_sources()
    for rh in list(c.rh.values()) + [c.pick_i]:
        rh.release()
    for o in c.obj:
        o.destroy()


@pytest.fixture(autouse=True)
def _knobs_back(gpu_lib):
    try:
        yield
    finally:
        gpu_lib.tune("a3_staged", -1)
        gpu_lib.tune("lf_variant", -1)


# ---- comparison ---------------------------------------------------------------------------------------------------------------------
def held(got, want, what):
    """the GPU result `got` has the bits of the host array `want`, or both are NaN"""
    import torch
    w = torch.from_numpy(np.ascontiguousarray(want)).cuda()
    g = got.contiguous().reshape(w.shape)
    assert g.dtype == w.dtype, (what, g.dtype, w.dtype)
    it = torch.int64 if g.dtype == torch.float64 else torch.int32
    bad = (g.view(it) != w.view(it)) & ~(torch.isnan(g) & torch.isnan(w))
    if bool(bad.any()):
        first = tuple(torch.nonzero(bad)[0].tolist())
        raise AssertionError("%s: %d of %d outputs differ from the contract; the first at %s: got %r (%#x), contract %r (%#x)" % (
            what, int(bad.sum()), bad.numel(), first, float(g[first]), int(g.view(it)[first]), float(w[first]), int(w.view(it)[first])))


def tdt(dt):
    import torch
    return torch.float32 if dt == F32 else torch.float64


def layouts(R, s):
    return ((R.LAYOUT_CELL_FAST, False, s["cf"]), (R.LAYOUT_LEV_FAST, True, s["lf"]))


# ---- the handles and the inputs --------------------------------------------------------------------------------------------------------
def test_the_handles_exercise_what_they_should(case):
    p = case.pat
    assert p["m2g 3"].nnz == 3 and p["m2g 3"].unmapped.any() and not p["m2g 3"].unmapped.all() and p["m2g 1"].nnz == 1 and p["m2g csr"].nnz == 0
    assert case.rh["narrow 3"].nx_dst < 64 and p["narrow 3"].nnz == 3 and p["narrow csr"].nnz == 0
    assert p["g2g 4"].nnz == 4 and p["g2g 4"].pole is None
    assert p["pole 4"].nnz == 4 and p["pole 4"].pole is not None and p["pole 4"].pole[3] == 72 and (p["pole 4"].pole[2] != 0).sum() > 0
    for loc, n in (("cells", 20000), ("edges", 59994)):
        for st in ("E1", "E2", "C"):
            p4, p1 = p["g2m 4 %s %s" % (st, loc)], p["g2m 1 %s %s" % (st, loc)]
            assert p4.nnz == 4 and p1.nnz == 1 and p4.n_dst == p1.n_dst == n and n % 64 != 0
            assert p4.unmapped.mean() > 0.5 and not p4.unmapped.all(), "most points lie outside the grid"
        lens = np.diff(p["p2m csr " + loc].rowptr)
        assert set(np.unique(lens)) == {4, 72}
    assert p["fw csr"].nnz == 0
    for name, saved in cr.golden_patterns().items():          # what test_contract_ref.py checks on the CPU is what the Stores give
        live = p[name]
        assert (saved.n_src, saved.n_dst, saved.nnz) == (live.n_src, live.n_dst, live.nnz), name
        for attr in (("idx", "w") if live.nnz else ("rowptr", "col", "val")):
            assert np.array_equal(getattr(saved, attr), getattr(live, attr)), (name, attr)
    for a, b in zip((p["fw csr"].rowptr, p["fw csr"].col, p["fw csr"].val), (case.fw.rowptr, case.fw.col, case.fw.val)):
        assert np.array_equal(a, b), "from_weights keeps the stored order"


SHARE_HANDLES = ("m2g 3", "m2g 1", "m2g csr", "narrow 3", "narrow csr", "g2g 4", "pole 4", "g2m 4 C cells", "g2m 4 E1 edges", "g2m 1 C cells",
                 "p2m csr cells", "p2m csr edges", "fw csr")


@pytest.mark.parametrize("name", SHARE_HANDLES)
def test_the_inputs_can_tell_the_difference(case, name):
    """Reference against reference, on the pattern of the Store itself and the ordinary float64 source of 17 levels: every wrong recipe
    that can differ on this kind of pattern differs on at least 1 % of the mapped outputs (the all -0.0 input of the skipped epilogue: on
    every qualifying point).  The special sources are checked where they are made (Case.source: every kind reaches an output of every
    field, at least 90 % of the mapped outputs finite); here they are made for every level count and both types."""
    pat = case.pat[name]
    shares = cr.recipe_shares(pat, case.source(name, "ordinary", 17, F64)["np"], 17, NF)
    for k, v in shares.items():
        print("%-16s %-62s %6.2f %%" % (name, k, 100.0 * v))
    low = {k: v for k, v in shares.items() if not k.endswith("[info]") and v < 0.01}
    assert not low, (name, low)
    assert shares.get("epilogue skipped at (1, 0)", 1.0) == 1.0
    for nlev in NLEVS:
        for sdt in (F64, F32):
            assert len(case.source(name, "special", nlev, sdt)["where"]) == len(cr.SPECIALS)


# ---- mpg_regrid_dev: the float64 entry, no epilogue ---------------------------------------------------------------------------------------
F64_ENTRY = ("m2g 3", "m2g 1", "m2g csr", "narrow 3", "narrow 1", "narrow csr", "g2g 4", "g2m 4 C cells", "g2m 1 C cells", "p2m csr cells", "fw csr")


@pytest.mark.parametrize("name", F64_ENTRY)
def test_regrid_float64_entry(gpu_lib, case, name):
    import torch
    from mpassit_amd import regrid as R
    rh, pat = case.rh[name], case.pat[name]
    knobs = [(a, l) for a in A3 for l in LFV] if pat.nnz == 3 else [(-1, -1)]
    for nlev in NLEVS:
        for kind in KINDS:
            s = case.source(name, kind, nlev, F64)
            want = cr.apply(pat, s["np"], nlev, NF, epilogue=False)
            for a3, lfv in knobs:
                gpu_lib.tune("a3_staged", a3)
                gpu_lib.tune("lf_variant", lfv)
                for layout, _, src in layouts(R, s):
                    held(rh.regrid(src.view(-1), nlev=nlev, nfields=NF, layout=layout), want, (name, "regrid", nlev, kind, a3, lfv, layout))
            gpu_lib.tune("a3_staged", -1)
            gpu_lib.tune("lf_variant", -1)
            for layout, _, src in layouts(R, s):
                out = rh.empty_pitched(nlev, NF, torch.float64)
                rh.regrid(src.view(-1), nlev=nlev, nfields=NF, layout=layout, out=out)
                held(out, want, (name, "regrid pitched", nlev, kind, layout))


# ---- mpg_regrid_typed_pitched_dev ------------------------------------------------------------------------------------------------------
TYPED = ("m2g 3", "m2g 1", "m2g csr", "narrow 3", "narrow 1", "narrow csr", "g2g 4", "g2m 4 C cells", "p2m csr cells", "fw csr")


@pytest.mark.parametrize("name", TYPED)
def test_regrid_typed(gpu_lib, case, name):
    from mpassit_amd import regrid as R
    rh, pat = case.rh[name], case.pat[name]
    for nlev in NLEVS:
        for kind in KINDS:
            for sdt, ddt in TYPE_PAIRS:
                s = case.source(name, kind, nlev, sdt)
                for scale, offset in EPIS:
                    want = cr.apply(pat, s["np"], nlev, NF, dst_dtype=ddt, scale=scale, offset=offset)
                    for layout, _, src in layouts(R, s):
                        got = rh.regrid_typed(src.view(-1), nlev=nlev, nfields=NF, layout=layout, out_dtype=tdt(ddt), scale=scale, offset=offset)
                        held(got, want, (name, "typed", nlev, kind, sdt, ddt, scale, offset, layout))
                        out = rh.empty_pitched(nlev, NF, tdt(ddt))
                        rh.regrid_typed(src.view(-1), nlev=nlev, nfields=NF, layout=layout, scale=scale, offset=offset, out=out)
                        held(out, want, (name, "typed pitched", nlev, kind, sdt, ddt, scale, offset, layout))


@pytest.mark.parametrize("name", ("m2g 3", "narrow 3"))
def test_regrid_typed_three_slot_kernels(gpu_lib, case, name):
    """every a3_staged and lf_variant setting serves the 3-slot handle with the same bits: the contract's"""
    from mpassit_amd import regrid as R
    rh, pat = case.rh[name], case.pat[name]
    for nlev in NLEVS:
        for kind, sdt, ddt, (scale, offset) in (("ordinary", F32, F32, cr.EPI), ("special", F64, F64, (1.0, 0.0)), ("special", F64, F32, cr.EPI_SHARP),
                                                ("ordinary", F32, F64, cr.EPI_SHARP)):
            s = case.source(name, kind, nlev, sdt)
            want = cr.apply(pat, s["np"], nlev, NF, dst_dtype=ddt, scale=scale, offset=offset)
            for a3 in A3:
                gpu_lib.tune("a3_staged", a3)
                for lfv in LFV:
                    gpu_lib.tune("lf_variant", lfv)
                    for layout, _, src in layouts(R, s):
                        got = rh.regrid_typed(src.view(-1), nlev=nlev, nfields=NF, layout=layout, out_dtype=tdt(ddt), scale=scale, offset=offset)
                        held(got, want, (name, "typed", nlev, kind, a3, lfv, layout))


@pytest.mark.parametrize("name", ("m2g 3", "g2g 4"))
def test_regrid_typed_big_endian(case, name):
    """a big-endian side is the little-endian result with its bytes reversed"""
    import torch
    from mpassit_amd import regrid as R
    rh, pat = case.rh[name], case.pat[name]
    for nlev in NLEVS:
        for kind in KINDS:
            for (sdt, ddt), (scale, offset) in ((tp, e) for tp in TYPE_PAIRS for e in EPIS):
                s = case.source(name, kind, nlev, sdt)
                want = cr.apply(pat, s["np"], nlev, NF, dst_dtype=ddt, scale=scale, offset=offset)
                be_cf = torch.from_numpy(cr.swap(s["np"])).cuda()
                for layout, src, src_be in ((R.LAYOUT_CELL_FAST, be_cf, True), (R.LAYOUT_LEV_FAST, be_cf.transpose(1, 2).contiguous(), True),
                                            (R.LAYOUT_CELL_FAST, s["cf"], False)):
                    for dst_be in (False, True):
                        got = rh.regrid_typed(src.view(-1), nlev=nlev, nfields=NF, layout=layout, out_dtype=tdt(ddt), scale=scale, offset=offset,
                                              src_be=src_be, dst_be=dst_be)
                        it = torch.int64 if ddt == F64 else torch.int32
                        w = cr.swap(want) if dst_be else want
                        same = torch.equal(got.contiguous().view(it).reshape(-1), torch.from_numpy(cr.bits(w).reshape(-1)).cuda())
                        if not same:   # NaN payloads are free: compare the values after swapping back
                            back = torch.from_numpy(cr.swap(got.cpu().numpy())).cuda() if dst_be else got
                            held(back, want, (name, "typed BE", nlev, kind, sdt, ddt, scale, layout, src_be, dst_be))


@pytest.mark.parametrize("name", ("m2g 3", "m2g csr"))
def test_regrid_bundle_per_field_offsets(case, name):
    from mpassit_amd import regrid as R
    rh, pat = case.rh[name], case.pat[name]
    offsets = [-300.0, 7.5]
    for nlev in NLEVS:
        for kind in KINDS:
            for sdt, ddt in TYPE_PAIRS:
                s = case.source(name, kind, nlev, sdt)
                want = cr.apply(pat, s["np"], nlev, NF, dst_dtype=ddt, scale=9.81, offset=offsets)
                for layout, _, src in layouts(R, s):
                    outs = rh.regrid_bundle([src[f].contiguous().view(-1) for f in range(NF)], nlev=nlev, layout=layout, out_dtype=tdt(ddt), scale=9.81,
                                            offsets=offsets)
                    for f in range(NF):
                        held(outs[f], want[f], (name, "bundle", nlev, kind, sdt, ddt, layout, f))


# ---- pole caps -------------------------------------------------------------------------------------------------------------------------
def test_pole_caps(case):
    """The periodic 72 x 36 grid, CENTER -> EDGE2.  Points outside the caps: identity with the 4-slot chain.  A cap point is
    fma(wp, m, acc4) then the epilogue, m the mean of its CENTER row -- whose summation order the header does not promise, so it is held to
    a bound, with m computed exactly (math.fsum / row_len):
        |got - want| <= (row_len + 3) * 2^-53 * |wp| * mean(|x_row|) * |scale|  +  one unit in the last place of `want` in the destination type
    (any order of row_len - 1 additions and one division stays within (row_len + 1) * 2^-53 * mean|x| of the exact mean; the product with
    wp and the accumulate round once more each; the cast of a value that close to `want` lands on `want` or a neighbour).  A cap point
    whose row holds a NaN, or infinities of both signs, must be NaN; where `want` is not finite the bits must agree.  One exemption: a
    (field, level) row whose sum of absolute values is beyond the largest float64 -- two values near 1.7e308 in one row of 72 -- can
    overflow in one summation order and not in another, and its cap points are left free; a row with one such value cannot, and is held
    to the bound.  The test counts both kinds and requires rows with a 1.7e308 among the checked ones."""
    import torch
    from mpassit_amd import regrid as R
    rh, pat = case.rh["pole 4"], case.pat["pole 4"]
    n_checked = n_free = n_huge = 0
    for nlev in NLEVS:
        for kind in KINDS:
            for sdt, ddt in TYPE_PAIRS:
                s = case.source("pole 4", kind, nlev, sdt)
                calls = [(None, ddt)] if (sdt, ddt) == (F64, F64) else []
                calls += [(e, ddt) for e in EPIS]
                for epi, dt in calls:
                    scale, offset = epi or (1.0, 0.0)
                    plain = cr.apply(pat, s["np"], nlev, NF, dst_dtype=dt, epilogue=epi is not None, scale=scale, offset=offset)
                    pts, want, bound, must_nan, free = cr.pole_caps(pat, s["np"], nlev, NF, False, dt, epi is not None, scale, offset)
                    other = np.ones(pat.n_dst, bool)
                    other[pts] = False
                    for layout, _, src in layouts(R, s):
                        if epi is None:
                            got = rh.regrid(src.view(-1), nlev=nlev, nfields=NF, layout=layout)
                        else:
                            got = rh.regrid_typed(src.view(-1), nlev=nlev, nfields=NF, layout=layout, out_dtype=tdt(dt), scale=scale, offset=offset)
                        got = got.reshape(NF, nlev, -1)
                        what = ("pole", nlev, kind, sdt, dt, epi, layout)
                        held(got[:, :, torch.from_numpy(other).cuda()], plain[:, :, other], what)
                        g = got[:, :, torch.from_numpy(pts.astype(np.int64)).cuda()].cpu().numpy()
                        with np.errstate(invalid="ignore", over="ignore"):
                            w = want.astype(dt)
                            exact = ~np.isfinite(w) & ~must_nan & ~free
                            tol = bound + np.spacing(np.abs(w)).astype(F64)
                            ok = np.where(must_nan, np.isnan(g), np.where(exact, ~cr.differs(g, w), free | (np.abs(g.astype(F64) - w.astype(F64)) <= tol)))
                        assert ok.all(), (what, "cap points", int((~ok).sum()), g[~ok][:3], w[~ok][:3], tol[~ok][:3])
                        n_checked += int((~free).sum())
                        n_free += int(free.sum())
                        with np.errstate(invalid="ignore"):
                            n_huge += int((~free & ~must_nan & np.isfinite(bound) & (bound > 1e280)).sum())
    print("pole caps: %d cap outputs held, %d of them on a row with a value near 1.7e308, %d left free" % (n_checked, n_huge, n_free))
    assert n_checked > 1000 and n_huge > 0 and n_free < 0.01 * n_checked


# ---- mesh order: mpg_regrid_to_mesh_dev, mpg_regrid_csr_to_mesh_dev -----------------------------------------------------------------------
def _pitched_source(torch, s, nlev, n_src):
    """the source as a plane-pitched view (NF, nlev, 1, n_src) over a NaN-filled buffer"""
    ld = (n_src + 15) // 16 * 16 + 16
    buf = torch.full((NF * nlev * ld,), float("nan"), dtype=s.dtype, device="cuda")
    view = buf.as_strided((NF, nlev, 1, n_src), (nlev * ld, ld, n_src, 1))
    view.copy_(s.reshape(NF, nlev, 1, n_src))
    return view


def _mesh_order(case, name, nlevs, kinds, pairs, epis):
    import torch
    from mpassit_amd import regrid as R
    rh, pat = case.rh[name], case.pat[name]
    call = rh.regrid_csr_to_mesh if pat.nnz == 0 else rh.regrid_to_mesh
    for nlev in nlevs:
        for kind in kinds:
            for sdt, ddt in pairs:
                s = case.source(name, kind, nlev, sdt)
                for scale, offset in epis:
                    for layout, lev_fast in ((R.LAYOUT_CELL_FAST, False), (R.LAYOUT_LEV_FAST, True)):
                        want = cr.apply(pat, s["np"], nlev, NF, dst_dtype=ddt, dst_lev_fast=lev_fast, scale=scale, offset=offset)
                        got = call(s["cf"], nlev=nlev, nfields=NF, layout=layout, out_dtype=tdt(ddt), scale=scale, offset=offset)
                        held(got, want, (name, "to_mesh", nlev, kind, sdt, ddt, scale, offset, layout))
                        if nlev in (2, 17):
                            got = call(_pitched_source(torch, s["cf"], nlev, pat.n_src), nlev=nlev, nfields=NF, layout=layout, out_dtype=tdt(ddt),
                                       scale=scale, offset=offset)
                            held(got, want, (name, "to_mesh, pitched source", nlev, kind, sdt, ddt, scale, offset, layout))


@pytest.mark.parametrize("name", ("g2m 4 C cells", "g2m 1 C cells", "g2m 4 E2 cells", "p2m csr cells", "fw csr"))
def test_regrid_to_mesh(case, name):
    _mesh_order(case, name, NLEVS, KINDS, TYPE_PAIRS, EPIS)


@pytest.mark.parametrize("name", ("g2m 4 E1 edges", "g2m 1 E2 edges", "p2m csr edges"))
def test_regrid_to_mesh_edges(case, name):
    """The same kernels onto the 59 994 edges.  Trimmed for run time (a reference over 59 994 points x 65 levels x 2 fields is 8 M
    outputs): special sources, the two unmixed type pairs, the (9.81, -300) epilogue, 2 and 65 levels.  The full cross product runs on the
    20 000 cells in test_regrid_to_mesh."""
    _mesh_order(case, name, (2, 65), ("special",), ((F64, F64), (F32, F32)), (cr.EPI,))


# ---- rows to rows: mpg_regrid_rows_dev, mpg_regrid_csr_rows_dev -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("m2g 3", "g2g 4", "m2g 1", "narrow 3", "m2g csr", "p2m csr cells", "fw csr"))
def test_regrid_rows(case, name):
    rh, pat = case.rh[name], case.pat[name]
    call = rh.regrid_csr_rows if pat.nnz == 0 else rh.regrid_rows
    for nlev in NLEVS:
        for kind in KINDS:
            for sdt, ddt in TYPE_PAIRS:
                s = case.source(name, kind, nlev, sdt)
                for scale, offset in EPIS:
                    want = cr.apply(pat, s["np"], nlev, NF, dst_dtype=ddt, dst_lev_fast=True, scale=scale, offset=offset)
                    got = call(s["lf"], nlev=nlev, nfields=NF, out_dtype=tdt(ddt), scale=scale, offset=offset)
                    held(got, want, (name, "rows", nlev, kind, sdt, ddt, scale, offset))


# ---- mpg_regrid_masked_dev ---------------------------------------------------------------------------------------------------------------
MISSING = -9999.0


def _holes(case, name, nlev, sdt):
    """the ordinary source with 10 % NaN and 3 % MISSING (a value float32 holds exactly), and a static mask over 10 % of the sources"""
    import torch
    key = (name, "holes", nlev, sdt, 0)
    if key not in case._src:
        pat = case.pat[name]
        x = cr.ordinary(pat.n_src, nlev, NF).copy()
        rng = np.random.default_rng(99 + nlev)
        r = rng.random(x.shape)
        x[r < 0.10] = np.nan
        x[(r >= 0.10) & (r < 0.13)] = MISSING
        x = cr.to_f32(x) if sdt == F32 else x
        cf = torch.from_numpy(x).cuda()
        mask = (np.random.default_rng(5).random(pat.n_src) < 0.10).astype(np.uint8)
        case._src[key] = dict(np=x, cf=cf, lf=cf.transpose(1, 2).contiguous(), mask=mask, mask_dev=torch.from_numpy(mask).cuda())
    return case._src[key]


@pytest.mark.parametrize("name", ("m2g 3", "m2g 1", "g2g 4", "m2g csr", "narrow 3", "fw csr"))
def test_regrid_masked(case, name):
    """"defined" is decided by identity too: Wt and Wv are exact restatements, so no output is left out as an edge case.  Inf is not
    missing: the special set without NaN, with no missing rule at all, must match as well."""
    from mpassit_amd import regrid as R
    rh, pat = case.rh[name], case.pat[name]
    nan = float("nan")
    # (source, missing=, flags, static mask, fill, epilogue)
    configs = (("holes", "nan", 1, False, nan, (1.0, 0.0)), ("holes", ("nan", MISSING), 3, True, -7777.0, cr.EPI), ("holes", MISSING, 2, False, nan, cr.EPI_SHARP),
               ("special", "nan", 1, True, -7777.0, cr.EPI), ("special without NaN", None, 0, False, nan, (1.0, 0.0)))
    for nlev in NLEVS:
        for sdt, ddt in TYPE_PAIRS:
            for srcname, missing, flags, use_mask, fill, (scale, offset) in configs:
                h = _holes(case, name, nlev, sdt)
                s = h if srcname == "holes" else case.source(name, srcname, nlev, sdt)
                for frac in (0.0, 0.5, 1.0):
                    want = cr.apply_masked(pat, s["np"], nlev, NF, dst_dtype=ddt, flags=flags, missing_value=MISSING, src_mask=h["mask"] if use_mask else None,
                                           min_valid_frac=frac, fill_value=fill, scale=scale, offset=offset)
                    for layout, _, src in layouts(R, s):
                        got = rh.regrid_masked(src.view(-1), nlev=nlev, nfields=NF, layout=layout, missing=missing, src_mask=h["mask_dev"] if use_mask else None,
                                               min_valid_frac=frac, fill_value=fill, out_dtype=tdt(ddt), scale=scale, offset=offset)
                        held(got, want, (name, "masked", nlev, sdt, ddt, srcname, missing, use_mask, frac, fill, scale, layout))


# ---- winds -------------------------------------------------------------------------------------------------------------------------------
def _winds(case, mode, name_u, name_v, call, c, s, nlevs, kinds, tangentials=(True,)):
    """mode "mesh" / "edges"; c, s: CUDA angle tensors (or None, mesh mode), copied to the host as inputs of the restatement"""
    from mpassit_amd import regrid as R
    rh_u, rh_v, pu, pv = case.rh[name_u], case.rh[name_v], case.pat[name_u], case.pat[name_v]
    ch, sh = (None, None) if c is None else (c.cpu().numpy(), s.cpu().numpy())
    for nlev in nlevs:
        for kind in kinds:
            for sdt, ddt in TYPE_PAIRS:
                su, sv = case.source(name_u, kind, nlev, sdt), case.source(name_v, kind, nlev, sdt, seed=1)
                u, v = su["cf"][0].contiguous(), sv["cf"][1].contiguous()
                for layout, lev_fast in ((R.LAYOUT_CELL_FAST, False), (R.LAYOUT_LEV_FAST, True)):
                    want = cr.wind_pair(mode, pu, pv, su["np"][0], sv["np"][1], ch, sh, nlev, ddt, lev_fast)
                    for tan in tangentials:
                        if mode == "mesh":
                            got = call(rh_u, rh_v, c, s, u, v, nlev, layout=layout, out_dtype=tdt(ddt))
                        else:
                            got = call(rh_u, rh_v, c, s, u, v, nlev, layout=layout, out_dtype=tdt(ddt), tangential=tan)
                            got = got if tan else (got,)
                        for i, g in enumerate(got):
                            held(g, want[i], (mode, name_u, name_v, nlev, kind, sdt, ddt, layout, tan, i, c is not None))


@pytest.mark.parametrize("nnz", (4, 1))
@pytest.mark.parametrize("angles", (True, False))
def test_wind_to_mesh(case, nnz, angles):
    from mpassit_amd import regrid as R
    c, s = R.mesh_rotang(case.grid_c, case.mesh_g) if angles else (None, None)
    _winds(case, "mesh", "g2m %d E1 cells" % nnz, "g2m %d E2 cells" % nnz, R.wind_to_mesh, c, s, NLEVS, KINDS)


@pytest.mark.parametrize("nnz", (4, 1))
def test_wind_to_edges(case, nnz):
    """Trimmed for run time on 59 994 edges: special sources at 1, 2 and 17 levels, ordinary ones at 65; every type pair, both orders and
    tangential on and off in both.  wind_to_mesh runs the full cross product on the cells with the same kernel family."""
    from mpassit_amd import regrid as R
    c, s = R.mesh_edge_rotang(case.grid_c, case.mesh_g)
    _winds(case, "edges", "g2m %d E1 edges" % nnz, "g2m %d E2 edges" % nnz, R.wind_to_edges, c, s, (1, 2, 17), ("special",), (True, False))
    _winds(case, "edges", "g2m %d E1 edges" % nnz, "g2m %d E2 edges" % nnz, R.wind_to_edges, c, s, (65,), ("ordinary",), (True, False))


@pytest.fixture(scope="module")
def twins(case):
    """the periodic CSR handles a second time, as handles of their own with the same stored pattern"""
    from mpassit_amd import regrid as R
    out = {}
    for loc in ("cells", "edges"):
        rh = case.rh["p2m csr " + loc]
        row, col, S = rh.to_esmf_weights()
        name = "p2m csr %s twin" % loc
        out[loc] = case.add(name, R.RouteHandle.from_weights(rh.n_src, rh.n_dst, 1, row, col, S))
        a, b = case.pat[name], case.pat["p2m csr " + loc]
        assert out[loc]._h.value != rh._h.value and np.array_equal(a.rowptr, b.rowptr) and np.array_equal(a.col, b.col) and np.array_equal(a.val, b.val)
    return out


@pytest.mark.parametrize("twice", (False, True))
def test_wind_csr_to_mesh(case, twins, twice):
    from mpassit_amd import regrid as R
    name_v = "p2m csr cells twin" if twice else "p2m csr cells"
    c, s = R.mesh_rotang(case.grid_c, case.mesh_g)          # angles are inputs here: any [n_dst] pair serves
    _winds(case, "mesh", "p2m csr cells", name_v, R.wind_csr_to_mesh, c, s, NLEVS, KINDS)
    _winds(case, "mesh", "p2m csr cells", name_v, R.wind_csr_to_mesh, None, None, (2, 17), ("special",))


@pytest.mark.parametrize("twice", (False, True))
def test_wind_csr_to_edges(case, twins, twice):
    """trimmed as test_wind_to_edges is, for the same reason; wind_csr_to_mesh runs the full cross product on the cells"""
    from mpassit_amd import regrid as R
    name_v = "p2m csr edges twin" if twice else "p2m csr edges"
    c, s = R.mesh_edge_rotang(None, case.mesh_g)
    _winds(case, "edges", "p2m csr edges", name_v, R.wind_csr_to_edges, c, s, (1, 2, 17), ("special",), (True, False))
    _winds(case, "edges", "p2m csr edges", name_v, R.wind_csr_to_edges, c, s, (65,), ("ordinary",), (True, False))


# ---- the transpose: mpg_regrid_transpose_dev ---------------------------------------------------------------------------------------------
TRANSPOSED = ("m2g 3", "m2g 1", "m2g csr", "g2g 4", "narrow 3", "fw csr", "g2m 4 C cells", "p2m csr cells", "rec csr", "comp csr", "syn csr")


def test_the_transposed_handles_exercise_what_they_should(case):
    """on the host, before anything is launched: the synthetic handle's segments bracket TR_SHORT = 16, the 4-slot form and a wave"""
    p = case.pat
    lens = cr.segment_lengths(p["syn csr"])
    assert set(cr.SYN_LENGTHS) <= set(lens.tolist()) and lens.max() == 300 and p["syn csr"].n_src % 64 != 0 and p["syn csr"].nnz == 0
    for a, b in zip((p["syn csr"].rowptr, p["syn csr"].col, p["syn csr"].val), (case.syn.rowptr, case.syn.col, case.syn.val)):
        assert np.array_equal(a, b), "from_weights keeps the stored order"
    assert cr.segment_lengths(p["p2m csr cells"]).max() > 16 and cr.segment_lengths(p["m2g 1"]).max() >= 1
    assert p["rec csr"].nnz == 0 and (p["rec csr"].val == 1.0).all() and p["rec csr"].n_src == 1920 and p["rec csr"].n_dst == 642
    assert p["comp csr"].nnz == 0 and p["comp csr"].n_src == 1920 and p["comp csr"].n_dst == 300 and (p["comp csr"].val != 1.0).all()
    for name in TRANSPOSED:
        n = cr.segment_lengths(p[name])
        print("%-16s %6d sources, %6d referenced, segments up to %4d, %5d beyond 16, %6d of at most 4" % (
            name, p[name].n_src, int((n > 0).sum()), int(n.max()), int((n > 16).sum()), int(((n > 0) & (n <= 4)).sum())))
        assert p[name].pole is None


@pytest.mark.parametrize("name", TRANSPOSED)
def test_transpose_inputs_can_tell_the_difference(case, name):
    """reference against reference on the ordinary grid values of 17 levels: a reversed segment and a separate multiply and add each
    change at least 1 % of the outputs they can change at all (_contract_ref.transpose_shares); the special grid values are checked
    where they are made (Case.grid_values), here for every level count and both types"""
    pat = case.pat[name]
    shares = cr.transpose_shares(pat, case.grid_values(name, "ordinary", 17, F64)["np"], 17, NF)
    for k, v in shares.items():
        print("%-16s transpose: %-40s %6.2f %%" % (name, k, 100.0 * v))
    low = {k: v for k, v in shares.items() if v < 0.01}
    assert not low, (name, low)
    if name == "syn csr":
        assert set(shares) == {"segment reversed", "separate multiply and add"}
    for nlev in NLEVS:
        for sdt in (F64, F32):
            assert np.isnan(case.grid_values(name, "special", nlev, sdt)["np"][:, :, 0]).all()


def _transposes(R, rh, s, nlev, ddt):
    """every way to the same result: both layouts, dense and pitched grid values; yields (what, result as (NF, nlev, n_src))"""
    for lname, layout in (("[lev][cell]", R.LAYOUT_CELL_FAST), ("[cell][lev]", R.LAYOUT_LEV_FAST)):
        for sname, src in (("dense", s["cf"]), ("pitched", s["pitched"])):
            got = rh.regrid_transpose(src, nlev=nlev, nfields=NF, layout=layout, out_dtype=tdt(ddt))
            yield (lname, sname), got if layout == R.LAYOUT_CELL_FAST else got.transpose(1, 2)


@pytest.mark.parametrize("name", TRANSPOSED)
def test_regrid_transpose(case, name):
    """acc = fma(w_j, (double)g[k][row_j], acc) from +0.0 in ascending (destination point, slot) order, (dst type)acc, +0.0 for a source
    nothing references: the bits of cr_apply_transpose on every source, level, field, type pair, layout and pitch"""
    from mpassit_amd import regrid as R
    rh, pat = case.rh[name], case.pat[name]
    unref = cr.segment_lengths(pat) == 0
    for nlev in NLEVS:
        for kind in KINDS:
            for sdt in (F64, F32):
                s = case.grid_values(name, kind, nlev, sdt)
                want64, cap = cr.transpose(pat, s["np"], nlev, NF)
                assert not cap.any() and (cr.bits(want64[:, :, unref]) == 0).all()
                for ddt in (F64, F32):
                    with np.errstate(over="ignore"):
                        want = want64.astype(ddt)                         # one rounding at the store
                    for how, got in _transposes(R, rh, s, nlev, ddt):
                        held(got, want, (name, "transpose", nlev, kind, sdt, ddt) + how)


def test_regrid_transpose_pole_caps(case):
    """The periodic 72 x 36 grid, CENTER -> EDGE2.  Off the two CENTER rows under the caps: the bits of the restatement.  On them the
    kernel adds its cap term last, a reduction whose order the header states but the restatement does not follow: those 2 * row_len
    sources -- counted, and no more -- are held to _transpose_ref.transpose_ref's derived bound on the ordinary grid values.  On the
    special ones a cap-row source is held where its bound is finite; where a NaN or infinities of both signs enter its terms it must
    be NaN; infinities of one sign alone: that infinity; the rest (finite terms whose bound is beyond the largest float64: one order
    can overflow where another does not) is left free and counted."""
    from _transpose_ref import EPS, transpose_ref
    from mpassit_amd import regrid as R
    rh, pat = case.rh["pole 4"], case.pat["pole 4"]
    dst, src0, wp, row_len = pat.pole
    n_held = n_free = n_forced = 0
    for nlev in NLEVS:
        for kind in KINDS:
            for sdt in (F64, F32):
                key = ("pole 4", "g " + kind, nlev, sdt, 0)
                s = case.grid_values("pole 4", kind, nlev, sdt)
                g = s["np"].astype(F64)
                want64, cap = cr.transpose(pat, s["np"], nlev, NF)
                assert int(cap.sum()) == 2 * row_len == 144 and cap[:row_len].all() and cap[-row_len:].all(), key
                capd, offd = np.nonzero(cap)[0], np.nonzero(~cap)[0]
                with np.errstate(all="ignore"):
                    ref = [transpose_ref(rh, g[f]) for f in range(NF)]
                    exact = np.stack([r[0] for r in ref])[:, :, capd]
                    bound = np.stack([r[1] for r in ref])[:, :, capd]
                    # the terms of a cap-row source: its own entries and the cap's, as products
                    pt = cr.transposed(pat)
                    nan_in = np.zeros(exact.shape, bool)
                    pos_in, neg_in = nan_in.copy(), nan_in.copy()
                    for i, c in enumerate(capd):
                        q = (src0 == (0 if c < row_len else pat.n_src - row_len)) & (wp != 0.0)
                        e = slice(pt.rowptr[c], pt.rowptr[c + 1])
                        terms = np.concatenate([pt.val[e] * g[:, :, pt.col[e]], wp[q] * g[:, :, dst[q]]], axis=2)
                        nan_in[:, :, i] = np.isnan(terms).any(axis=2)
                        pos_in[:, :, i], neg_in[:, :, i] = np.isposinf(terms).any(axis=2), np.isneginf(terms).any(axis=2)
                must_nan = nan_in | (pos_in & neg_in)
                must_inf = (pos_in | neg_in) & ~must_nan
                checked = ~must_nan & ~must_inf & np.isfinite(bound)
                free = ~must_nan & ~must_inf & ~checked
                if kind == "ordinary":
                    assert checked.all(), key
                for ddt in (F64, F32):
                    with np.errstate(over="ignore"):
                        want = want64.astype(ddt)
                    for how, got in _transposes(R, rh, s, nlev, ddt):
                        what = ("pole 4", "transpose", nlev, kind, sdt, ddt) + how
                        held(got[:, :, offd], want[:, :, offd], what)
                        gc = got[:, :, capd].cpu().numpy().astype(F64)
                        with np.errstate(all="ignore"):
                            w = exact.astype(ddt).astype(F64)
                            tol = 8 * EPS * bound + (np.spacing(np.abs(exact.astype(F32))).astype(F64) if ddt == F32 else 0.0)
                            over = (ddt == F32) & (np.abs(exact) > 3.0e38)          # the float32 store of such a value may overflow
                            ok = np.where(must_nan, np.isnan(gc), np.where(must_inf, gc == np.where(pos_in, np.inf, -np.inf),
                                          np.where(checked & ~over, np.abs(gc - w) <= tol, True)))
                        assert ok.all(), (what, "cap rows", int((~ok).sum()), gc[~ok][:3], w[~ok][:3], tol[~ok][:3])
                n_held += int(checked.sum())
                n_free += int(free.sum())
                n_forced += int((must_nan | must_inf).sum())
    print("transpose pole caps: %d cap-row outputs held to the bound, %d forced non-finite, %d left free" % (n_held, n_forced, n_free))
    assert n_held > 10000 and n_forced > 0 and n_free < n_held


# ---- the rotation: mpg_rotate_winds_dev, mpg_rotate_winds ------------------------------------------------------------------------------
@pytest.mark.parametrize("nlev", (1, 65))
@pytest.mark.parametrize("npts", (1, 255, 256, 257))
def test_rotate_winds(gpu_lib, npts, nlev):
    """tana = sa / ca; den = ca + sa * tana; un = (uo + vo * tana) / den; vn = (vo - un * sa) / ca, seven rounded operations, in place;
    cos(alpha) entries of exactly 0.0 and -0.0 (a quotient by zero, an infinity times zero) come out as IEEE 754 has them"""
    import torch
    from mpassit_amd import regrid as R
    rng = np.random.default_rng(40 + npts)
    phi = rng.uniform(0.0, 2.0 * np.pi, npts)
    angles = []
    for zero in ((), (0.0,), (-0.0,)) if npts == 1 else ((0.0, -0.0),):
        ca, sa = np.cos(phi), np.sin(phi)
        for i, z in enumerate(zero):
            ca[(3 + 100 * i) % npts::131] = z
        if npts > 1:
            ca[npts - 1] = 0.0
            assert (ca == 0.0).sum() >= 3 and np.signbit(ca[ca == 0.0]).any() and not np.signbit(ca[ca == 0.0]).all()
        angles.append((ca, sa))
    for ca, sa in angles:
        for kind in KINDS:
            um, vm, _ = cr.mass_winds(npts, 1, nlev, kind)
            with np.errstate(all="ignore"):
                wu, wv = cr.rotate(ca, sa, um, vm)
            ut, vt = torch.from_numpy(um).cuda(), torch.from_numpy(vm).cuda()
            R.rotate_winds_cgrid(torch.from_numpy(ca).cuda(), torch.from_numpy(sa).cuda(), ut, vt)
            held(ut, wu, ("rotate, device", npts, nlev, kind, "u"))
            held(vt, wv, ("rotate, device", npts, nlev, kind, "v"))
            uh, vh = um.copy(), vm.copy()
            R.rotate_winds_cgrid(ca, sa, uh, vh)
            assert cr.same(uh, wu) and cr.same(vh, wv), ("rotate, host", npts, nlev, kind)


# ---- the Grid -> Grid wind chain: mpg_wind_destagger_dev, _pitched_dev, mpg_wind_destagger --------------------------------------------------
WIND_GRIDS = ((19, 11, 300000.0), (65, 17, 80000.0), (203, 35, 25000.0))      # mass points: narrower than a 64-point tile, one past it, 203 = 12 * 16 + 11
WIND_NLEVS = (1, 2, 17)


@pytest.fixture(scope="module")
def wind_grids(gpu_lib):
    from mpassit_amd import regrid as R, target_grid as T
    out = {}
    for nx, ny, dx in WIND_GRIDS:
        t = T.define_target_grid_params("lambert", nx + 1, ny + 1, dx=dx, dy=dx, **LAMBERT)
        grid = R.Grid.from_target(t)
        rh1, rh2 = R.regrid_store_grid(grid, R.STAGGERLOC_EDGE1), R.regrid_store_grid(grid, R.STAGGERLOC_EDGE2)
        ca, sa = (np.ascontiguousarray(a, F64).reshape(-1).copy() for a in (t.cosa, t.sina))
        assert ca.size == nx * ny and (rh1.nx_dst, rh1.ny_dst, rh2.nx_dst, rh2.ny_dst) == (nx + 1, ny, nx, ny + 1)
        # two points whose rotation divides by zero, on the first and the last row: a rim point is read by half the outputs an interior
        # one is, and on 19 x 11 at one level every non-finite mass point already costs 1 to 2 % of them
        ca[nx // 2], ca[(ny - 1) * nx + 1] = 0.0, -0.0
        out[nx] = dict(grid=grid, rh=(rh1, rh2), pat=(cr.Pattern.of(rh1), cr.Pattern.of(rh2)), ca=ca, sa=sa, nx=nx, ny=ny)
    yield out
    for d in out.values():
        for rh in d["rh"]:
            rh.release()
        d["grid"].destroy()


def _wind_dev(rh1, rh2, ca, sa, um, vm, nlev, dst_type, keep, ld):
    """mpg_wind_destagger_dev (ld 0) or mpg_wind_destagger_pitched_dev through the library itself, into NaN-filled results;
    returns (U, V, umass', vmass') as numpy arrays, U / V (nlev, ld or n_dst)"""
    import ctypes as C
    import torch
    from mpassit_amd import _lib as L
    dt = torch.float32 if dst_type & 1 else torch.float64
    new = lambda rh: None if rh is None else torch.full((nlev, ld or rh.n_dst), float("nan"), dtype=dt, device="cuda")   # noqa: E731
    U, V = new(rh1), new(rh2)
    ur, vr = (torch.full_like(um, float("nan")), torch.full_like(vm, float("nan"))) if keep else (None, None)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())       # noqa: E731
    h = lambda rh: None if rh is None else rh._h                         # noqa: E731
    head = (h(rh1), h(rh2), p(ca), p(sa), p(um), p(vm), C.c_int(nlev), p(U), p(V), C.c_int(dst_type), p(ur), p(vr))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if ld:
        L.check(L.load().mpg_wind_destagger_pitched_dev(*head, C.c_int64(ld), stream))
    else:
        L.check(L.load().mpg_wind_destagger_dev(*head, stream))
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (U, V, ur, vr))


def _same_result(got, want, dst_type, what):
    """equal bits, or NaN on both sides -- of a big-endian result after turning both round"""
    if got is None or want is None:
        assert got is None and want is None, what
        return
    g, w = (cr.swap(got), cr.swap(want)) if dst_type & 2 else (got, want)
    bad = cr.differs(g.reshape(w.shape), w)
    assert not bad.any(), (what, int(bad.sum()), bad.size, np.argwhere(bad)[0], g[bad][:2], w[bad][:2])


def _ring_is_plus_zero(d, U, V):
    """the outer half-cell ring -- U's first and last column, V's first and last row -- is unmapped: +0.0, the sign bit clear"""
    nx, ny = d["nx"], d["ny"]
    if U is not None:
        u = U[:, :ny * (nx + 1)].reshape(-1, ny, nx + 1)
        assert (cr.bits(u[:, :, [0, nx]]) == 0).all(), "U ring"
    if V is not None:
        v = V[:, :(ny + 1) * nx].reshape(-1, ny + 1, nx)
        assert (cr.bits(v[:, [0, ny], :]) == 0).all(), "V ring"


@pytest.mark.parametrize("rot", (True, False), ids=("rotated", "unrotated"))
@pytest.mark.parametrize("nx", [g[0] for g in WIND_GRIDS])
def test_wind_destagger(wind_grids, nx, rot):
    """cr_rotate on copies of the mass winds, the 4-slot chain on each handle's own idx / w, the float64 entry storing the sum as it
    stands and every typed result (TD)fma(sum, 1, 0): the bits of cr_wind_destagger from the device entry, the pitched one (one odd
    stride for both, NaN between the planes untouched) and the host entry; both components, U only, V only; the rotated mass winds asked
    for and left out; specials on the first and last row and column of the mass winds"""
    import torch
    from mpassit_amd import regrid as R
    d = wind_grids[nx]
    (rh1, rh2), (p1, p2), ny = d["rh"], d["pat"], d["ny"]
    ring1, ring2 = np.zeros((ny, nx + 1), bool), np.zeros((ny + 1, nx), bool)
    ring1[:, [0, nx]], ring2[[0, ny], :] = True, True
    assert p1.unmapped[ring1.reshape(-1)].all() and p2.unmapped[ring2.reshape(-1)].all() and not p1.unmapped[~ring1.reshape(-1)].any()
    ca, sa = (d["ca"], d["sa"]) if rot else (None, None)
    cat, sat = (torch.from_numpy(ca).cuda(), torch.from_numpy(sa).cuda()) if rot else (None, None)
    which = ((p1, p2, rh1, rh2),) if rot else ((p1, p2, rh1, rh2), (p1, None, rh1, None), (None, p2, None, rh2))
    ld = max(p1.n_dst, p2.n_dst) + 5
    for nlev in WIND_NLEVS:
        for kind in KINDS:
            um, vm, where = cr.mass_winds(nx, ny, nlev, kind)
            umt, vmt = torch.from_numpy(um).cuda(), torch.from_numpy(vm).cuda()
            if kind == "special":
                with np.errstate(all="ignore"):
                    U, V, _, _ = cr.wind_destagger(p1, p2, ca, sa, um, vm, nlev)
                fin = cr.winds_are_informative(p1, p2, rot, where, U, V)
                print("%3d x %2d, %2d levels, %s: %.2f %% of the outputs of the special mass winds finite" % (nx, ny, nlev, "rotated" if rot else "unrotated", 100 * fin))
            for q1, q2, h1, h2 in which:
                for dst_type in (0, 1, 2, 3):
                    for keep in ((True, False) if rot else (False,)):
                        with np.errstate(all="ignore"):
                            dense = cr.wind_destagger(q1, q2, ca, sa, um, vm, nlev, dst_type, 0, keep)
                            pitched = cr.wind_destagger(q1, q2, ca, sa, um, vm, nlev, dst_type, ld, keep)
                        what = (nx, nlev, kind, rot, dst_type, keep, q1 is not None, q2 is not None)
                        a, b = (umt if (q1 is not None or rot) else None), (vmt if (q2 is not None or rot) else None)
                        for entry, want, got in (("device", dense, _wind_dev(h1, h2, cat, sat, a, b, nlev, dst_type, keep, 0)),
                                                 ("pitched", pitched, _wind_dev(h1, h2, cat, sat, a, b, nlev, dst_type, keep, ld))):
                            for i in range(4):
                                _same_result(got[i], want[i], dst_type if i < 2 else 0, what + (entry, i))
                            _ring_is_plus_zero(d, got[0], got[1])
                        ha, hb = (um.copy() if a is not None else None), (vm.copy() if b is not None else None)
                        got = R.wind_destagger(h1, h2, ca, sa, ha, hb, nlev, out_dtype=F32 if dst_type & 1 else F64, dst_be=bool(dst_type & 2), keep_mass=keep)
                        for i in range(4):
                            _same_result(got[i], dense[i], dst_type if i < 2 else 0, what + ("host", i))
                        assert (ha is None or cr.same(ha, um)) and (hb is None or cr.same(hb, vm)), "the host entry leaves its inputs alone"


def test_wind_destagger_periodic(case):
    """The periodic 72 x 36 grid, unrotated.  U, and V off its two pole rows: the bits of cr_wind_destagger.  The pole rows of V -- counted:
    2 * 72 points, rows 0 and ny -- are cap points and held as test_pole_caps holds them: must-be-NaN rows, bits where the reference is
    not finite, its bound plus one unit in the last place elsewhere."""
    import torch
    rh1, rh2, p1, p2 = case.rh["periodic E1"], case.rh["pole 4"], case.pat["periodic E1"], case.pat["pole 4"]
    nx, ny = 72, 36
    assert (p1.pole is None or not (p1.pole[2] != 0.0).any()) and p2.pole is not None and (rh1.nx_dst, rh1.ny_dst, rh2.nx_dst, rh2.ny_dst) == (nx + 1, ny, nx, ny + 1)
    n_cap = 0
    for nlev in WIND_NLEVS:
        for kind in KINDS:
            um, vm, _ = cr.mass_winds(nx, ny, nlev, kind)
            umt, vmt = torch.from_numpy(um).cuda(), torch.from_numpy(vm).cuda()
            for dst_type in (0, 1, 2, 3):
                dt = F32 if dst_type & 1 else F64
                with np.errstate(all="ignore"):
                    wu, wv, _, _ = cr.wind_destagger(p1, p2, None, None, um, vm, nlev, dst_type)
                    pts, want, bound, must_nan, free = cr.pole_caps(p2, vm[None], nlev, 1, False, dt, dst_type != 0, 1.0, 0.0)
                assert pts.size == 2 * nx and set((pts // nx).tolist()) == {0, ny}, "the excluded points are V's two pole rows and no more"
                other = np.ones(p2.n_dst, bool)
                other[pts] = False
                U, V, _, _ = _wind_dev(rh1, rh2, None, None, umt, vmt, nlev, dst_type, False, 0)
                what = ("periodic", nlev, kind, dst_type)
                _same_result(U, wu, dst_type, what + ("U",))
                _same_result(V[:, other], wv[:, other], dst_type, what + ("V off the pole rows",))
                g = (cr.swap(V) if dst_type & 2 else V)[:, pts][None]
                with np.errstate(all="ignore"):
                    w = want.astype(dt)
                    exact = ~np.isfinite(w) & ~must_nan & ~free
                    tol = bound + np.spacing(np.abs(w)).astype(F64)
                    ok = np.where(must_nan, np.isnan(g), np.where(exact, ~cr.differs(g, w), free | (np.abs(g.astype(F64) - w.astype(F64)) <= tol)))
                assert ok.all(), (what, "pole rows", int((~ok).sum()), g[~ok][:3], w[~ok][:3], tol[~ok][:3])
                n_cap += int((~free).sum())
    assert n_cap > 1000
