"""The fused wind chain (mpg_wind_destagger_dev, csrc/k_wind.hip) against the ORACLE at the sizes it runs at.

test_wind_gpu.py holds the kernel to the library's own three-call chain on grids of at most 203 x 131 points.  Here it is held to the
oracle's restatement -- orc_rotate_winds, then orc_apply_fixed / the monopole apply of the Grid -> Grid weights -- on
  * the README's 1800 x 1060 Lambert grid (U rows 1801 wide: 29 x 67 tiles, a partial last tile in both directions),
  * HRRR's 1799 x 1059 (namelist nx = 1800, ny = 1060 in the reference's parm/namelist.input): U rows 1800 wide, V rows 1799 wide,
    other row residues mod 8 and other partial tiles, an odd number of points per level plane,
  * the periodic 3600 x 1800 lat-lon grid of configuration 5, whose V pole rows are pole-cap points (the kernel's `far` path, then
    k_pole_fix).
The mass winds are i.i.d. per point AND per level, so a wrong window slot, a wrong neighbour, a level-buffer swap or a wrong level is an
O(1) error at the point it hits; 55 levels on the Lambert grids take the double-buffered window through every parity many times.  Results
go into NaN-filled buffers between canary bands (tests/_oracle_compare.py): an unwritten point or a write outside the result fails."""
import ctypes as C

import numpy as np
import pytest

from _oracle_compare import Banded, assert_close, assert_f32_ulp, assert_zero, compare_grid_weights, from_be32, ring_mask

pytestmark = pytest.mark.gpu

NLEV_LAMBERT = 55
NLEV_C5 = 5                # odd; 3600 x 1800 points per level keep the host side small
CHUNK = 5                  # levels per oracle chunk (host memory: a few hundred MB at a time)
F64, F32_BE = 0, 3         # dst_type: MPG_TYPE_F32 = 1 | MPG_TYPE_BE = 2

GRIDS = {
    "lambert_1800x1060": lambda W, T: W.conus_lambert_grid(),
    "lambert_1799x1059": lambda W, T: W.conus_lambert_grid(nx=1800, ny=1060),
    "latlon_3600x1800_poles": lambda W, T: T.define_target_grid_params("lat-lon", nx=3601, ny=1801, stand_lon=0.0, is_regional=False),
}


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _handle_ref(o, t, idx, w, pole, src, nlev):
    """The handle's own weights through the oracle's apply: orc_apply_fixed, plus the pole term on a periodic grid."""
    if pole is None:
        return o.apply_fixed(idx, w, src, nlev)
    return o.apply_grid_periodic(t.nx, idx, w, pole[0], pole[1], src, nlev)


@pytest.mark.parametrize("name", list(GRIDS))
def test_fused_wind_chain_against_oracle(gpu_lib, oracle, name):
    import torch
    from mpassit_amd import _lib as L, regrid as R, target_grid as T, workloads as W
    o = oracle
    t = GRIDS[name](W, T)
    periodic = name.startswith("latlon")
    rot = not periodic
    nlev = NLEV_C5 if periodic else NLEV_LAMBERT
    nx, ny = t.nx, t.ny
    grid = R.Grid.from_target(t)
    rh = {"U": R.regrid_store_grid(grid, R.STAGGERLOC_EDGE1), "V": R.regrid_store_grid(grid, R.STAGGERLOC_EDGE2)}
    shape = {"U": (ny, nx + 1), "V": (ny + 1, nx)}
    P = {c: shape[c][0] * shape[c][1] for c in "UV"}
    report = {}

    # ---- 1. the Store: the handles' weights against the oracle's Grid -> Grid search --------------------------------------------
    cen = o.lonlat_deg_to_xyz(t.lon, t.lat)
    wts = {}
    for c, st, lon, lat in (("U", 1, t.lon_u, t.lat_u), ("V", 2, t.lon_v, t.lat_v)):
        dxyz = o.lonlat_deg_to_xyz(lon, lat)
        gi, gw = rh[c].weights()
        dst, src0, wp, row_len = rh[c].pole()
        if periodic:
            oi, ow, opsrc0, opw = o.grid_bilinear_periodic(nx, ny, 1, cen, st, dxyz)
            nxd = shape[c][1]
            assert row_len == nx and np.array_equal(dst, np.r_[np.arange(nxd), P[c] - nxd + np.arange(nxd)])
            cap = opw.reshape(-1) != 0.0
            assert cap.any() == (c == "V"), "the V pole rows, and only they, are pole caps"
            np.testing.assert_allclose(wp, opw.reshape(-1), rtol=0, atol=1e-12)
            assert np.array_equal(src0[cap], opsrc0.reshape(-1)[cap])
            assert (gi[:, 0] >= 0).all() and (oi[:, 0] >= 0).all(), "a closed sphere has no unmapped point"
            # cap rows: corners A / B as the oracle's, zero-weight fillers (oracle: -1) in the other two slots
            capd = dst[cap]
            assert np.array_equal(gi[capd, :2], oi[capd, :2]) and (gw[capd, 2:] == 0.0).all() and (oi[capd, 2:] == -1).all()
            np.testing.assert_allclose(gw[capd, :2], ow[capd, :2], rtol=0, atol=1e-12)
            gpole, opole = (src0.reshape(2, nxd), wp.reshape(2, nxd)), (opsrc0, opw)
        else:
            oi, ow = o.grid_bilinear(nx, ny, cen, st, dxyz)
            assert dst.size == 0
            gpole = opole = None
        # 3-km Lambert: 2e-12, the float64 floor of a weight there (DESIGN s2: whole Stores against 50-digit answers, the lat / lon ->
        # unit vector step over a 4.7e-4 rad cell); 1e-12 on the 0.1-degree lat-lon grid
        dw, ring_diff = compare_grid_weights(oi, ow, gi, gw, shape[c], tol=1e-12 if periodic else 2e-12)
        report["store_%s" % c] = dict(interior_weight_diff=dw, ring_mapped_set_diff=ring_diff)
        # check 3's bar per point: what the two weight sets' difference can explain (sum over the corners of |dw| x max|wind|) plus
        # the rounding of the sum -- an error of the kernel is not explained by it; the ring's differing corners are not compared
        dsum = np.where((oi == gi).all(axis=1), np.abs(ow - gw).sum(axis=1), 0.0) + 1e-14
        wts[c] = dict(gi=gi, gw=gw, oi=oi, ow=ow, gpole=gpole, opole=opole, unmapped=torch.as_tensor(gi[:, 0] < 0, device="cuda"),
                      bar_o=torch.as_tensor(dsum, device="cuda"))
    inner = {c: torch.as_tensor(~ring_mask(*shape[c]).reshape(-1), device="cuda") for c in "UV"}

    # ---- inputs: i.i.d. per point and level --------------------------------------------------------------------------------------
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1799 + nx)
    um = (torch.rand((nlev, ny, nx), dtype=torch.float64, device="cuda", generator=gen) - 0.5) * 60.0
    vm = (torch.rand((nlev, ny, nx), dtype=torch.float64, device="cuda", generator=gen) - 0.5) * 60.0
    um0, vm0 = um.clone(), vm.clone()
    cosa = torch.as_tensor(np.ascontiguousarray(t.cosa, dtype=np.float64), device="cuda") if rot else None
    sina = torch.as_tensor(np.ascontiguousarray(t.sina, dtype=np.float64), device="cuda") if rot else None
    lib = L.load()
    if periodic:   # a rotation under pole caps: no projection of the reference asks for it -> refused, nothing written
        ones = torch.ones((ny, nx), dtype=torch.float64, device="cuda")
        bu, bv = Banded(torch, nlev * P["U"], torch.float64), Banded(torch, nlev * P["V"], torch.float64)
        rc = lib.mpg_wind_destagger_dev(rh["U"]._h, rh["V"]._h, _p(ones), _p(ones * 0.0), _p(um), _p(vm), nlev, _p(bu.res), _p(bv.res), F64,
                                        None, None, None)
        assert rc == L.MPG_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool(bu.res.isnan().all()) and bool(bv.res.isnan().all())
        bu.assert_canaries("refused U")
        bv.assert_canaries("refused V")

    # ---- the kernel: (result type, elements into a 128-byte line, KEEP) ----------------------------------------------------------
    runs = [(F64, 0, rot), (F64, 1, False), (F32_BE, 0, False), (F32_BE, 1, False)]
    out = {}
    for dt, shift, keep in runs:
        tdt = torch.float64 if dt == F64 else torch.float32
        bu, bv = Banded(torch, nlev * P["U"], tdt, shift), Banded(torch, nlev * P["V"], tdt, shift)
        kr = (Banded(torch, nlev * nx * ny, torch.float64, shift), Banded(torch, nlev * nx * ny, torch.float64, shift)) if keep else (None, None)
        rc = lib.mpg_wind_destagger_dev(rh["U"]._h, rh["V"]._h, _p(cosa), _p(sina), _p(um), _p(vm), nlev, _p(bu.res), _p(bv.res), dt,
                                        _p(kr[0].res) if keep else None, _p(kr[1].res) if keep else None, None)
        assert rc == 0, lib.mpg_last_error()
        torch.cuda.synchronize()
        what = "%s dst_type %d shift %d" % (name, dt, shift)
        for b, c in ((bu, "U"), (bv, "V")) + (((kr[0], "UMASS"), (kr[1], "VMASS")) if keep else ()):
            b.assert_canaries("%s %s" % (what, c))
        out[(dt, shift)] = (bu, bv, kr)
    assert torch.equal(um, um0) and torch.equal(vm, vm0), "the mass winds are inputs"
    # the results one element into a line: the same bits as the aligned ones (which are held to the oracle below)
    for dt in (F64, F32_BE):
        for k in (0, 1):
            a, b = out[(dt, 0)][k].res, out[(dt, 1)][k].res
            it = torch.int64 if a.element_size() == 8 else torch.int32
            assert torch.equal(a.view(it), b.view(it)), "%s: dst_type %d, %s one element into a line differs" % (name, dt, "UV"[k])

    # ---- 2.-5. against the oracle, a chunk of levels at a time -------------------------------------------------------------------
    stat = {k: 0.0 for k in ("U_vs_handle_w", "V_vs_handle_w", "U_vs_oracle_w", "V_vs_oracle_w")}
    ne32 = {"U": 0, "V": 0}
    umax32 = 0
    keep_checked = 0
    for k0 in range(0, nlev, CHUNK):
        k1 = min(nlev, k0 + CHUNK)
        nl = k1 - k0
        umh = um[k0:k1].reshape(nl, -1).cpu().numpy()
        vmh = vm[k0:k1].reshape(nl, -1).cpu().numpy()
        if rot:
            umh, vmh = o.rotate_winds(t.cosa, t.sina, umh, vmh)
            kr = out[(F64, 0)][2]
            for b, want, c in ((kr[0], umh, "UMASS"), (kr[1], vmh, "VMASS")):      # 4. KEEP: bit for bit
                got = b.res.view(nlev, -1)[k0:k1]
                assert torch.equal(got.view(torch.int64), torch.as_tensor(want, device="cuda").view(torch.int64)), "%s %s levels %d-%d" % (name, c, k0, k1)
                keep_checked += 1
        for c, src, slot in (("U", umh, 0), ("V", vmh, 1)):
            wc = wts[c]
            scale = float(np.abs(src).max())
            ref_g = torch.as_tensor(_handle_ref(o, t, wc["gi"], wc["gw"], wc["gpole"], src, nl), device="cuda")
            ref_o = torch.as_tensor(_handle_ref(o, t, wc["oi"], wc["ow"], wc["opole"], src, nl), device="cuda")
            got = out[(F64, 0)][slot].res.view(nlev, -1)[k0:k1]
            what = "%s %s levels %d-%d" % (name, c, k0, k1)
            # 2. every point, ring included, against the handle's weights through the oracle's apply; unmapped points exactly 0.0
            stat[c + "_vs_handle_w"] = max(stat[c + "_vs_handle_w"], assert_close(got, ref_g, 1e-14, scale, what + " vs handle weights"))
            assert_zero(got, wc["unmapped"], what)
            # 3. interior against the oracle's own weights: the mathematics, not the Store
            stat[c + "_vs_oracle_w"] = max(stat[c + "_vs_oracle_w"], assert_close(got, ref_o, wc["bar_o"], scale, what + " vs oracle weights",
                                                                                   mask=inner[c]))
            # 5. float32 | BE: byte-swapped back, against float32(reference)
            g32 = from_be32(out[(F32_BE, 0)][slot].res.view(nlev, -1)[k0:k1])
            u, frac = assert_f32_ulp(g32, ref_g, what + " float32 BE", eps=1e-14 * scale)
            umax32 = max(umax32, u)
            ne32[c] += int(round(frac * g32.numel()))
            del ref_g, ref_o
    assert keep_checked == (2 * len(range(0, nlev, CHUNK)) if rot else 0)
    for c in "UV":
        report["f32_be_%s" % c] = dict(max_ulp=umax32, frac_1ulp=ne32[c] / (nlev * P[c]))
    report.update(stat)
    print("\n%s: %s" % (name, report))
    for c in "UV":
        rh[c].release()
    grid.destroy()

