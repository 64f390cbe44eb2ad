#!/usr/bin/env python3
"""Masked Regrid (mpg_regrid_masked_dev) on configuration 4: c4_3m_regional's bilinear handle (3.0 M cells -> 1800 x 1060), 13 fields x 55
levels, float64 cell-fast and float32 file order (level-fast).  Per layout, in ONE process:
    masked_nogap    the masked call on a field without gaps (missing = NaN, none present)
    masked_mask30   the masked call with a land-sea-like static mask: about 30 % of the cells, in coherent patches
    unmasked_model  the unmasked typed call forced onto the kernel the masked one is modelled on -- the lane gather (tune a3_staged = -2)
                    for cell-fast, the row gather on grid-row tiles (tune lf_variant = 2) for file order: the cost of masking itself
    unmasked        the unmasked typed call as the library picks it (context)
A timed block is --batch launches back to back between one pair of HIP events behind one untimed launch; the median per-call ms over --reps
blocks and the fraction of the 8 TB/s peak of bench.py's algorithmic bytes,  nf * nlev * (U * es_src + P * es_dst) + P * 36  (U = the
sources the handle references), go out as one JSON line.  Run it under rocprofv3 --kernel-trace --stats for the per-kernel times
(--only LAYOUT:LEG runs one leg).
    python tools/masked_probe.py [--reps 7] [--batch 3] [--warmup 2] [--nfields 13] [--only cell_fast_f64:masked_nogap]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12
LEGS = ("masked_nogap", "masked_mask30", "unmasked_model", "unmasked")


def land_sea_mask(lat, lon, frac=0.3):
    """True on about `frac` of the cells, in coherent patches: where a smooth function of position exceeds its (1 - frac) quantile."""
    import numpy as np
    f = np.sin(7.0 * lon) * np.cos(5.0 * lat) + 0.6 * np.sin(13.0 * lat + 3.0 * lon) + 0.3 * np.cos(29.0 * lon - 17.0 * lat)
    return f > np.quantile(f, 1.0 - frac)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nfields", type=int, default=13)
    ap.add_argument("--only", default=None, help="LAYOUT:LEG, LAYOUT in cell_fast_f64 | lev_fast_f32")
    a = ap.parse_args()
    import time
    import torch
    from mpassit_amd import _lib, regrid as R, workloads
    _lib.init(0)
    t0 = time.time()
    m, g, nlev, desc = workloads.workload("c4_3m_regional")
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
    rh = R.regrid_store(mesh, grid, R.REGRIDMETHOD_BILINEAR)
    nf = a.nfields
    U = int(rh.unique_sources().size)
    mask_np = land_sea_mask(m.latCell, m.lonCell)
    mask = torch.as_tensor(mask_np, device="cuda")
    res = {"what": "masked_probe", "workload": desc, "nfields": nf, "nlev": nlev, "n_src": rh.n_src, "n_dst": rh.n_dst, "unique_src": U,
           "mask_fraction": round(float(mask_np.mean()), 4), "setup_s": round(time.time() - t0, 1), "peak_tb_s": PEAK / 1e12}
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        e0.record()
        for _ in range(a.batch):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.batch

    for lname, dt, layout, knob in (("cell_fast_f64", torch.float64, R.LAYOUT_CELL_FAST, ("a3_staged", -2, -1)),
                                    ("lev_fast_f32", torch.float32, R.LAYOUT_LEV_FAST, ("lf_variant", 2, -1))):
        if a.only and a.only.split(":")[0] != lname:
            continue
        es = 4 if dt == torch.float32 else 8
        src = torch.rand(nf * nlev * rh.n_src, dtype=dt, device="cuda", generator=gen) - 0.5
        out = torch.empty((nf, nlev, rh.ny_dst, rh.nx_dst), dtype=dt, device="cuda")
        by = nf * nlev * (U * es + rh.n_dst * es) + rh.n_dst * 36
        kw = dict(nlev=nlev, nfields=nf, layout=layout, out=out)

        def model():
            _lib.tune(knob[0], knob[1])
            rh.regrid_typed(src, **kw)
            _lib.tune(knob[0], knob[2])

        legs = {"masked_nogap": lambda: rh.regrid_masked(src, fill_value=-9999.0, **kw),
                "masked_mask30": lambda: rh.regrid_masked(src, src_mask=mask, fill_value=-9999.0, **kw),
                "unmasked_model": model,
                "unmasked": lambda: rh.regrid_typed(src, **kw)}
        r = {"alg_bytes": by}
        if not a.only:   # no gaps: the same bits as the unmasked call on mapped points
            legs["unmasked"]()
            want = out.clone()
            legs["masked_nogap"]()
            torch.cuda.synchronize()
            diff = out != want
            r["nogap_differs_only_where_filled"] = bool((out[diff] == -9999.0).all())
            r["filled_points_per_plane"] = int(diff[0, 0].sum())
            del want, diff
        for name in LEGS:
            if a.only and a.only.split(":")[1] != name:
                continue
            fn = legs[name]
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            ms = sorted(timed(fn) for _ in range(a.reps))
            med = ms[len(ms) // 2]
            r[name] = {"ms_median": round(med, 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3), "hbm_fraction": round(by / (med * 1e-3) / PEAK, 3)}
        res[lname] = r
        del src, out
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    rh.release()
    mesh.destroy()
    grid.destroy()
    _lib.finalize()


if __name__ == "__main__":
    main()
