#!/usr/bin/env python3
"""Store-time masks (mpg_handle_mask, mpg_handle_extrapolate_masked) on configuration 4 (c4_3m_regional: 3.0 M cells -> 1800 x 1060), in ONE
process on one card.  Source mask: tools/masked_probe.py's land-sea mask, about 30 % of the cells in coherent patches; no destination mask.
Per handle -- bilinear (fixed, 3 slots), nearest (fixed, 1 slot), conservative (CSR) -- the GPU time (mpg_handle_store_ms) of

  mask          mask_handle(rh, mask) under MASKRULE_AUTO: the ROW rule for bilinear and nearest, the ENTRY rule for conservative
  fill_masked   extrapolate_masked(masked handle, mask), nearest-source-to-destination: the rows the mask unmapped, refilled from land
  fill_zero     extrapolate_masked(masked handle, an all-zero mask): the same rows from every cell THROUGH the alive walk -- against
  fill_plain    extrapolate(masked handle), the unmasked kernels, it shows what the alive pass and the mask loads cost
  fill_idavg8   extrapolate_masked(masked handle, mask) with the inverse-distance average of N = 8 (a CSR result)

each the median of --reps calls with min and max.  One JSON line; --out writes markdown too.  Run it under a time limit of its own:
    timeout -k 10 900 python tools/store_masks_probe.py [--out profiles/r28_store_masks_measured.md]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="the same cases at a size for a quick look (20 000 cells under 181 x 107)")
    ap.add_argument("--out", default=None, help="also write the record as markdown to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    from masked_probe import land_sea_mask
    from mpassit_amd import _lib, regrid as R, synth, workloads
    _lib.init(0)
    t0 = time.time()

    def note(what):
        print("[%6.1f s] %s" % (time.time() - t0, what), file=sys.stderr, flush=True)

    if a.small:
        g = workloads.conus_lambert_grid(nx=181, ny=107, dx=30000.0, dy=30000.0)
        m = synth.regional_mesh_for_lambert(g.proj, 181, 107, 20000)
        desc = "small: 20 000 cells under 181 x 107"
    else:
        m, g, _, desc = workloads.workload("c4_3m_regional")
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
    mask_np = land_sea_mask(m.latCell, m.lonCell)
    mask = torch.as_tensor(mask_np, device="cuda")
    zero = torch.zeros_like(mask)
    note("mesh (%d cells) and grid (%d x %d); %.1f %% of the cells masked" % (m.nCells, g.nx, g.ny, 100.0 * mask_np.mean()))
    res = {"what": "store_masks_probe", "workload": desc, "cells": int(m.nCells), "grid": [g.nx, g.ny], "mask_fraction": round(float(mask_np.mean()), 4),
           "reps": a.reps, "handles": {}}

    def timed(make):
        ms, last = [], None
        for _ in range(a.reps):
            if last is not None:
                last.release()
            last = make()
            ms.append(last.store_ms)
        s = sorted(ms)
        return last, {"ms_median": round(s[len(s) // 2], 3), "ms_min": round(s[0], 3), "ms_max": round(s[-1], 3)}

    STOD, IDAVG = R.EXTRAPMETHOD_NEAREST_STOD, R.EXTRAPMETHOD_NEAREST_IDAVG
    for name, method in (("bilinear", R.REGRIDMETHOD_BILINEAR), ("nearest", R.REGRIDMETHOD_NEAREST_STOD), ("conservative", R.REGRIDMETHOD_CONSERVE)):
        rh = R.regrid_store(mesh, grid, method)
        r = {"store_ms": round(rh.store_ms, 3), "nnz_per_row": rh.nnz_per_row, "nnz": rh.nnz, "rows": rh.n_dst}
        masked, r["mask"] = timed(lambda: R.mask_handle(rh, mask))
        st = masked.store_stats
        r["mask"].update(rows_unmapped_by_source=st[1], entries_removed=st[3])
        legs = (("fill_masked", lambda: R.extrapolate_masked(masked, mesh, grid, mask, None, STOD)),
                ("fill_zero", lambda: R.extrapolate_masked(masked, mesh, grid, zero, None, STOD)),
                ("fill_plain", lambda: R.extrapolate(masked, mesh, grid, STOD)),
                ("fill_idavg8", lambda: R.extrapolate_masked(masked, mesh, grid, mask, None, IDAVG, 8, 2.0)))
        keep = {}
        for leg, make in legs:
            h, r[leg] = timed(make)
            r[leg].update(rows_filled=h.store_stats[1], K=h.store_stats[2], nnz_per_row=h.nnz_per_row)
            keep[leg] = h
        # the zero mask must give the plain call's bytes; the masked fill must reference land alone
        if masked.nnz_per_row:
            r["zero_mask_equals_plain"] = bool(all(np.array_equal(x, y) for x, y in zip(keep["fill_zero"].weights(), keep["fill_plain"].weights())))
            idx = keep["fill_masked"].weights()[0]
            r["masked_fill_references_land_only"] = bool(not mask_np[idx[idx >= 0]].any())
        else:
            r["zero_mask_equals_plain"] = bool(all(np.array_equal(x, y) for x, y in zip(keep["fill_zero"].csr(), keep["fill_plain"].csr())))
            r["masked_fill_references_land_only"] = bool(not mask_np[keep["fill_masked"].csr()[1]].any())
        r["ns_per_filled_row"] = {leg: round(r[leg]["ms_median"] * 1e6 / max(r[leg]["rows_filled"], 1), 2) for leg, _ in legs}
        note("%s: mask %.3f ms; fill masked %.3f, zero mask %.3f, plain %.3f, idavg8 %.3f ms (%d rows)" % (
            name, r["mask"]["ms_median"], r["fill_masked"]["ms_median"], r["fill_zero"]["ms_median"], r["fill_plain"]["ms_median"],
            r["fill_idavg8"]["ms_median"], r["fill_masked"]["rows_filled"]))
        for h in list(keep.values()) + [masked, rh]:
            h.release()
        res["handles"][name] = r
    res["total_s"] = round(time.time() - t0, 1)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("%s; %d cells, %d x %d mass points; %.1f %% of the cells masked.  Medians of %d calls.\n\n" % (
                desc, res["cells"], g.nx, g.ny, 100.0 * res["mask_fraction"], a.reps))
            f.write("```json\n%s\n```\n" % json.dumps(res, indent=1))
    for o in (mesh, grid):
        o.destroy()
    _lib.finalize()


if __name__ == "__main__":
    main()
