#!/usr/bin/env python3
"""Creep-fill extrapolation (mpg_handle_creep) at configuration 4's sizes, in ONE process on one card: the 3.0 M-cell regional mesh built
with a NEGATIVE margin, so that it stops short of the rim of its 1800 x 1060 Lambert grid, and the bilinear Mesh -> Grid handle of the two.

  creep      mpg_handle_creep with 1, 4 and all levels: GPU time of the call (mpg_handle_store_ms), the median of --reps calls with min and
             max after a first call that loads the module; rows filled, the last level, rows left, entries and the longest row of the result.
  split      one call per level count 1, 2, 3, ... up to the last level: the time of L levels minus the time of L - 1 is level L's share
             (single calls: read them as a profile, not as medians).
  yardstick  mpg_handle_extrapolate NEAREST_STOD on the same handle, the same way: the only way to fill those rows without the creep.
  regrid     55 levels, float32, file order, through the unfilled handle (fixed, 3 slots), the nearest-filled one (fixed) and the crept one
             (CSR, every row): the median per-call ms with min and max.

One JSON line; --out writes markdown too.  Run it under a time limit of its own:
    timeout -k 10 900 python tools/creep_probe.py [--out profiles/r31_creep_measured.md]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stat(v):
    return {"ms_median": round(sorted(v)[len(v) // 2], 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--margin", type=float, default=-0.01, help="the mesh's margin about the grid, negative: it stops short of the rim")
    ap.add_argument("--small", action="store_true", help="the same at a size for a quick look (20 000 cells under 181 x 107)")
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--out", default=None, help="also write the record as markdown to this file")
    a = ap.parse_args()
    import torch
    from mpassit_amd import _lib, regrid as R, synth, workloads
    _lib.init(0)
    t0 = time.time()

    def note(what):
        print("[%6.1f s] %s" % (time.time() - t0, what), file=sys.stderr, flush=True)

    nxs, nys, ncells, over = (181, 107, 20000, dict(dx=30000.0, dy=30000.0)) if a.small else (1801, 1061, 3_000_000, {})
    nlev = 55
    note("building the mesh")
    g = workloads.conus_lambert_grid(nx=nxs, ny=nys, **over)
    m = synth.regional_mesh_for_lambert(g.proj, nxs, nys, ncells, margin=a.margin)
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
    note("mesh (%d cells, margin %g) and grid (%d x %d mass points)" % (m.nCells, a.margin, g.nx, g.ny))
    res = {"what": "creep_probe", "cells": int(m.nCells), "margin": a.margin, "grid": [g.nx, g.ny], "nlev": nlev}
    bil = R.regrid_store(mesh, grid, R.REGRIDMETHOD_BILINEAR)
    res["bilinear_store_ms"] = round(bil.store_ms, 3)

    def timed(make):
        """the median of --reps calls after a first one -> (the last handle, the record)"""
        ms, wall, h = [], [], None
        for _ in range(a.reps + 1):
            if h is not None:
                h.release()
            torch.cuda.synchronize()
            w0 = time.time()
            h = make()
            wall.append((time.time() - w0) * 1e3)
            ms.append(h.store_ms)
        rec = _stat(ms[1:])
        rec.update(first_call_ms=round(ms[0], 3), wall_ms_median=round(sorted(wall[1:])[len(wall[1:]) // 2], 2))
        return h, rec

    res["creep"] = {}
    crept = None
    for name, levels in (("1", 1), ("4", 4), ("all", R.CREEP_ALL_LEVELS)):
        h, rec = timed(lambda: R.creep(bil, grid, levels))
        st = h.store_stats
        rec.update(rows_filled=st[1], last_level=st[2], rows_left=st[3], longest_row=st[6], nnz=h.nnz,
                   ns_per_filled_row=round(rec["ms_median"] * 1e6 / max(st[1], 1), 2))
        res["creep"][name] = rec
        note("creep, %s levels: %.3f ms, %d rows filled, last level %d, %d left, longest row %d" % (name, rec["ms_median"], st[1], st[2], st[3], st[6]))
        if name == "all":
            crept = h
        else:
            h.release()
    last = res["creep"]["all"]["last_level"]
    if not a.no_split:
        cum = []
        for L in range(1, last + 1):
            h = R.creep(bil, grid, L)
            cum.append((h.store_ms, h.store_stats[1], h.nnz))
            h.release()
        res["split"] = [{"level": L + 1, "ms": round(c[0] - (cum[L - 1][0] if L else 0.0), 3), "cumulative_ms": round(c[0], 3),
                         "rows": c[1] - (cum[L - 1][1] if L else 0), "entries": c[2] - cum[L - 1][2] if L else None}
                        for L, c in enumerate(cum)]                 # (level 1's own entries: its count includes the copy of the mapped rows)
        note("split: %d single calls" % len(cum))

    stod, rec = timed(lambda: R.extrapolate(bil, mesh, grid, R.EXTRAPMETHOD_NEAREST_STOD))
    rec.update(rows_filled=stod.store_stats[1], nnz_per_row=stod.nnz_per_row)
    res["yardstick_nearest_stod"] = rec
    note("extrapolate NEAREST_STOD: %.3f ms, %d rows" % (rec["ms_median"], rec["rows_filled"]))

    x = torch.randn((m.nCells, nlev), dtype=torch.float32, device="cuda")
    outs = {k: torch.empty((1, nlev, g.ny, g.nx), dtype=torch.float32, device="cuda") for k in ("unfilled", "nearest", "crept")}
    routes = {"unfilled": lambda: bil.regrid_typed(x, nlev=nlev, layout=R.LAYOUT_LEV_FAST, out=outs["unfilled"]),
              "nearest": lambda: stod.regrid_typed(x, nlev=nlev, layout=R.LAYOUT_LEV_FAST, out=outs["nearest"]),
              "crept": lambda: crept.regrid_typed(x, nlev=nlev, layout=R.LAYOUT_LEV_FAST, out=outs["crept"])}
    for fn in routes.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in routes}
    for _ in range(a.reps):
        for k, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            e0.record()
            for _ in range(a.batch):
                fn()
            e1.record()
            e1.synchronize()
            t[k].append(e0.elapsed_time(e1) / a.batch)
    res["regrid"] = {k: _stat(v) for k, v in t.items()}
    res["regrid"]["nnz_per_row"] = {"unfilled": bil.nnz_per_row, "nearest": stod.nnz_per_row, "crept": crept.nnz_per_row}
    note("regrid: unfilled %.3f ms, nearest-filled %.3f ms, crept %.3f ms" % tuple(res["regrid"][k]["ms_median"] for k in ("unfilled", "nearest", "crept")))
    del x, outs
    for h in (crept, stod, bil):
        h.release()
    res["total_s"] = round(time.time() - t0, 1)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("%d cells (margin %g) under %d x %d mass points; %d levels in the Regrid.  Medians of %d calls.\n\n"
                    % (res["cells"], a.margin, g.nx, g.ny, nlev, a.reps))
            f.write("```json\n%s\n```\n" % json.dumps(res, indent=1))
    for o in (mesh, grid):
        o.destroy()
    _lib.finalize()


if __name__ == "__main__":
    main()
