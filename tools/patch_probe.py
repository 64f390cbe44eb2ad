#!/usr/bin/env python3
"""Patch regridding (mpg_handle_patch) at configuration 4's sizes, in ONE process on one card: the 3.0 M-cell regional mesh onto its
1800 x 1060 Lambert grid.

  store    the bilinear Store, then mpg_handle_patch on its handle: GPU time of the call (mpg_handle_store_ms), the median of --reps calls
           with min and max; rows written, (row, slot) pairs per attempt, entries per row, the longest row.
  regrid   55 levels, float32, through the patch handle (CSR) beside the bilinear handle (fixed, 3 slots), alternating, level-fast
           sources ([cell][lev], file order) and cell-fast ones ([lev][cell]): the median per-call ms with min and max, and the bytes moved.
  copy     the card's device-to-device copy rate on 1 GiB, the yardstick for both.

One JSON line; --out writes markdown too.  Run it under a time limit of its own:
    timeout -k 10 900 python tools/patch_probe.py [--out profiles/r29_patch_measured.md]"""
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
    ap.add_argument("--small", action="store_true", help="the same at a size for a quick look (20 000 cells under 181 x 107)")
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
    m = synth.regional_mesh_for_lambert(g.proj, nxs, nys, ncells)
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
    note("mesh (%d cells) and grid (%d x %d mass points)" % (m.nCells, g.nx, g.ny))
    res = {"what": "patch_probe", "cells": int(m.nCells), "grid": [g.nx, g.ny], "nlev": nlev}

    bil = R.regrid_store(mesh, grid, R.REGRIDMETHOD_BILINEAR)
    ms, wall, out = [], [], None
    for _ in range(a.reps + 1):                      # the first call loads the module: not counted
        if out is not None:
            out.release()
        torch.cuda.synchronize()
        w0 = time.time()
        out = R.patch(bil, mesh, grid)
        wall.append((time.time() - w0) * 1e3)
        ms.append(out.store_ms)
    st = out.store_stats
    res["store"] = {"bilinear_store_ms": round(bil.store_ms, 3), "patch": _stat(ms[1:]), "patch_first_call_ms": round(ms[0], 3),
                    "patch_wall_ms_median": round(sorted(wall[1:])[len(wall[1:]) // 2], 2), "rows": bil.n_dst, "rows_written": st[1],
                    "pairs_A_B_C_D": st[2:6], "longest_row": st[6], "nnz": out.nnz, "entries_per_written_row": round(out.nnz / max(st[1], 1), 3),
                    "ns_per_written_row": round(sorted(ms[1:])[len(ms[1:]) // 2] * 1e6 / max(st[1], 1), 2)}
    note("patch: %.3f ms (bilinear Store %.3f ms), %.2f entries per row, longest %d" % (res["store"]["patch"]["ms_median"], bil.store_ms,
                                                                                      res["store"]["entries_per_written_row"], st[6]))

    x = torch.randn((m.nCells, nlev), dtype=torch.float32, device="cuda")
    xc = x.t().contiguous()                            # the same values [lev][cell]
    outs = {k: torch.empty((1, nlev, g.ny, g.nx), dtype=torch.float32, device="cuda") for k in ("bilinear", "patch")}
    routes = {"bilinear": lambda: bil.regrid_typed(x, nlev=nlev, layout=R.LAYOUT_LEV_FAST, out=outs["bilinear"]),
              "patch": lambda: out.regrid_typed(x, nlev=nlev, layout=R.LAYOUT_LEV_FAST, out=outs["patch"]),
              "bilinear_cell_fast": lambda: bil.regrid_typed(xc, nlev=nlev, layout=R.LAYOUT_CELL_FAST, out=outs["bilinear"]),
              "patch_cell_fast": lambda: out.regrid_typed(xc, nlev=nlev, layout=R.LAYOUT_CELL_FAST, out=outs["patch"])}
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
    routes["bilinear"](), routes["patch"]()           # the comparison below reads the level-fast results
    moved = 4 * nlev * (m.nCells + bil.n_dst)         # every source and every destination value once
    res["regrid"]["field_bytes"] = moved
    res["regrid"]["pattern_bytes"] = {"bilinear": 3 * 12 * bil.n_dst, "patch": 12 * out.nnz + 4 * (out.n_dst + 1)}
    for k in routes:
        res["regrid"][k]["field_GBps"] = round(moved / (res["regrid"][k]["ms_median"] * 1e6), 1)
    mapped = torch.from_numpy((bil.weights()[0][:, 0] >= 0).reshape(g.ny, g.nx)).cuda()
    d = (outs["patch"][0][:, mapped] - outs["bilinear"][0][:, mapped]).abs().max().item()
    res["regrid"]["max_abs_difference_on_white_noise"] = round(d, 4)
    note("regrid: bilinear %.3f ms, patch %.3f ms" % (res["regrid"]["bilinear"]["ms_median"], res["regrid"]["patch"]["ms_median"]))
    del x, outs
    out.release()
    bil.release()

    n = 1 << 28
    src, dst = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
    dst.copy_(src)
    torch.cuda.synchronize()
    c = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        c.append(e0.elapsed_time(e1))
    res["copy"] = {"bytes_read_plus_written": 8 * n, "ms_median": round(sorted(c)[len(c) // 2], 3),
                   "GBps": round(8 * n / (sorted(c)[len(c) // 2] * 1e6), 1)}
    res["total_s"] = round(time.time() - t0, 1)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("%d cells under %d x %d mass points; %d levels; medians of %d.\n\n" % (res["cells"], g.nx, g.ny, nlev, a.reps))
            f.write("```json\n%s\n```\n" % json.dumps(res, indent=1))
    for o in (mesh, grid):
        o.destroy()
    _lib.finalize()


if __name__ == "__main__":
    main()
