#!/usr/bin/env python3
"""Nearest destination to source (mpg_regrid_store_nearest_dtos) at configuration 4's sizes, in ONE process on one card:

  cases    the 3.0 M-cell regional mesh and its 1800 x 1060 Lambert grid as SOURCES, binned onto a coarse verification grid (every
           --coarsen-th point of the Lambert grid in each direction: fine onto coarse, rows of hundreds of entries) and onto each other:
             cells -> coarse, vertices -> coarse, with --edges edges -> coarse (the Morton-ordered visit of a mesh's points),
             grid -> coarse (row-major ids as they are), grid -> cells and cells -> grid (about one source per destination).
           Per case --reps Stores, alternating over the cases: the GPU time of the call (mpg_handle_store_ms) as median, min and max,
           the sources mapped, the non-empty rows and the longest row, the wall time of the first call (it builds the tree).
  scale    beside each: mpg_handle_extrapolate NEAREST_STOD on the SAME point sets -- an all-but-empty handle whose rows are the DTOS
           sources, filled from the DTOS destinations: the same queries through the same tree, without the pattern passes -- and whether
           its ids equal nearest[].
  check    --check: rowptr / col / val / nearest of the --small cases against target_grid.nearest_dtos_rows (a brute-force mirror: small
           sizes only).

One JSON line; --out writes markdown too.  Run it under a time limit of its own:
    timeout -k 10 900 python tools/dtos_probe.py [--out profiles/r34_nearest_dtos_measured.md]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--coarsen", type=int, default=8, help="the verification grid keeps every n-th point of the Lambert grid")
    ap.add_argument("--small", action="store_true", help="the same cases at a size for a quick look (20 000 cells under 181 x 107)")
    ap.add_argument("--edges", action="store_true", help="derive the mesh's edges on the host (minutes at full size) and add edges -> coarse; --small implies it")
    ap.add_argument("--check", action="store_true", help="with --small: compare every case with the numpy mirror")
    ap.add_argument("--out", default=None, help="also write the record as markdown to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    from mpassit_amd import _lib, regrid as R, synth, target_grid as tg, workloads
    _lib.init(0)
    t0 = time.time()

    def note(what):
        print("[%6.1f s] %s" % (time.time() - t0, what), file=sys.stderr, flush=True)

    nxs, nys, ncells, over = (181, 107, 20000, dict(dx=30000.0, dy=30000.0)) if a.small else (1801, 1061, 3_000_000, {})
    g = workloads.conus_lambert_grid(nx=nxs, ny=nys, **over)
    m = synth.regional_mesh_for_lambert(g.proj, nxs, nys, ncells)
    if a.edges or a.small:
        m = synth.mesh_edges(m)
    k = max(1, a.coarsen)
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
    coarse = R.Grid(np.ascontiguousarray(g.lon[k // 2::k, k // 2::k]), np.ascontiguousarray(g.lat[k // 2::k, k // 2::k]))
    note("mesh (%d cells, %d vertices, %d edges), grid %d x %d, coarse %d x %d" % (mesh.nCells, mesh.nVertices, mesh.nEdges, grid.nx, grid.ny, coarse.nx, coarse.ny))
    E, N, ED, CEN = R.MESHLOC_ELEMENT, R.MESHLOC_NODE, R.MESHLOC_EDGE, R.STAGGERLOC_CENTER
    cases = {"cells -> coarse": (mesh, E, coarse, CEN), "vertices -> coarse": (mesh, N, coarse, CEN), "edges -> coarse": (mesh, ED, coarse, CEN),
             "grid -> coarse": (grid, CEN, coarse, CEN), "grid -> cells": (grid, CEN, mesh, E), "cells -> grid": (mesh, E, grid, CEN)}
    if mesh.nEdges == 0:
        del cases["edges -> coarse"]
    res = {"what": "dtos_probe", "cells": int(mesh.nCells), "grid": [grid.nx, grid.ny], "coarse": [coarse.nx, coarse.ny], "reps": a.reps, "cases": {}}
    times = {name: [] for name in cases}
    first = {}
    for rep in range(a.reps + 1):           # (the first round builds the trees and loads the code: kept apart)
        for name, (src, sloc, dst, dloc) in cases.items():
            torch.cuda.synchronize()
            w0 = time.time()
            rh = R.regrid_store_nearest_dtos(src, dst, R.DTOS_MEAN, None, None, sloc, dloc)
            wall = (time.time() - w0) * 1e3
            if rep == 0:
                st = rh.store_stats
                first[name] = {"n_src": rh.n_src, "n_dst": rh.n_dst, "mapped": st[1], "rows": st[2], "longest": st[3], "first_call_gpu_ms": round(rh.store_ms, 3),
                               "first_call_wall_ms": round(wall, 1)}
            else:
                times[name].append(rh.store_ms)
            rh.release()
    for name, (src, sloc, dst, dloc) in cases.items():
        v = sorted(times[name])
        c = dict(first[name])
        c.update(gpu_ms_median=round(v[len(v) // 2], 3), gpu_ms_min=round(v[0], 3), gpu_ms_max=round(v[-1], 3),
                 ns_per_source=round(v[len(v) // 2] * 1e6 / max(c["n_src"], 1), 2))
        # for scale: the same searches as mpg_handle_extrapolate NEAREST_STOD fills them (rows = the DTOS sources, candidates = its destinations)
        nd = dst.nCells if dst is mesh else dst.nx * dst.ny
        rows = (src.xyz(sloc).shape[1], 1) if src is mesh else (src.stagger_shape(sloc)[1], src.stagger_shape(sloc)[0])
        hole = R.RouteHandle.from_weights(nd, rows[0], rows[1], np.array([1], np.int32), np.array([1], np.int32), np.array([1.0]))
        ex = []
        for _ in range(a.reps):
            h = R.extrapolate(hole, dst, src, R.EXTRAPMETHOD_NEAREST_STOD, src_loc=dloc, dst_loc=sloc)
            ex.append(h.store_ms)
            last = h
            if len(ex) < a.reps:
                h.release()
        rh = R.regrid_store_nearest_dtos(src, dst, R.DTOS_SUM, None, None, sloc, dloc)
        rp, col, _ = last.csr() if last.nnz_per_row == 0 else (None, last.weights()[0][:, 0], None)
        ids = col if rp is None else col[rp[:-1]]
        near = rh.src_nearest()
        ex = sorted(ex)
        c.update(extrapolate_stod_ms_median=round(ex[len(ex) // 2], 3), extrapolate_stod_ms_min=round(ex[0], 3), extrapolate_stod_ms_max=round(ex[-1], 3),
                 ids_equal_from_row_1=bool(np.array_equal(ids[1:], near[1:])))
        if a.check and a.small:
            want = tg.nearest_dtos_rows(src.xyz(sloc), dst.xyz(dloc), tg.DTOS_SUM)
            got = rh.csr()
            c["mirror_equal"] = bool(all(np.array_equal(x, y) for x, y in zip(got, want[:3])) and np.array_equal(near, want[3]))
        for h in (last, rh, hole):
            h.release()
        res["cases"][name] = c
        note("%s: %d -> %d, %.3f ms (%.3f .. %.3f), longest row %d; extrapolate STOD %.3f ms" % (
            name, c["n_src"], c["n_dst"], c["gpu_ms_median"], c["gpu_ms_min"], c["gpu_ms_max"], c["longest"], c["extrapolate_stod_ms_median"]))
    res["total_s"] = round(time.time() - t0, 1)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("%d cells, grid %d x %d, coarse %d x %d; %d Stores per case after a first one.\n\n" % (res["cells"], grid.nx, grid.ny, coarse.nx, coarse.ny, a.reps))
            f.write("```json\n%s\n```\n" % json.dumps(res, indent=1))
    for o in (mesh, grid, coarse):
        o.destroy()
    _lib.finalize()


if __name__ == "__main__":
    main()
