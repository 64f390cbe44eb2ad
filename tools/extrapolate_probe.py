#!/usr/bin/env python3
"""Extrapolation (mpg_handle_extrapolate) at configuration 4's sizes, in ONE process on one card:

  fill     the 3.0 M-cell regional mesh under its Lambert grid ENLARGED (--grow points on every side) until about a tenth of the grid points
           lie outside the mesh: the bilinear Mesh -> Grid handle filled nearest-source-to-destination (stays fixed, 3 slots) and with
           the inverse-distance average of N = 8 (becomes CSR).  GPU time of the call (mpg_handle_store_ms) and wall time, twice each.
  yardstick  the nearest Store of the same mesh and grid with "store_boxes" 0: it walks the same tree for EVERY grid point with K = 1, so
           the comparison is per searched point.
  regrid   55 levels, float32, through the filled fixed handle against the unfilled one, alternating: the kernel choice of both and the
           median per-call ms with min and max.
  winds    configuration 4's two destagger handles (CENTER -> EDGE1 / EDGE2 of its own grid) filled nearest-source-to-destination.

--pow-ulp  instead of all that: the ulp error of the DEVICE pow (torch.pow on float64 CUDA tensors -- the platform's pow, not this library)
           over r_i = d2_0 / d2_i of the small pairings tests/test_extrapolate_gpu.py uses, exponents e / 2 for e in {1.0, 3.5}, against
           mpmath at 50 digits.  The bound B of that test is this figure rounded up.

One JSON line; --out writes markdown too.  Run it under a time limit of its own:
    timeout -k 10 900 python tools/extrapolate_probe.py [--out profiles/r27_extrapolate_measured.md]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAMBERT = dict(ref_lat=38.5, ref_lon=-97.5, truelat1=38.5, truelat2=38.5, stand_lon=-97.5)


def pow_ulp():
    import mpmath
    import numpy as np
    import torch
    from mpassit_amd import regrid as R, synth, target_grid as tg
    mpmath.mp.dps = 50
    g = tg.define_target_grid_params("lambert", 61, 41, dx=30000.0, dy=30000.0, **LAMBERT)
    m_in = synth.regional_mesh_for_lambert(g.proj, 61, 41, 5003, margin=-0.08, seed=12)
    m_over = synth.regional_mesh_for_lambert(g.proj, 61, 41, 6001, margin=0.05, seed=11)
    grid, mesh_in, mesh_over = R.Grid.from_target(g), R.Mesh.from_mpas(m_in), R.Mesh.from_mpas(m_over)
    cases = (("mesh to grid", R.regrid_store(mesh_in, grid), mesh_in.xyz(), grid.xyz()),
             ("mesh to mesh", R.regrid_store_mesh(mesh_in, mesh_over), mesh_in.xyz(), mesh_over.xyz()),
             ("grid to mesh", R.regrid_store_to_mesh(grid, mesh_over), grid.xyz(), mesh_over.xyz()),
             ("centre to edge1", R.regrid_store_grid(grid, R.STAGGERLOC_EDGE1), grid.xyz(), grid.xyz(R.STAGGERLOC_EDGE1)),
             ("centre to edge2", R.regrid_store_grid(grid, R.STAGGERLOC_EDGE2), grid.xyz(), grid.xyz(R.STAGGERLOC_EDGE2)))
    res = {"what": "device pow against mpmath, in ulp of the exact value", "cases": []}
    worst = 0.0
    for name, rh, sxyz, dxyz in cases:
        rows = np.flatnonzero(rh.weights()[0][:, 0] < 0)
        _, d2 = tg.extrapolate_neighbours(sxyz, dxyz, rows, 8)
        r = (d2[:, :1] / d2).reshape(-1)
        for e in (1.0, 3.5):
            got = torch.pow(torch.from_numpy(r).cuda(), 0.5 * e).cpu().numpy()
            err = 0.0
            for x, y in zip(r.tolist(), got.tolist()):
                exact = mpmath.power(mpmath.mpf(x), mpmath.mpf(e) / 2)
                ulp = float(np.spacing(float(exact)))
                err = max(err, float(abs(mpmath.mpf(y) - exact)) / ulp)
            res["cases"].append({"case": name, "e": e, "values": int(r.size), "max_ulp": round(err, 4)})
            worst = max(worst, err)
        rh.release()
    res["max_ulp"] = round(worst, 4)
    res["B"] = int(np.ceil(worst)) if worst > 0 else 1
    for x in (grid, mesh_in, mesh_over):
        x.destroy()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pow-ulp", action="store_true")
    ap.add_argument("--grow", type=int, default=110, help="grid points added on every side of configuration 4's grid")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="the same cases at a size for a quick look (20 000 cells under 181 x 107)")
    ap.add_argument("--out", default=None, help="also write the record as markdown to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    from mpassit_amd import _lib, regrid as R, synth, workloads
    _lib.init(0)
    if a.pow_ulp:
        res = pow_ulp()
        print(json.dumps(res), flush=True)
        _lib.finalize()
        return
    t0 = time.time()

    def note(what):
        print("[%6.1f s] %s" % (time.time() - t0, what), file=sys.stderr, flush=True)

    nxs, nys, ncells, over = (181, 107, 20000, dict(dx=30000.0, dy=30000.0)) if a.small else (1801, 1061, 3_000_000, {})
    grow = max(1, a.grow // 10) if a.small else a.grow
    g0 = workloads.conus_lambert_grid(nx=nxs, ny=nys, **over)
    g = workloads.conus_lambert_grid(nx=nxs + 2 * grow, ny=nys + 2 * grow, **over)
    m = synth.regional_mesh_for_lambert(g0.proj, nxs, nys, ncells)
    nlev = 55
    mesh, grid, grid0 = R.Mesh.from_mpas(m), R.Grid.from_target(g), R.Grid.from_target(g0)
    note("mesh (%d cells), the grid enlarged to %d x %d mass points and configuration 4's own" % (m.nCells, g.nx, g.ny))
    res = {"what": "extrapolate_probe", "cells": int(m.nCells), "grid": [g.nx, g.ny], "nlev": nlev}

    def fill(rh, src, dst, method, N, **loc):
        out = []
        for _ in range(2):
            torch.cuda.synchronize()
            w0 = time.time()
            h = R.extrapolate(rh, src, dst, method, N, 2.0, **loc)
            out.append({"gpu_ms": round(h.store_ms, 3), "wall_ms": round((time.time() - w0) * 1e3, 1), "rows_filled": h.store_stats[1], "K": h.store_stats[2],
                        "nnz_per_row": h.nnz_per_row, "nnz": h.nnz})
            if len(out) < 2:
                h.release()
        return h, out

    bil = R.regrid_store(mesh, grid, R.REGRIDMETHOD_BILINEAR)
    stod, t_stod = fill(bil, mesh, grid, R.EXTRAPMETHOD_NEAREST_STOD, 1)
    idavg, t_idavg = fill(bil, mesh, grid, R.EXTRAPMETHOD_NEAREST_IDAVG, 8)
    nu = t_stod[0]["rows_filled"]
    res["fill"] = {"points": bil.n_dst, "unmapped": nu, "share": round(nu / bil.n_dst, 4), "bilinear_store_ms": round(bil.store_ms, 3), "stod": t_stod, "idavg8": t_idavg,
                   "stod_ns_per_row": round(t_stod[1]["gpu_ms"] * 1e6 / max(nu, 1), 2), "idavg8_ns_per_row": round(t_idavg[1]["gpu_ms"] * 1e6 / max(nu, 1), 2)}
    note("fill: %d of %d unmapped; STOD %.3f ms, IDAVG 8 %.3f ms (second calls)" % (nu, bil.n_dst, t_stod[1]["gpu_ms"], t_idavg[1]["gpu_ms"]))
    _lib.tune("store_boxes", 0)
    near = R.regrid_store(mesh, grid, R.REGRIDMETHOD_NEAREST_STOD)
    _lib.tune("store_boxes", 1)
    res["yardstick"] = {"nearest_store_boxes_0_ms": round(near.store_ms, 3), "points": near.n_dst, "ns_per_point": round(near.store_ms * 1e6 / near.n_dst, 2)}
    same = bool(np.array_equal(near.weights()[0][:, 0][bil.weights()[0][:, 0] < 0], stod.weights()[0][:, 0][bil.weights()[0][:, 0] < 0]))
    res["yardstick"]["stod_ids_equal_the_nearest_store"] = same
    note("yardstick: nearest Store with store_boxes 0 %.3f ms for %d points" % (near.store_ms, near.n_dst))
    near.release()

    x = torch.randn((m.nCells, nlev), dtype=torch.float32, device="cuda")
    outs = {k: torch.empty((1, nlev, g.ny, g.nx), dtype=torch.float32, device="cuda") for k in ("unfilled", "filled")}
    routes = {"unfilled": lambda: bil.regrid_typed(x, nlev=nlev, layout=R.LAYOUT_LEV_FAST, out=outs["unfilled"]),
              "filled": lambda: stod.regrid_typed(x, nlev=nlev, layout=R.LAYOUT_LEV_FAST, out=outs["filled"])}
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
    res["regrid"] = {k: {"ms_median": round(sorted(v)[len(v) // 2], 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)} for k, v in t.items()}
    res["regrid"]["kernel_choice"] = {"unfilled": list(bil.kernel_choice()), "filled": list(stod.kernel_choice())}
    mapped = (bil.weights()[0][:, 0] >= 0).reshape(g.ny, g.nx)
    res["regrid"]["mapped_points_equal"] = bool(torch.equal(outs["unfilled"][0][:, torch.from_numpy(mapped).cuda()], outs["filled"][0][:, torch.from_numpy(mapped).cuda()]))
    note("regrid: unfilled %.3f ms, filled %.3f ms" % (res["regrid"]["unfilled"]["ms_median"], res["regrid"]["filled"]["ms_median"]))
    del x, outs
    for h in (stod, idavg, bil):
        h.release()

    res["winds"] = {}
    for name, st in (("edge1", R.STAGGERLOC_EDGE1), ("edge2", R.STAGGERLOC_EDGE2)):
        rh = R.regrid_store_grid(grid0, st)
        h, tt = fill(rh, grid0, grid0, R.EXTRAPMETHOD_NEAREST_STOD, 1, dst_loc=st)
        res["winds"][name] = {"points": rh.n_dst, "store_ms": round(rh.store_ms, 3), "stod": tt}
        note("%s: %d of %d filled in %.3f ms" % (name, tt[1]["rows_filled"], rh.n_dst, tt[1]["gpu_ms"]))
        h.release()
        rh.release()
    res["total_s"] = round(time.time() - t0, 1)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("%d cells under %d x %d mass points; %d levels.  Second calls where two are listed.\n\n" % (res["cells"], g.nx, g.ny, nlev))
            f.write("```json\n%s\n```\n" % json.dumps(res, indent=1))
    for o in (mesh, grid, grid0):
        o.destroy()
    _lib.finalize()


if __name__ == "__main__":
    main()
