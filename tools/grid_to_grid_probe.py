#!/usr/bin/env python3
"""The Stores between two grids (mpg_regrid_store_grid_to_grid, mpg_regrid_store_conserve_grid_to_grid) at configuration 4's sizes, in ONE
process on one card: the 1800 x 1060 Lambert grid against a 0.03-degree lat-lon grid of similar point count over the same region, both ways.

  stores     GPU time of each Store (mpg_handle_store_ms) on FRESH grids per repetition, so that nothing comes from the handle cache or from
             a pyramid built earlier: bilinear by the index route (the source from its projection), bilinear by the pyramid walk
             (mpg_tune("store_boxes", 0)), nearest, conservative.  The median of --reps Stores with min and max, after one that loads the module.
  regrid     regrid_typed of 55 levels, float32 and float64, through the bilinear and the conservative handle: per-call ms, the median of
             --reps batches with min and max.
  yardstick  (--mesh) on a regional mesh of the destination's point count under the same source grid: regrid_store_to_mesh (bilinear,
             nearest), regrid_store_conserve_to_mesh and regrid_to_mesh of 55 levels -- the calls whose search code the new Stores share.
             For orientation, not a bar.

One JSON line; --out writes markdown too.  Run it under a time limit of its own:
    timeout -k 10 900 python tools/grid_to_grid_probe.py [--mesh] [--out profiles/r33_grid_to_grid_measured.md]"""
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
    ap.add_argument("--small", action="store_true", help="the same at a size for a quick look (180 x 106 against 0.3 degrees)")
    ap.add_argument("--mesh", action="store_true", help="also the Grid -> Mesh yardsticks (builds a mesh of the destination's point count)")
    ap.add_argument("--out", default=None, help="also write the record as markdown to this file")
    a = ap.parse_args()
    import torch
    from mpassit_amd import _lib, regrid as R, synth, target_grid as tg, workloads
    _lib.init(0)
    t0 = time.time()

    def note(what):
        print("[%6.1f s] %s" % (time.time() - t0, what), file=sys.stderr, flush=True)

    nxs, nys, over, dll = (181, 107, dict(dx=30000.0, dy=30000.0), 0.3) if a.small else (1801, 1061, {}, 0.03)
    nlev = 55
    lam = workloads.conus_lambert_grid(nx=nxs, ny=nys, **over)
    lat0, lat1, lon0, lon1 = float(lam.lat_c.min()), float(lam.lat_c.max()), float(lam.lon_c.min()), float(lam.lon_c.max())
    # the lat-lon grid covers the Lambert grid's bounding box, shifted off its lines by an odd fraction of a cell
    nlon, nlat = int((lon1 - lon0) / dll) + 2, int((lat1 - lat0) / dll) + 2
    ll = tg.define_target_grid_params("lat-lon", nlon, nlat, dx=dll, dy=dll, ref_lat=0.5 * (lat0 + lat1) + 0.37 * dll, ref_lon=0.5 * (lon0 + lon1) + 0.13 * dll)
    targets = {"lambert": lam, "latlon": ll}
    res = {"what": "grid_to_grid_probe", "lambert": [lam.nx, lam.ny], "latlon": [ll.nx, ll.ny], "dll_deg": dll, "nlev": nlev, "reps": a.reps}
    note("grids: Lambert %d x %d, lat-lon %d x %d" % (lam.nx, lam.ny, ll.nx, ll.ny))

    def store_times(make):
        """make(src_grid, dst_grid) -> handle, on fresh grids each time -> (the record, counts of the last handle)"""
        def run(s, d):
            ms, info = [], None
            for _ in range(a.reps + 1):
                gs, gd = R.Grid.from_target(targets[s]), R.Grid.from_target(targets[d])
                rh = make(gs, gd)
                ms.append(rh.store_ms)
                info = dict(n_src=rh.n_src, n_dst=rh.n_dst, nnz=rh.nnz, store_path=rh.store_path, stats=[int(x) for x in rh.store_stats[1:7]])
                rh.release()
                gs.destroy()
                gd.destroy()
            return dict(_stat(ms[1:]), first_ms=round(ms[0], 3), **info)
        return {"lambert_to_latlon": run("lambert", "latlon"), "latlon_to_lambert": run("latlon", "lambert")}

    res["store_bilinear_index"] = store_times(lambda s, d: R.regrid_store_grid_to_grid(s, d))
    note("bilinear, index route")
    _lib.tune("store_boxes", 0)
    try:
        res["store_bilinear_walk"] = store_times(lambda s, d: R.regrid_store_grid_to_grid(s, d))
    finally:
        _lib.tune("store_boxes", 1)
    note("bilinear, pyramid walk")
    res["store_nearest"] = store_times(lambda s, d: R.regrid_store_grid_to_grid(s, d, R.REGRIDMETHOD_NEAREST_STOD))
    note("nearest")
    res["store_conserve"] = store_times(lambda s, d: R.regrid_store_conserve_grid_to_grid(s, d))
    note("conservative")

    def regrid_times(rh, call):
        out = {}
        for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
            src = torch.rand(nlev * rh.n_src, dtype=dt, device="cuda")
            call(rh, src)
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.batch):
                    call(rh, src)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / a.batch)
            out[name] = _stat(ms)
        return out

    glam, gll = R.Grid.from_target(lam), R.Grid.from_target(ll)
    typed = lambda rh, src: rh.regrid_typed(src, nlev=nlev)   # noqa: E731
    for tag, (s, d) in (("lambert_to_latlon", (glam, gll)), ("latlon_to_lambert", (gll, glam))):
        for kind, make in (("bilinear", R.regrid_store_grid_to_grid), ("conserve", R.regrid_store_conserve_grid_to_grid)):
            rh = make(s, d)
            res.setdefault("regrid_typed_" + kind, {})[tag] = regrid_times(rh, typed)
            rh.release()
    note("Regrids")
    if a.mesh:
        n_pts = ll.nx * ll.ny
        m = synth.regional_mesh_for_lambert(lam.proj, nxs, nys, n_pts, margin=0.0)
        mesh = R.Mesh.from_mpas(m)
        note("mesh of %d cells" % m.nCells)
        y = {"cells": int(m.nCells)}
        for name in ("store_to_mesh_bilinear", "store_to_mesh_nearest", "store_conserve_to_mesh"):
            ms = []
            for _ in range(a.reps + 1):
                gs, ms_mesh = R.Grid.from_target(lam), R.Mesh.from_mpas(m)
                rh = {"store_to_mesh_bilinear": lambda: R.regrid_store_to_mesh(gs, ms_mesh),
                      "store_to_mesh_nearest": lambda: R.regrid_store_to_mesh(gs, ms_mesh, R.REGRIDMETHOD_NEAREST_STOD),
                      "store_conserve_to_mesh": lambda: R.regrid_store_conserve_to_mesh(gs, ms_mesh)}[name]()
                ms.append(rh.store_ms)
                rh.release()
                gs.destroy()
                ms_mesh.destroy()
            y[name] = dict(_stat(ms[1:]), first_ms=round(ms[0], 3))
        rh = R.regrid_store_to_mesh(glam, mesh)
        y["regrid_to_mesh"] = regrid_times(rh, lambda h, src: h.regrid_to_mesh(src, nlev=nlev))
        rh.release()
        mesh.destroy()
        res["yardstick_grid_to_mesh"] = y
        note("yardsticks")
    glam.destroy()
    gll.destroy()
    res["wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write("# Grid -> Grid Stores at configuration 4's sizes (tools/grid_to_grid_probe.py)\n\n")
            f.write("Lambert %d x %d against lat-lon %d x %d (%.3g degrees), %d levels; medians of %d with min and max, GPU ms.\n\n" % (
                lam.nx, lam.ny, ll.nx, ll.ny, dll, nlev, a.reps))
            for key, val in res.items():
                if isinstance(val, dict):
                    f.write("## %s\n\n```json\n%s\n```\n\n" % (key, json.dumps(val, indent=1)))
    _lib.finalize()


if __name__ == "__main__":
    main()
