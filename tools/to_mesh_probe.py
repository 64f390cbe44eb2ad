#!/usr/bin/env python3
"""Grid -> Mesh (mpg_regrid_store_to_mesh, mpg_regrid_to_mesh_dev) on configuration 4 turned round: the 1800 x 1060 CENTER points of the
3-km Lambert grid -> the 3.0 M-cell regional mesh, one field of 55 levels, float32, both destination layouts.  In ONE process:
    store           the bilinear Store through the inverse projection and through the pyramid (tune store_boxes 0), and the nearest Store
    to_mesh_cf      regrid_to_mesh into [lev][cell]
    to_mesh_lf      regrid_to_mesh into [cell][lev] (MPAS file order): the new kernel
    baseline_lf     what the library could do before for the same bytes: the same weights as a from-weights (CSR) handle through
                    regrid_typed into [lev][cell], then a device transposition (tensor.transpose(...).contiguous()) into [cell][lev]
    d2d_copy        a device-to-device copy of the result's size: the box's own copy rate, the yardstick of the fractions below
A timed block is --batch launches back to back between one pair of HIP events behind one untimed launch; the median per-call ms over --reps
blocks goes out with the algorithmic bytes  nlev * (U * 4 + P * 4) + P * 48  (U = the grid points the handle references, P = cells) as a
fraction of the measured copy rate, as one JSON line.  Run it under rocprofv3 --kernel-trace --stats for per-kernel times.
    python tools/to_mesh_probe.py [--reps 7] [--batch 3] [--warmup 2] [--nfields 1]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nfields", type=int, default=1)
    a = ap.parse_args()
    import time
    import numpy as np
    import torch
    from mpassit_amd import _lib, regrid as R, workloads
    _lib.init(0)
    t0 = time.time()
    m, g, nlev, desc = workloads.workload("c4_3m_regional")
    nf = a.nfields
    res = {"what": "to_mesh_probe", "workload": desc + ", turned round", "nfields": nf, "nlev": nlev}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        e0.record()
        for _ in range(a.batch):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.batch

    def median(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = sorted(timed(fn) for _ in range(a.reps))
        return ms[len(ms) // 2], ms[0], ms[-1]

    # ---- Stores: fresh grid / mesh objects per route, so that nothing comes from the handle cache -------------------------------------
    store = {}
    for name, boxes, method in (("bilinear_inverse", 1, R.REGRIDMETHOD_BILINEAR), ("bilinear_pyramid", 0, R.REGRIDMETHOD_BILINEAR),
                                ("nearest_inverse", 1, R.REGRIDMETHOD_NEAREST_STOD), ("nearest_pyramid", 0, R.REGRIDMETHOD_NEAREST_STOD)):
        ms = []
        for _ in range(3):
            mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_proj(g, fill_target=False)
            _lib.tune("store_boxes", boxes)
            try:
                h = R.regrid_store_to_mesh(grid, mesh, method)
            finally:
                _lib.tune("store_boxes", 1)
            ms.append(h.store_ms)
            path, stats = h.store_path, h.store_stats
            h.release()
            mesh.destroy()
            grid.destroy()
        store[name] = {"ms_first": round(ms[0], 3), "ms_later_min": round(min(ms[1:]), 3), "store_path": path, "fell_to_pyramid": stats[1]}
    res["store_ms"] = store

    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_proj(g, fill_target=False)
    rh = R.regrid_store_to_mesh(grid, mesh)
    U, P = int(rh.unique_sources().size), rh.n_dst
    idx, w = rh.weights()
    keep = idx >= 0
    row = np.broadcast_to(np.arange(1, P + 1, dtype=np.int32)[:, None], idx.shape)[keep]
    csr = R.RouteHandle.from_weights(rh.n_src, P, 1, row, idx[keep] + 1, w[keep])
    del idx, w, keep, row
    by = nf * nlev * (U * 4 + P * 4) + P * 48
    res.update({"n_src": rh.n_src, "n_dst": P, "unique_src": U, "alg_bytes": by, "setup_s": round(time.time() - t0, 1)})
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    src = torch.rand((nf, nlev, rh.n_src), dtype=torch.float32, device="cuda", generator=gen) - 0.5
    out_cf = torch.empty((nf, nlev, P), dtype=torch.float32, device="cuda")
    out_lf = torch.empty((nf, P, nlev), dtype=torch.float32, device="cuda")
    tmp = torch.empty((nf, nlev, 1, P), dtype=torch.float32, device="cuda")
    base_lf = torch.empty((nf, P, nlev), dtype=torch.float32, device="cuda")

    def baseline():
        csr.regrid_typed(src.reshape(-1), nlev=nlev, nfields=nf, out=tmp)
        base_lf.copy_(tmp.reshape(nf, nlev, P).transpose(1, 2))

    legs = {"to_mesh_cf": lambda: rh.regrid_to_mesh(src, nlev=nlev, nfields=nf, layout=R.LAYOUT_CELL_FAST, out=out_cf),
            "to_mesh_lf": lambda: rh.regrid_to_mesh(src, nlev=nlev, nfields=nf, layout=R.LAYOUT_LEV_FAST, out=out_lf),
            "baseline_lf": baseline,
            "d2d_copy": lambda: base_lf.copy_(out_lf)}
    legs["to_mesh_lf"]()
    baseline()
    torch.cuda.synchronize()
    res["lf_equals_baseline_values"] = bool(torch.allclose(out_lf, base_lf, rtol=0, atol=1e-5))   # (the CSR sum skips unmapped slots: same values)
    # interleaved rounds: every leg once per round, medians over the rounds
    for name, fn in legs.items():
        med, lo, hi = median(fn)
        res[name] = {"ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3)}
    copy_rate = 2 * out_lf.numel() * 4 / (res["d2d_copy"]["ms_median"] * 1e-3)   # bytes read + written per second
    res["d2d_copy"]["tb_s"] = round(copy_rate / 1e12, 3)
    for name in ("to_mesh_cf", "to_mesh_lf", "baseline_lf"):
        res[name]["alg_tb_s"] = round(by / (res[name]["ms_median"] * 1e-3) / 1e12, 3)
        res[name]["fraction_of_copy_rate"] = round(by / (res[name]["ms_median"] * 1e-3) / copy_rate, 3)
    res["lf_speedup_over_baseline"] = round(res["baseline_lf"]["ms_median"] / res["to_mesh_lf"]["ms_median"], 2)
    print(json.dumps(res), flush=True)
    csr.release()
    rh.release()
    mesh.destroy()
    grid.destroy()
    _lib.finalize()


if __name__ == "__main__":
    main()
