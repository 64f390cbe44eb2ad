#!/usr/bin/env python3
"""Conservative Grid -> Mesh (mpg_regrid_store_conserve_to_mesh, mpg_regrid_csr_to_mesh_dev) on configuration 4 turned round: the
1800 x 1060 cells of the 3-km Lambert grid -> the 3.0 M-cell regional mesh, one field of 55 levels, float32 and float64.  In ONE process:
    store           the conservative Store through the index boxes and through the pyramid walk (tune store_boxes 0)
    csr_lf          regrid_csr_to_mesh into [cell][lev] (MPAS file order): the new kernel
    baseline_lf     the only route to those bytes before: regrid_typed on the same handle into [lev][cell], then a device transposition
    csr_cf          regrid_csr_to_mesh into [lev][cell]
    typed_cf        regrid_typed on the same handle (k_apply_generic_t, NNZ = 0): the kernel csr_cf must not lose to by more than 10 %
    d2d_copy        a device-to-device copy of the result's size: the box's own copy rate, the yardstick of the fractions below
A timed block is --batch launches back to back between one pair of HIP events behind one untimed launch; the median per-call ms over --reps
blocks goes out with the algorithmic bytes  nlev * (U + P) * elem + nnz * 12 + P * 4  (U = the grid cells the handle references, P = mesh
cells) as a fraction of the measured copy rate, as one JSON line.  Run it under rocprofv3 --kernel-trace --stats for per-kernel times.
    python tools/conserve_to_mesh_probe.py [--reps 7] [--batch 3] [--warmup 2] [--dtypes f32,f64] [--stores 3]"""
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
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--stores", type=int, default=3)
    a = ap.parse_args()
    import time
    import torch
    from mpassit_amd import _lib, regrid as R, workloads
    _lib.init(0)
    t0 = time.time()
    m, g, nlev, desc = workloads.workload("c4_3m_regional")
    res = {"what": "conserve_to_mesh_probe", "workload": desc + ", turned round", "nlev": nlev, "device": _lib.device_info()[0]}

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
    for name, boxes in (("index_boxes", 1), ("pyramid", 0)):
        ms = []
        for _ in range(a.stores):
            mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_proj(g, fill_target=False)
            _lib.tune("store_boxes", boxes)
            try:
                h = R.regrid_store_conserve_to_mesh(grid, mesh)
            finally:
                _lib.tune("store_boxes", 1)
            ms.append(h.store_ms)
            path, stats, nnz = h.store_path, h.store_stats, h.nnz
            h.release()
            mesh.destroy()
            grid.destroy()
        store[name] = {"ms_first": round(ms[0], 3), "ms_later_min": round(min(ms[1:]) if len(ms) > 1 else ms[0], 3), "store_path": path,
                       "pairs_clipped": int(stats[1]), "nnz": int(nnz)}
    res["store_ms"] = store

    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_proj(g, fill_target=False)
    rh = R.regrid_store_conserve_to_mesh(grid, mesh)
    U, P, nnz = int(rh.unique_sources().size), rh.n_dst, rh.nnz
    res.update({"n_src": rh.n_src, "n_dst": P, "unique_src": U, "nnz": nnz, "setup_s": round(time.time() - t0, 1)})
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    for name in a.dtypes.split(","):
        dt = torch.float32 if name == "f32" else torch.float64
        es = 4 if name == "f32" else 8
        by = nlev * (U + P) * es + nnz * 12 + P * 4
        src = (torch.rand((1, nlev, rh.n_src), dtype=torch.float64, device="cuda", generator=gen) - 0.5).to(dt)
        out_cf = torch.empty((1, nlev, P), dtype=dt, device="cuda")
        out_lf = torch.empty((1, P, nlev), dtype=dt, device="cuda")
        tmp = torch.empty((1, nlev, 1, P), dtype=dt, device="cuda")
        base_lf = torch.empty((1, P, nlev), dtype=dt, device="cuda")

        def baseline():
            rh.regrid_typed(src.reshape(-1), nlev=nlev, out=tmp)
            base_lf.copy_(tmp.reshape(1, nlev, P).transpose(1, 2))

        legs = {"csr_lf": lambda: rh.regrid_csr_to_mesh(src, nlev=nlev, layout=R.LAYOUT_LEV_FAST, out=out_lf),
                "baseline_lf": baseline,
                "csr_cf": lambda: rh.regrid_csr_to_mesh(src, nlev=nlev, layout=R.LAYOUT_CELL_FAST, out=out_cf),
                "typed_cf": lambda: rh.regrid_typed(src.reshape(-1), nlev=nlev, out=tmp),
                "d2d_copy": lambda: base_lf.copy_(out_lf)}
        legs["csr_lf"]()
        legs["csr_cf"]()
        baseline()
        torch.cuda.synchronize()
        r = {"alg_bytes": by, "lf_equals_baseline_bytes": bool(torch.equal(out_lf, base_lf)),
             "cf_equals_typed_bytes": bool(torch.equal(out_cf.reshape(-1), tmp.reshape(-1)))}
        for leg, fn in legs.items():
            med, lo, hi = median(fn)
            r[leg] = {"ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3)}
        copy_rate = 2 * out_lf.numel() * es / (r["d2d_copy"]["ms_median"] * 1e-3)   # bytes read + written per second
        r["d2d_copy"]["tb_s"] = round(copy_rate / 1e12, 3)
        for leg in ("csr_lf", "baseline_lf", "csr_cf", "typed_cf"):
            r[leg]["alg_tb_s"] = round(by / (r[leg]["ms_median"] * 1e-3) / 1e12, 3)
            r[leg]["fraction_of_copy_rate"] = round(by / (r[leg]["ms_median"] * 1e-3) / copy_rate, 3)
        r["lf_speedup_over_baseline"] = round(r["baseline_lf"]["ms_median"] / r["csr_lf"]["ms_median"], 2)
        r["cf_time_over_typed"] = round(r["csr_cf"]["ms_median"] / r["typed_cf"]["ms_median"], 3)
        res[name] = r
        del src, out_cf, out_lf, tmp, base_lf
    print(json.dumps(res), flush=True)
    rh.release()
    mesh.destroy()
    grid.destroy()
    _lib.finalize()


if __name__ == "__main__":
    main()
