#!/usr/bin/env python3
"""Dense against pitched destinations, in one process: the odd grid x_c4_1799x1059 (1799 x 1059 mass points, every dense level plane
off a 128-byte line) and its control c4_3m_regional (1800 x 1060: dense planes on lines already), 55 levels.  For each grid, three legs:
  f32be_file_order  float32 big-endian file order -> float32 big-endian (the driver's Regrid: k_apply3_lf_rows)
  f64_cell_fast     float64 cell-fast -> float64 (the headline kernel: k_apply3_cfu)
  wind_f32be        the rotated wind chain, float32 big-endian U / V (k_wind_destagger)
Dense and pitched blocks alternate (--reps blocks each, after --warmup): a block is --batch launches back to back between one pair of
HIP events, behind one untimed launch that keeps the GPU busy while the first event is recorded -- so the host time of the Python call
(larger for a pitched `out`, whose strides are checked) stays hidden behind the queue and a block's time is the kernels' own.  The median
per-launch ms and the fraction of the 8 TB/s peak of its algorithmic bytes (regrid.ACCOUNT, the bench's count) go out as one JSON line.
For a per-kernel trace, --grid and --only run one grid and one form (separate rocprofv3 --kernel-trace --stats runs).
    python tools/pitch_probe.py [--reps 10] [--batch 20] [--warmup 3] [--grid odd|control] [--only dense|pitched]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--grid", choices=["odd", "control"], default=None)
    ap.add_argument("--only", choices=["dense", "pitched"], default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from mpassit_amd import _lib, regrid as R, workloads
    _lib.init(0)
    result = {"what": "pitch_probe", "reps": a.reps, "batch": a.batch, "peak_tb_s": PEAK / 1e12, "only": a.only}

    def timed(fn):   # ms per launch of a block of back-to-back launches
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()                       # untimed: the GPU is busy when e0 is recorded, and the timed launches queue up behind it
        e0.record()
        for _ in range(a.batch):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.batch

    def nbytes(fn):
        R.ACCOUNT = []
        fn()
        torch.cuda.synchronize()
        b = sum(x[1] for x in R.ACCOUNT)
        R.ACCOUNT = None
        return b

    def leg(dense_fn, pitched_fn):
        by = nbytes(dense_fn)
        fns = {"dense": dense_fn, "pitched": pitched_fn}
        if a.only:
            fns = {a.only: fns[a.only]}
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
        ts = {k: [] for k in fns}
        for _ in range(a.reps):            # alternating blocks: both forms see the same clocks and the same neighbours
            for k, fn in fns.items():
                ts[k].append(timed(fn))
        res = {"bytes": int(by)}
        for k, t in ts.items():
            med = float(np.median(t))
            res[k + "_ms"] = round(med, 4)
            res[k + "_frac"] = round(by / (med * 1e-3) / PEAK, 4)
        return res

    names = {"odd": "x_c4_1799x1059", "control": "c4_3m_regional"}
    for name in ([names[a.grid]] if a.grid else list(names.values())):
        m, g, nlev, _ = workloads.workload(name)
        mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
        rh = R.regrid_store(mesh, grid, R.REGRIDMETHOD_BILINEAR)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(55)
        s64 = (torch.rand((nlev, m.nCells), dtype=torch.float64, device="cuda", generator=gen) - 0.5) * 60.0
        lf32 = s64.t().contiguous().to(torch.float32).view(-1)       # file order; the bytes' order does not change the work
        out = {"grid": "%dx%d" % (g.nx, g.ny), "nlev": nlev, "plane_points": g.nx * g.ny,
               "ld_f32": rh.level_stride(torch.float32), "ld_f64": rh.level_stride(torch.float64)}
        be = dict(nlev=nlev, layout=R.LAYOUT_LEV_FAST, out_dtype=torch.float32, src_be=True, dst_be=True)
        d32, p32 = torch.empty((1, nlev, g.ny, g.nx), dtype=torch.float32, device="cuda"), rh.empty_pitched(nlev, dtype=torch.float32)
        out["f32be_file_order"] = leg(lambda: rh.regrid_typed(lf32, out=d32, **be), lambda: rh.regrid_typed(lf32, out=p32, **be))
        del d32, p32
        d64, p64 = torch.empty((1, nlev, g.ny, g.nx), dtype=torch.float64, device="cuda"), rh.empty_pitched(nlev, dtype=torch.float64)
        s = s64.view(-1)
        out["f64_cell_fast"] = leg(lambda: rh.regrid(s, nlev=nlev, out=d64), lambda: rh.regrid(s, nlev=nlev, out=p64))
        out["kernel_choice"] = rh.kernel_choice()
        del d64, p64
        rh.release()
        # the wind chain: mass winds on the CENTER stagger, U / V float32 big-endian
        rh_u, rh_v = R.regrid_store_grid(grid, R.STAGGERLOC_EDGE1), R.regrid_store_grid(grid, R.STAGGERLOC_EDGE2)
        um = (torch.rand((nlev, g.ny, g.nx), dtype=torch.float64, device="cuda", generator=gen) - 0.5) * 40.0
        vm = (torch.rand((nlev, g.ny, g.nx), dtype=torch.float64, device="cuda", generator=gen) - 0.5) * 40.0
        ca = torch.as_tensor(np.ascontiguousarray(g.cosa), device="cuda")
        sa = torch.as_tensor(np.ascontiguousarray(g.sina), device="cuda")
        ld = max(rh_u.level_stride(torch.float32), rh_v.level_stride(torch.float32))
        pu = torch.empty(nlev * ld, dtype=torch.float32, device="cuda").as_strided((nlev, rh_u.ny_dst, rh_u.nx_dst), (ld, rh_u.nx_dst, 1))
        pv = torch.empty(nlev * ld, dtype=torch.float32, device="cuda").as_strided((nlev, rh_v.ny_dst, rh_v.nx_dst), (ld, rh_v.nx_dst, 1))
        du = torch.empty((nlev, rh_u.ny_dst, rh_u.nx_dst), dtype=torch.float32, device="cuda")
        dv = torch.empty((nlev, rh_v.ny_dst, rh_v.nx_dst), dtype=torch.float32, device="cuda")
        wk = dict(out_dtype=torch.float32, dst_be=True)
        out["wind_f32be"] = leg(lambda: R.wind_destagger(rh_u, rh_v, ca, sa, um, vm, nlev, outs=(du, dv), **wk),
                                lambda: R.wind_destagger(rh_u, rh_v, ca, sa, um, vm, nlev, outs=(pu, pv), **wk))
        out["wind_ld"] = ld
        rh_u.release()
        rh_v.release()
        grid.destroy()
        mesh.destroy()
        result[name] = out
        del s64, lf32, um, vm
        torch.cuda.empty_cache()
    if "x_c4_1799x1059" in result and "c4_3m_regional" in result and not a.only:
        odd, ctl = result["x_c4_1799x1059"], result["c4_3m_regional"]
        result["f32be_file_order_pitched_odd_vs_control"] = round(odd["f32be_file_order"]["pitched_frac"] / ctl["f32be_file_order"]["dense_frac"], 4)
    print(json.dumps(result))
    _lib.finalize()


if __name__ == "__main__":
    main()
