#!/usr/bin/env python3
"""The adjoint of the masked Regrid (mpg_regrid_masked_transpose_dev) on configuration 4: c4_3m_regional's bilinear handle (3.0 M cells ->
1800 x 1060), 1 field x 55 levels, NaN on 10 % of the source elements (i.i.d.), float32 and float64, both layouts.  Per (type, layout), in
ONE process on one card, the new call is timed against the two calls it is built from, on the same handle and arrays:
    masked_transpose   regrid_masked_transpose(g, src)     pass 1: the forward's gathers without its fmas; pass 2: the transpose plus one load
    masked             regrid_masked(src)                  the forward
    transpose          regrid_transpose(g)                 the unmasked adjoint
The yardstick is masked + transpose.  Every leg is warmed up (the first transposed call builds the handle's transposed index), then the
three legs alternate; a timed block is --batch launches between one pair of device events behind one untimed launch.  --repeats blocks
per leg give the median per-call ms and the run-to-run spread (max - min).  One JSON line.
    python tools/masked_transpose_probe.py [--repeats 5] [--batch 5] [--warmup 2] [--nlev 55]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEGS = ("masked_transpose", "masked", "transpose")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nlev", type=int, default=0, help="0: the workload's 55")
    a = ap.parse_args()
    import time
    import torch
    from mpassit_amd import _lib, regrid as R, workloads
    _lib.init(0)
    t0 = time.time()
    m, g, nlev, desc = workloads.workload("c4_3m_regional")
    nlev = a.nlev or nlev
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
    rh = R.regrid_store(mesh, grid, R.REGRIDMETHOD_BILINEAR)
    res = {"what": "masked_transpose_probe", "workload": desc, "nfields": 1, "nlev": nlev, "n_src": rh.n_src, "n_dst": rh.n_dst, "nan_share": 0.1,
           "repeats": a.repeats, "batch": a.batch, "setup_s": round(time.time() - t0, 1)}
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        e0.record()
        for _ in range(a.batch):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.batch

    work = torch.empty((1, nlev, rh.n_dst), dtype=torch.float64, device="cuda")
    for dt, layout in ((torch.float64, R.LAYOUT_CELL_FAST), (torch.float64, R.LAYOUT_LEV_FAST), (torch.float32, R.LAYOUT_CELL_FAST),
                       (torch.float32, R.LAYOUT_LEV_FAST)):
        name = "%s_%s" % ("lev_fast" if layout else "cell_fast", "f32" if dt == torch.float32 else "f64")
        src = torch.rand(nlev * rh.n_src, dtype=dt, device="cuda", generator=gen) - 0.5
        src[torch.rand(src.shape, device="cuda", generator=gen) < 0.1] = float("nan")
        grad = torch.rand((1, nlev, rh.ny_dst, rh.nx_dst), dtype=dt, device="cuda", generator=gen) - 0.5
        fwd = torch.empty((1, nlev, rh.ny_dst, rh.nx_dst), dtype=dt, device="cuda")
        back = torch.empty(nlev * rh.n_src, dtype=dt, device="cuda")
        kw = dict(nlev=nlev, nfields=1, layout=layout)
        legs = {"masked_transpose": lambda: rh.regrid_masked_transpose(grad, src, out=back, work=work, **kw),
                "masked": lambda: rh.regrid_masked(src, out=fwd, **kw),
                "transpose": lambda: rh.regrid_transpose(grad, out=back, out_dtype=dt, **kw)}
        for fn in legs.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in LEGS}
        for _ in range(a.repeats):                     # the legs alternate: drift of the card hits them alike
            for k in LEGS:
                ms[k].append(timed(legs[k]))
        r = {}
        for k in LEGS:
            v = sorted(ms[k])
            r[k] = {"ms_median": round(v[len(v) // 2], 3), "ms_min": round(v[0], 3), "ms_max": round(v[-1], 3), "spread_ms": round(v[-1] - v[0], 3)}
        both = r["masked"]["ms_median"] + r["transpose"]["ms_median"]
        r["sum_ms"] = round(both, 3)
        r["ratio_to_sum"] = round(r["masked_transpose"]["ms_median"] / both, 3)
        legs["masked_transpose"]()
        torch.cuda.synchronize()
        r["defined_share"] = round(float((work != 0).double().mean()), 4)
        res[name] = r
        del src, grad, fwd, back
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    rh.release()
    mesh.destroy()
    grid.destroy()
    _lib.finalize()


if __name__ == "__main__":
    main()
