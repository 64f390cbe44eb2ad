#!/usr/bin/env python3
"""Transpose Regrid (mpg_regrid_transpose_dev) on configuration 4: c4_3m_regional's bilinear handle (3.0 M cells <- 1800 x 1060), 13 float64
fields x 55 levels, cell-fast and level-fast results; against a plain torch index_add_ scatter of the same operator (field by field).
A timed block is --batch launches back to back between one pair of HIP events behind one untimed launch; the median per-call ms over --reps
blocks and the fraction of the 8 TB/s peak of the algorithmic bytes
    nf * nlev * (n_dst * es_in + n_src * es_out) + nnz_T * 12 + 4 * (n_src + 1)
go out as one JSON line, with the RegridStore and transposed-index build times.  Run it under rocprofv3 --kernel-trace --stats for the
per-kernel split (--only cell_fast|lev_fast|index_add runs one leg).
    python tools/transpose_probe.py [--reps 7] [--batch 5] [--warmup 2] [--nfields 13] [--only LEG]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nfields", type=int, default=13)
    ap.add_argument("--only", choices=["cell_fast", "lev_fast", "index_add"], default=None)
    a = ap.parse_args()
    import time
    import numpy as np
    import torch
    from mpassit_amd import _lib, regrid as R, workloads
    _lib.init(0)
    t0 = time.time()
    m, g, nlev, desc = workloads.workload("c4_3m_regional")
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
    rh = R.regrid_store(mesh, grid, R.REGRIDMETHOD_BILINEAR)
    nf = a.nfields
    res = {"what": "transpose_probe", "workload": desc, "nfields": nf, "nlev": nlev, "n_src": rh.n_src, "n_dst": rh.n_dst,
           "store_ms": round(rh.store_ms, 3), "setup_s": round(time.time() - t0, 1), "peak_tb_s": PEAK / 1e12}
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    src = torch.rand((nf, nlev, rh.n_dst), dtype=torch.float64, device="cuda", generator=gen) - 0.5
    out_cf = torch.empty((nf, nlev, rh.n_src), dtype=torch.float64, device="cuda")
    out_lf = torch.empty((nf, rh.n_src, nlev), dtype=torch.float64, device="cuda")
    rh.regrid_transpose(src, nlev=nlev, nfields=nf, out=out_cf)       # first call: builds the transposed index
    torch.cuda.synchronize()
    nref, mx = rh.transpose_stats()
    res.update(build_ms=round(rh.transpose_build_ms(), 3), n_referenced=nref, max_per_source=mx)
    row, col, S = rh.to_esmf_weights()
    nnzt = int(S.size)
    res["nnz_T"] = nnzt
    by = nf * nlev * (rh.n_dst * 8 + rh.n_src * 8) + nnzt * 12 + 4 * (rh.n_src + 1)
    res["alg_bytes"] = by
    rt = torch.as_tensor(row.astype(np.int64) - 1, device="cuda")
    ct = torch.as_tensor(col.astype(np.int64) - 1, device="cuda")
    st = torch.as_tensor(S, device="cuda")
    out_ia = torch.empty((nlev, rh.n_src), dtype=torch.float64, device="cuda")

    def index_add():   # the scatter form: every entry adds w * g[row] into its source, field by field
        for f in range(nf):
            out_ia.zero_()
            out_ia.index_add_(1, ct, src[f][:, rt] * st)

    legs = {"cell_fast": lambda: rh.regrid_transpose(src, nlev=nlev, nfields=nf, out=out_cf),
            "lev_fast": lambda: rh.regrid_transpose(src, nlev=nlev, nfields=nf, layout=R.LAYOUT_LEV_FAST, out=out_lf),
            "index_add": index_add}
    if a.only:
        legs = {a.only: legs[a.only]}
    else:   # the two layouts agree bit for bit, and the scatter agrees with the last field within rounding
        legs["cell_fast"]()
        legs["lev_fast"]()
        index_add()
        torch.cuda.synchronize()
        res["layouts_bitwise_equal"] = bool(torch.equal(out_lf.transpose(1, 2), out_cf))
        res["index_add_max_rel_diff"] = float((out_ia - out_cf[nf - 1]).abs().max() / out_cf[nf - 1].abs().max())

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        e0.record()
        for _ in range(a.batch):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.batch

    for name, fn in legs.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = sorted(timed(fn) for _ in range(a.reps))
        med = ms[len(ms) // 2]
        res[name] = {"ms_median": round(med, 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3),
                     "hbm_fraction": round(by / (med * 1e-3) / PEAK, 3)}
    print(json.dumps(res), flush=True)
    rh.release()
    mesh.destroy()
    grid.destroy()
    _lib.finalize()


if __name__ == "__main__":
    main()
