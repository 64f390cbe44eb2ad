#!/usr/bin/env python3
"""Winds through CSR handles (mpg_wind_csr_to_edges_dev, mpg_wind_csr_to_mesh_dev) on configuration 5 turned round: U and V on the
3600 x 1800 CENTER points of the periodic global lat-lon grid -> the edge-normal wind on the about 9 M edges (synth.mesh_edges) and the
earth-relative winds on the cells of the 3 003 042-cell geodesic mesh, 55 levels, float32 and float64 (in and out), both destination
layouts.  In ONE process, on ONE POLEMETHOD_ALLAVG handle per destination given as both rh_u and rh_v (a collocated analysis) and the
angles of mesh_edge_rotang(None, mesh), per (type, results, layout):
    fused   wind_csr_to_edges (un; un + ut) / wind_csr_to_mesh without rotation (ue, ve) into [lev][point] (cf) / [point][lev] (lf)
    chain   the route a host could improvise before: two regrid_csr_to_mesh calls into float64 [lev][point], the torch products and
            the sum (a * cn + b * sn; with ut also b * cn - a * sn; cells: a, b), the cast and -- for [point][lev] -- the transposition
    d2d     a device-to-device copy of ONE result's size in float32: the box's own copy rate, the yardstick of the fractions
A timed block is --batch launches back to back between one pair of HIP events behind one untimed launch; the median per-call ms over
--reps blocks goes out with the algorithmic bytes  L (U_u + U_v) e_s + n_out P L e_d + 12 nnz + 4 (P + 1) [per distinct handle] + 16 P
[with angles]  (U = the grid points the handle references, P = points, L = levels) as a fraction of the measured copy rate, as one JSON
line.  Run it under a time limit of its own:
    timeout -k 10 1100 python tools/wind_csr_probe.py [--reps 5] [--batch 10] [--warmup 2] [--out profiles/r21_wind_csr_measured.md]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="c5_global_latlon", help="c5_small: the same legs at a size for a quick look")
    ap.add_argument("--only", default=None, choices=["edges", "cells"], help="one destination's legs (a kernel trace, a second look)")
    ap.add_argument("--pole-method", default="allavg", choices=["allavg", "none"],
                    help="none: no cap rows of nx entries (what the walk of ONE long row by one lane costs shows in the difference)")
    ap.add_argument("--out", default=None, help="also write the record as markdown to this file")
    a = ap.parse_args()
    import time
    import numpy as np
    import torch
    from mpassit_amd import _lib, regrid as R, synth, workloads
    _lib.init(0)
    t0 = time.time()
    m, g, nlev, desc = workloads.workload(a.workload)
    m = synth.mesh_edges(m)
    res = {"what": "wind_csr_probe", "workload": desc + ", turned round: U, V (CENTER) -> mesh edges and cells", "nlev": nlev,
           "pole_method": a.pole_method}

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
        return {"ms_median": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3)}

    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
    pm = R.POLEMETHOD_ALLAVG if a.pole_method == "allavg" else R.POLEMETHOD_NONE
    rh_e = R.regrid_store_periodic_to_mesh(grid, mesh, meshloc=R.MESHLOC_EDGE, pole_method=pm)
    rh_c = R.regrid_store_periodic_to_mesh(grid, mesh, meshloc=R.MESHLOC_ELEMENT, pole_method=pm)
    cn, sn = R.mesh_edge_rotang(None, mesh)
    info = {}
    for tag, rh in (("edges", rh_e), ("cells", rh_c)):
        info[tag] = {"n_dst": rh.n_dst, "nnz": rh.nnz, "unique_src": int(rh.unique_sources().size), "cap_rows": rh.store_stats[3],
                     "empty_rows": int((np.diff(rh.csr()[0]) == 0).sum()), "store_ms": round(rh.store_ms, 1)}
    n_src = rh_e.n_src
    res.update({"n_cells": int(m.nCells), "n_src": n_src, "handles": info, "setup_s": round(time.time() - t0, 1)})
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    u32 = torch.randn((nlev, n_src), dtype=torch.float32, device="cuda", generator=gen) * 12.0
    v32 = torch.randn((nlev, n_src), dtype=torch.float32, device="cuda", generator=gen) * 12.0
    res["legs"] = []
    for tag, rh, results in (("edges", rh_e, ("un", "un+ut")), ("cells", rh_c, ("ue,ve",))):
        if a.only not in (None, tag):
            continue
        P, uu = rh.n_dst, info[tag]["unique_src"]
        a64 = torch.empty((1, nlev, P), dtype=torch.float64, device="cuda")
        b64 = torch.empty((1, nlev, P), dtype=torch.float64, device="cuda")
        c32 = [torch.empty((nlev, P), dtype=torch.float32, device="cuda") for _ in range(2)]
        d2d = median(lambda: c32[1].copy_(c32[0]))
        copy_rate = 2 * c32[0].numel() * 4 / (d2d["ms_median"] * 1e-3)      # bytes read + written per second
        d2d["tb_s"] = round(copy_rate / 1e12, 3)
        res["d2d_copy_" + tag] = d2d
        del c32
        for tname, dt in (("f32", torch.float32), ("f64", torch.float64)):
            u, v = u32.to(dt), v32.to(dt)
            e = u.element_size()
            for what in results:
                nout = 1 if what == "un" else 2
                by = nlev * 2 * uu * e + nout * P * nlev * e + 12 * rh.nnz + 4 * (P + 1) + (16 * P if tag == "edges" else 0)
                outs = {lay: [torch.empty(shape, dtype=dt, device="cuda") for _ in range(nout)] for lay, shape in (("cf", (nlev, P)), ("lf", (P, nlev)))}
                ref = {lay: [torch.empty_like(t) for t in outs[lay]] for lay in outs}

                def fused(lay):
                    layout = R.LAYOUT_CELL_FAST if lay == "cf" else R.LAYOUT_LEV_FAST
                    if tag == "cells":
                        R.wind_csr_to_mesh(rh, rh, None, None, u, v, nlev, layout=layout, outs=outs[lay])
                    else:
                        R.wind_csr_to_edges(rh, rh, cn, sn, u, v, nlev, layout=layout, tangential=nout == 2, outs=outs[lay] if nout == 2 else outs[lay][0])

                def chain(lay):
                    rh.regrid_csr_to_mesh(u, nlev=nlev, out=a64)
                    rh.regrid_csr_to_mesh(v, nlev=nlev, out=b64)
                    x, y = a64[0], b64[0]
                    if tag == "cells":
                        r = [x.to(dt), y.to(dt)]
                    else:
                        r = [(x * cn + y * sn).to(dt)] + ([(y * cn - x * sn).to(dt)] if nout == 2 else [])
                    for dst, t in zip(ref[lay], r):
                        dst.copy_(t.t() if lay == "lf" else t)

                for lay in ("cf", "lf"):
                    fused(lay)
                    chain(lay)
                    torch.cuda.synchronize()
                    same = all(bool(torch.equal(o, r)) for o, r in zip(outs[lay], ref[lay]))     # (an empty row: +0.0 on both sides, no rotation)
                    leg = {"dst": tag, "type": tname, "results": what, "layout": "[lev][point]" if lay == "cf" else "[point][lev]",
                           "alg_bytes": by, "equals_chain": same, "fused": median(lambda: fused(lay)), "chain": median(lambda: chain(lay))}
                    for k in ("fused", "chain"):
                        leg[k]["fraction_of_copy_rate"] = round(by / (leg[k]["ms_median"] * 1e-3) / copy_rate, 3)
                    leg["speedup_over_chain"] = round(leg["chain"]["ms_median"] / leg["fused"]["ms_median"], 2)
                    res["legs"].append(leg)
                del outs, ref
            del u, v
        del a64, b64
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("%s; %d levels; %d source points.\n" % (res["workload"], nlev, n_src))
            for tag in ("edges", "cells"):
                if a.only not in (None, tag):
                    continue
                i, d = info[tag], res["d2d_copy_" + tag]
                f.write("%s: P = %d, nnz = %d, %d cap rows, %d empty rows, U = %d referenced grid points, Store %.1f ms; device-to-device copy of P x L "
                        "float32: %.3f ms = %.3f TB/s.\n" % (tag, i["n_dst"], i["nnz"], i["cap_rows"], i["empty_rows"], i["unique_src"], i["store_ms"],
                                                             d["ms_median"], d["tb_s"]))
            f.write("Algorithmic bytes L (U_u + U_v) e_s + n_out P L e_d + 12 nnz + 4 (P + 1) per distinct handle + 16 P with angles; median of %d blocks "
                    "of %d calls.\n\n" % (a.reps, a.batch))
            f.write("| onto | type | results | layout | GB | fused ms (min .. max) | fraction of the copy rate | chain ms (min .. max) | chain / fused | equals the chain |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|\n")
            for leg in res["legs"]:
                fu, ch = leg["fused"], leg["chain"]
                f.write("| %s | %s | %s | %s | %.3f | %.3f (%.3f .. %.3f) | %.3f | %.3f (%.3f .. %.3f) | %.2f | %s |\n"
                        % (leg["dst"], leg["type"], leg["results"], leg["layout"], leg["alg_bytes"] / 1e9, fu["ms_median"], fu["ms_min"], fu["ms_max"],
                           fu["fraction_of_copy_rate"], ch["ms_median"], ch["ms_min"], ch["ms_max"], leg["speedup_over_chain"], leg["equals_chain"]))
    rh_e.release()
    rh_c.release()
    mesh.destroy()
    grid.destroy()
    _lib.finalize()


if __name__ == "__main__":
    main()
