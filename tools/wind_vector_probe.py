#!/usr/bin/env python3
"""The Cartesian-vector wind Regrid (mpg_wind_vector_dev) on configuration 5 turned round: U and V on the 3600 x 1800 CENTER points of
the periodic global lat-lon grid -> (un, ut) on the about 9 M edges (synth.mesh_edges; frames turned by angleEdge) and (ue, ve) on the
cells of the 3 003 042-cell geodesic mesh, 55 levels, float32 and float64 (in and out), both destination layouts.  In ONE process, per
destination and pole method one handle of regrid_store_periodic_to_mesh, its frames (sphere_frames) and blocks (wind_vector_weights),
and per (type, results, layout):
    fused   wind_vector (r0 alone: un; both: un + ut / ue, ve) into [lev][point] (cf) / [point][lev] (lf)
    chain   the route a host could improvise before: regrid_csr_to_mesh of four (two for un) from-weights handles with the values m[k]
            into float64 [lev][point], one torch add per result, the cast and -- for [point][lev] -- the transposition
    scalar  the scalar call on the same handle, for comparison: wind_csr_to_edges / wind_csr_to_mesh (what it costs, cap rows included)
    d2d     a device-to-device copy of ONE result's size in float32: the box's own copy rate, the yardstick of the fractions
The edges are measured on the POLEMETHOD_ALLAVG handle, the cells on a POLEMETHOD_NONE and on an ALLAVG handle (two cap rows of nx
entries, each walked by ONE lane).  A timed block is --batch launches back to back between one pair of HIP events behind one untimed
launch; the median per-call ms over --reps blocks goes out with the algorithmic bytes  2 L U e_s + n_out P L e_d + (4 + 16 n_out) nnz +
4 (P + 1)  (U = the grid points the handle references, P = points, L = levels) as a fraction of the measured copy rate, as one JSON
line.  Run it under a time limit of its own:
    timeout -k 10 1100 python tools/wind_vector_probe.py [--reps 5] [--batch 5] [--warmup 1] [--out profiles/r22_wind_vector_measured.md]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="c5_global_latlon", help="c5_small: the same legs at a size for a quick look")
    ap.add_argument("--only", default=None, choices=["edges", "cells"], help="one destination's legs (a kernel trace, a second look)")
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
    res = {"what": "wind_vector_probe", "workload": desc + ", turned round: U, V (CENTER) -> mesh edges and cells as a vector", "nlev": nlev}

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
    cn, sn = R.mesh_edge_rotang(None, mesh)
    sf = R.sphere_frames(np.radians(g.lon).reshape(-1), np.radians(g.lat).reshape(-1))
    frames = {"edges": R.sphere_frames(m.lonEdge, m.latEdge, np.cos(m.angleEdge), np.sin(m.angleEdge)), "cells": R.sphere_frames(m.lonCell, m.latCell)}
    n_src = sf.shape[1]
    res.update({"n_cells": int(m.nCells), "n_src": int(n_src), "setup_s": round(time.time() - t0, 1)})
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    u32 = torch.randn((nlev, n_src), dtype=torch.float32, device="cuda", generator=gen) * 12.0
    v32 = torch.randn((nlev, n_src), dtype=torch.float32, device="cuda", generator=gen) * 12.0
    res["legs"], res["handles"] = [], []
    for tag, pole, results in (("edges", "allavg", ("un", "un+ut")), ("cells", "none", ("ue,ve",)), ("cells", "allavg", ("ue,ve",))):
        if a.only not in (None, tag):
            continue
        t1 = time.time()
        rh = R.regrid_store_periodic_to_mesh(grid, mesh, meshloc=R.MESHLOC_EDGE if tag == "edges" else R.MESHLOC_ELEMENT,
                                             pole_method=R.POLEMETHOD_ALLAVG if pole == "allavg" else R.POLEMETHOD_NONE)
        blocks = R.wind_vector_weights(rh, sf, frames[tag])
        weights_ms = median(lambda: R.wind_vector_weights(rh, sf, frames[tag]))["ms_median"]
        rowptr, col, _ = rh.csr()
        row = np.repeat(np.arange(1, rh.n_dst + 1, dtype=np.int32), np.diff(rowptr))
        mh = blocks.cpu().numpy()
        A = [R.RouteHandle.from_weights(rh.n_src, rh.n_dst, 1, row, (col + 1).astype(np.int32), mh[k]) for k in range(4)]
        P, uu = rh.n_dst, int(rh.unique_sources().size)
        info = {"dst": tag, "pole_method": pole, "n_dst": P, "nnz": rh.nnz, "unique_src": uu, "cap_rows": rh.store_stats[3],
                "empty_rows": int((np.diff(rowptr) == 0).sum()), "longest_row": int(np.diff(rowptr).max()), "store_ms": round(rh.store_ms, 1),
                "weights_ms": weights_ms, "chain_setup_s": round(time.time() - t1, 1)}
        del row, col, mh
        t64 = [torch.empty((1, nlev, P), dtype=torch.float64, device="cuda") for _ in range(4)]
        c32 = [torch.empty((nlev, P), dtype=torch.float32, device="cuda") for _ in range(2)]
        d2d = median(lambda: c32[1].copy_(c32[0]))
        copy_rate = 2 * c32[0].numel() * 4 / (d2d["ms_median"] * 1e-3)      # bytes read + written per second
        d2d["tb_s"] = round(copy_rate / 1e12, 3)
        info["d2d_copy"] = d2d
        res["handles"].append(info)
        del c32
        for tname, dt in (("f32", torch.float32), ("f64", torch.float64)):
            u, v = u32.to(dt), v32.to(dt)
            e = u.element_size()
            for what in results:
                nout = 1 if what == "un" else 2
                by = nlev * 2 * uu * e + nout * P * nlev * e + (4 + 16 * nout) * rh.nnz + 4 * (P + 1)
                outs = {lay: [torch.empty(shape, dtype=dt, device="cuda") for _ in range(nout)] for lay, shape in (("cf", (nlev, P)), ("lf", (P, nlev)))}
                ref = {lay: [torch.empty_like(t) for t in outs[lay]] for lay in outs}
                sca = {lay: [torch.empty_like(t) for t in outs[lay]] for lay in outs}

                def fused(lay):
                    layout = R.LAYOUT_CELL_FAST if lay == "cf" else R.LAYOUT_LEV_FAST
                    R.wind_vector(rh, blocks, u, v, nlev, layout=layout, second=nout == 2, outs=outs[lay] if nout == 2 else outs[lay][0])

                def chain(lay):
                    for k in range(2 * nout):
                        A[k].regrid_csr_to_mesh(u if k % 2 == 0 else v, nlev=nlev, out=t64[k])
                    r = [(t64[0][0] + t64[1][0]).to(dt)] + ([(t64[2][0] + t64[3][0]).to(dt)] if nout == 2 else [])
                    for dst, t in zip(ref[lay], r):
                        dst.copy_(t.t() if lay == "lf" else t)

                def scalar(lay):
                    layout = R.LAYOUT_CELL_FAST if lay == "cf" else R.LAYOUT_LEV_FAST
                    if tag == "cells":
                        R.wind_csr_to_mesh(rh, rh, None, None, u, v, nlev, layout=layout, outs=sca[lay])
                    else:
                        R.wind_csr_to_edges(rh, rh, cn, sn, u, v, nlev, layout=layout, tangential=nout == 2, outs=sca[lay] if nout == 2 else sca[lay][0])

                for lay in ("cf", "lf"):
                    fused(lay)
                    chain(lay)
                    torch.cuda.synchronize()
                    same = all(bool(torch.equal(o, r)) for o, r in zip(outs[lay], ref[lay]))
                    leg = {"dst": tag, "pole_method": pole, "type": tname, "results": what, "layout": "[lev][point]" if lay == "cf" else "[point][lev]",
                           "alg_bytes": by, "equals_chain": same, "fused": median(lambda: fused(lay)), "chain": median(lambda: chain(lay)),
                           "scalar": median(lambda: scalar(lay))}
                    for k in ("fused", "chain"):
                        leg[k]["fraction_of_copy_rate"] = round(by / (leg[k]["ms_median"] * 1e-3) / copy_rate, 3)
                    leg["speedup_over_chain"] = round(leg["chain"]["ms_median"] / leg["fused"]["ms_median"], 2)
                    res["legs"].append(leg)
                del outs, ref, sca
            del u, v
        del t64, blocks
        for h in A:
            h.release()
        rh.release()
    res["total_s"] = round(time.time() - t0, 1)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("%s; %d levels; %d source points.\n" % (res["workload"], nlev, n_src))
            for i in res["handles"]:
                d = i["d2d_copy"]
                f.write("%s, %s: P = %d, nnz = %d, %d cap rows, %d empty rows, longest row %d, U = %d referenced grid points, Store %.1f ms, blocks %.3f ms; "
                        "device-to-device copy of P x L float32: %.3f ms = %.3f TB/s.\n"
                        % (i["dst"], i["pole_method"].upper(), i["n_dst"], i["nnz"], i["cap_rows"], i["empty_rows"], i["longest_row"], i["unique_src"],
                           i["store_ms"], i["weights_ms"], d["ms_median"], d["tb_s"]))
            f.write("Algorithmic bytes 2 L U e_s + n_out P L e_d + (4 + 16 n_out) nnz + 4 (P + 1); median of %d blocks of %d calls.\n\n" % (a.reps, a.batch))
            f.write("| onto | pole method | type | results | layout | GB | fused ms (min .. max) | fraction of the copy rate | chain ms (min .. max) | chain / fused "
                    "| equals the chain | scalar call ms (min .. max) |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|---|\n")
            for leg in res["legs"]:
                fu, ch, sc = leg["fused"], leg["chain"], leg["scalar"]
                f.write("| %s | %s | %s | %s | %s | %.3f | %.3f (%.3f .. %.3f) | %.3f | %.3f (%.3f .. %.3f) | %.2f | %s | %.3f (%.3f .. %.3f) |\n"
                        % (leg["dst"], leg["pole_method"].upper(), leg["type"], leg["results"], leg["layout"], leg["alg_bytes"] / 1e9, fu["ms_median"],
                           fu["ms_min"], fu["ms_max"], fu["fraction_of_copy_rate"], ch["ms_median"], ch["ms_min"], ch["ms_max"], leg["speedup_over_chain"],
                           leg["equals_chain"], sc["ms_median"], sc["ms_min"], sc["ms_max"]))
    mesh.destroy()
    grid.destroy()
    _lib.finalize()


if __name__ == "__main__":
    main()
