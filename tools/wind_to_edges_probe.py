#!/usr/bin/env python3
"""Winds onto mesh edges (mpg_wind_to_edges_dev) on configuration 4 turned round: U on the 1801 x 1060 EDGE1 points and V on the
1800 x 1061 EDGE2 points of the 3-km Lambert grid -> the edge-normal wind on the about 9 M edges (synth.mesh_edges) of the 3.0 M-cell
regional mesh, 55 levels, float32 and float64 (in and out), both destination layouts, un alone and with the tangential ut.  In ONE
process, on ONE pair of bilinear MESHLOC_EDGE handles and the angles of mesh_edge_rotang, per (type, results, layout):
    fused   wind_to_edges into [lev][edge] (cf) / [edge][lev] (lf)
    chain   the route a host could improvise before: two regrid_to_mesh calls into float64 [lev][edge], the torch products and the sum
            (a * cn + b * sn; with ut also b * cn - a * sn), the cast and -- for [edge][lev] -- the transposition
    d2d     a device-to-device copy of ONE result's size in float32: the box's own copy rate, the yardstick of the fractions
A timed block is --batch launches back to back between one pair of HIP events behind one untimed launch; the median per-call ms over
--reps blocks goes out with the algorithmic bytes  L * (U_u + U_v) * e_s + n_out * P * L * e_d + P * (2 * NNZ * 12 + 16)  (U_u / U_v =
the grid points each handle references, P = edges, L = levels, NNZ = 4) as a fraction of the measured copy rate, as one JSON line.
    python tools/wind_to_edges_probe.py [--reps 5] [--batch 10] [--warmup 2] [--out profiles/r19_wind_to_edges_measured.md]"""
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
    ap.add_argument("--out", default=None, help="also write the record as markdown to this file")
    a = ap.parse_args()
    import time
    import torch
    from mpassit_amd import _lib, regrid as R, synth, workloads
    _lib.init(0)
    t0 = time.time()
    m, g, nlev, desc = workloads.workload("c4_3m_regional")
    m = synth.mesh_edges(m)
    res = {"what": "wind_to_edges_probe", "workload": desc + ", turned round: U (EDGE1) / V (EDGE2) -> mesh edges", "nlev": nlev}

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

    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_proj(g, fill_target=False)
    rh_u = R.regrid_store_to_mesh(grid, mesh, staggerloc=R.STAGGERLOC_EDGE1, meshloc=R.MESHLOC_EDGE)
    rh_v = R.regrid_store_to_mesh(grid, mesh, staggerloc=R.STAGGERLOC_EDGE2, meshloc=R.MESHLOC_EDGE)
    cn, sn = R.mesh_edge_rotang(grid, mesh)
    uu, uv, P = int(rh_u.unique_sources().size), int(rh_v.unique_sources().size), rh_u.n_dst
    un = torch.as_tensor((rh_u.weights()[0][:, 0] < 0) | (rh_v.weights()[0][:, 0] < 0), device="cuda")
    res.update({"n_cells": int(m.nCells), "n_dst": P, "n_src_u": rh_u.n_src, "n_src_v": rh_v.n_src, "unique_src_u": uu, "unique_src_v": uv,
                "unmapped_in_either": int(un.sum()), "setup_s": round(time.time() - t0, 1)})
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    u32 = torch.randn((nlev, rh_u.n_src), dtype=torch.float32, device="cuda", generator=gen) * 12.0
    v32 = torch.randn((nlev, rh_v.n_src), dtype=torch.float32, device="cuda", generator=gen) * 12.0
    a64 = torch.empty((1, nlev, P), dtype=torch.float64, device="cuda")
    b64 = torch.empty((1, nlev, P), dtype=torch.float64, device="cuda")
    c32 = [torch.empty((nlev, P), dtype=torch.float32, device="cuda") for _ in range(2)]
    res["d2d_copy"] = median(lambda: c32[1].copy_(c32[0]))
    copy_rate = 2 * c32[0].numel() * 4 / (res["d2d_copy"]["ms_median"] * 1e-3)      # bytes read + written per second
    res["d2d_copy"]["tb_s"] = round(copy_rate / 1e12, 3)
    del c32
    res["legs"] = []
    for tname, dt in (("f32", torch.float32), ("f64", torch.float64)):
        u, v = u32.to(dt), v32.to(dt)
        e = u.element_size()
        for nout in (1, 2):
            tan = nout == 2
            by = nlev * (uu + uv) * e + nout * P * nlev * e + P * (2 * 4 * 12 + 16)
            outs = {lay: [torch.empty(shape, dtype=dt, device="cuda") for _ in range(nout)] for lay, shape in (("cf", (nlev, P)), ("lf", (P, nlev)))}
            ref = {lay: [torch.empty_like(t) for t in outs[lay]] for lay in outs}

            def fused(lay):
                R.wind_to_edges(rh_u, rh_v, cn, sn, u, v, nlev, layout=R.LAYOUT_CELL_FAST if lay == "cf" else R.LAYOUT_LEV_FAST, tangential=tan,
                                outs=outs[lay] if tan else outs[lay][0])

            def chain(lay):
                rh_u.regrid_to_mesh(u, nlev=nlev, out=a64)
                rh_v.regrid_to_mesh(v, nlev=nlev, out=b64)
                x, y = a64[0], b64[0]
                r = [(x * cn + y * sn).to(dt)] + ([(y * cn - x * sn).to(dt)] if tan else [])
                for dst, t in zip(ref[lay], r):
                    dst.copy_(t.t() if lay == "lf" else t)

            for lay in ("cf", "lf"):
                fused(lay)
                chain(lay)
                torch.cuda.synchronize()
                mapped = ~un
                same = all(bool(torch.equal(o[:, mapped] if lay == "cf" else o[mapped], r[:, mapped] if lay == "cf" else r[mapped]))
                           for o, r in zip(outs[lay], ref[lay]))
                leg = {"type": tname, "results": "un+ut" if tan else "un", "layout": "[lev][edge]" if lay == "cf" else "[edge][lev]",
                       "alg_bytes": by, "equals_chain_on_mapped_points": same, "fused": median(lambda: fused(lay)), "chain": median(lambda: chain(lay))}
                for k in ("fused", "chain"):
                    leg[k]["fraction_of_copy_rate"] = round(by / (leg[k]["ms_median"] * 1e-3) / copy_rate, 3)
                leg["speedup_over_chain"] = round(leg["chain"]["ms_median"] / leg["fused"]["ms_median"], 2)
                res["legs"].append(leg)
            del outs, ref
        del u, v
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("%s; %d levels; P = %d edges of %d cells, %d unmapped in either handle; U_u = %d, U_v = %d referenced grid points.\n"
                    % (res["workload"], nlev, P, res["n_cells"], res["unmapped_in_either"], uu, uv))
            f.write("Algorithmic bytes L (U_u + U_v) e_s + n_out P L e_d + P (2 NNZ 12 + 16); median of %d blocks of %d calls; device-to-device copy of "
                    "P x L float32: %.3f ms = %.3f TB/s.\n\n" % (a.reps, a.batch, res["d2d_copy"]["ms_median"], res["d2d_copy"]["tb_s"]))
            f.write("| type | results | layout | GB | fused ms (min .. max) | fraction of the copy rate | chain ms (min .. max) | chain / fused | equals the chain |\n")
            f.write("|---|---|---|---|---|---|---|---|---|\n")
            for leg in res["legs"]:
                fu, ch = leg["fused"], leg["chain"]
                f.write("| %s | %s | %s | %.3f | %.3f (%.3f .. %.3f) | %.3f | %.3f (%.3f .. %.3f) | %.2f | %s |\n"
                        % (leg["type"], leg["results"], leg["layout"], leg["alg_bytes"] / 1e9, fu["ms_median"], fu["ms_min"], fu["ms_max"],
                           fu["fraction_of_copy_rate"], ch["ms_median"], ch["ms_min"], ch["ms_max"], leg["speedup_over_chain"],
                           leg["equals_chain_on_mapped_points"]))
    rh_u.release()
    rh_v.release()
    mesh.destroy()
    grid.destroy()
    _lib.finalize()


if __name__ == "__main__":
    main()
