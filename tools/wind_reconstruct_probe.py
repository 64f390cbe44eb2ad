#!/usr/bin/env python3
"""The wind reconstruction from edge-normal u (mpg_wind_reconstruct_dev) on configuration 4's mesh: u on the about 9.0 M edges
(synth.mesh_edges) of the 3.0 M-cell regional mesh -> the winds at its cells, 55 levels.  The pattern is the mesh's own edgesOnCell
(synth.edges_on_cell); the coefficients are random numbers of the right shape (the kernel does not care which it gets, and the least-squares
stand-in of synth.reconstruct_coeffs buys nothing here).  In ONE process, one handle of reconstruct_store, its values with east / north
frames (nout = 2) and without (nout = 3), and per leg, alternating:
    fused   wind_reconstruct
    chain   the route a host could improvise before, existing code on the same tree: nout regrid_csr_rows calls of from-weights handles with
            the values m[k] (file-order sources), plus the transposition for [lev][cell] results; nout regrid_csr_to_mesh calls on
            [lev][edge] sources
    d2d     a device-to-device copy of ONE float32 result's size: the box's own copy rate
Legs: float32 file order -> float32 [lev][cell], nout 2; the same -> [cell][lev]; float64 [lev][edge] -> float64 [lev][cell], nout 3.
The timed outputs of both routes are compared bit for bit.  A timed block is --batch launches back to back between one pair of HIP events
behind one untimed launch; the median per-call ms over --reps blocks (with min and max) goes out with the algorithmic bytes
nEdges L e_src + nout nCells L e_dst + nnz (4 + 8 nout) and their share of 8 TB/s, as one JSON line.  Run it under a time limit of its own:
    timeout -k 10 900 python tools/wind_reconstruct_probe.py [--reps 5] [--batch 5] [--warmup 1] [--out profiles/r23_wind_reconstruct_measured.md]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="c4_3m_regional", help="tiny: the same legs at a size for a quick look")
    ap.add_argument("--only", type=int, default=None, help="one leg (0, 1, 2) and the fused call alone: for a kernel trace")
    ap.add_argument("--out", default=None, help="also write the record as markdown to this file")
    a = ap.parse_args()
    import time
    import numpy as np
    import torch
    from mpassit_amd import _lib, regrid as R, synth, workloads
    _lib.init(0)
    t0 = time.time()
    m, _, nlev, desc = workloads.workload(a.workload)
    m = synth.mesh_edges(m)
    n_on, eoc = synth.edges_on_cell(m)
    nc, ne, me = int(m.nCells), int(m.nEdges), int(eoc.shape[1])
    res = {"what": "wind_reconstruct_probe", "workload": desc.split(" ->")[0] + ": u on the edges -> winds at the cells", "nlev": nlev, "n_cells": nc,
           "n_edges": ne, "maxEdges": me}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        e0.record()
        for _ in range(a.batch):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.batch

    def stats(ms):
        ms = sorted(ms)
        return {"ms_median": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3)}

    def note(what):
        print("[%6.1f s] %s" % (time.time() - t0, what), file=sys.stderr, flush=True)

    note("mesh, edges and edgesOnCell: %d cells, %d edges" % (nc, ne))
    rh = R.reconstruct_store(n_on, eoc, ne)
    rowptr, col, _ = rh.csr()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    coeffs = torch.rand((nc, me, 3), dtype=torch.float64, device="cuda", generator=gen) - 0.5
    frames = R.sphere_frames(m.lonCell, m.latCell)
    mv = {2: R.reconstruct_weights(rh, coeffs, frames), 3: R.reconstruct_weights(rh, coeffs)}
    row = np.repeat(np.arange(1, nc + 1, dtype=np.int32), np.diff(rowptr))
    A = {k: [R.RouteHandle.from_weights(ne, nc, 1, row, (col + 1).astype(np.int32), x) for x in mv[k].cpu().numpy()] for k in (2, 3)}
    note("handle, values and the chain's from-weights handles")
    res.update({"nnz": rh.nnz, "longest_row": int(n_on.max()), "setup_s": round(time.time() - t0, 1)})
    del row, col
    c32 = [torch.empty((nlev, nc), dtype=torch.float32, device="cuda") for _ in range(2)]
    for _ in range(a.warmup + 1):
        c32[1].copy_(c32[0])
    d2d = stats([timed(lambda: c32[1].copy_(c32[0])) for _ in range(a.reps)])
    d2d["tb_s"] = round(2 * c32[0].numel() * 4 / (d2d["ms_median"] * 1e-3) / 1e12, 3)
    res["d2d_copy"] = d2d
    del c32
    u32 = torch.randn((ne, nlev), dtype=torch.float32, device="cuda", generator=gen) * 12.0      # file order
    CF, LF = R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST
    legs = (("float32 [edge][lev] -> float32 [lev][cell]", torch.float32, LF, CF, 2), ("float32 [edge][lev] -> float32 [cell][lev]", torch.float32, LF, LF, 2),
            ("float64 [lev][edge] -> float64 [lev][cell]", torch.float64, CF, CF, 3))
    res["legs"] = []
    for i, (name, dt, sl, dl, nout) in enumerate(legs):
        if a.only not in (None, i):
            continue
        u = u32.to(dt) if sl == LF else u32.t().contiguous().to(dt)
        e = u.element_size()
        by = ne * nlev * e + nout * nc * nlev * e + rh.nnz * (4 + 8 * nout)
        shape = (nlev, nc) if dl == CF else (nc, nlev)
        outs = [torch.empty(shape, dtype=dt, device="cuda") for _ in range(nout)]
        ref = [torch.empty(shape, dtype=dt, device="cuda") for _ in range(nout)]
        rows = [torch.empty((nc, nlev), dtype=dt, device="cuda") for _ in range(nout)] if sl == LF and dl == CF else None

        def fused():
            R.wind_reconstruct(rh, mv[nout], u, nlev, src_layout=sl, layout=dl, outs=outs)

        def chain():
            for k in range(nout):
                if sl == CF:
                    A[nout][k].regrid_csr_to_mesh(u, nlev=nlev, out=ref[k].reshape(1, nlev, nc))
                elif dl == LF:
                    A[nout][k].regrid_csr_rows(u, nlev=nlev, out=ref[k])
                else:
                    A[nout][k].regrid_csr_rows(u, nlev=nlev, out=rows[k])
                    ref[k].copy_(rows[k].t())

        if a.only is not None:
            for _ in range(a.warmup + a.reps):
                fused()
            torch.cuda.synchronize()
            continue
        for _ in range(a.warmup):
            fused()
            chain()
        torch.cuda.synchronize()
        tf, tc = [], []
        for _ in range(a.reps):                 # alternating legs
            tf.append(timed(fused))
            tc.append(timed(chain))
        torch.cuda.synchronize()
        bits = torch.int32 if dt == torch.float32 else torch.int64
        same = all(bool(torch.equal(o.view(bits), r.view(bits))) for o, r in zip(outs, ref))
        leg = {"leg": name, "nout": nout, "alg_bytes": by, "equals_chain": same, "fused": stats(tf), "chain": stats(tc)}
        for k in ("fused", "chain"):
            leg[k]["share_of_8_tb_s"] = round(by / (leg[k]["ms_median"] * 1e-3) / PEAK, 3)
        leg["chain_over_fused"] = round(leg["chain"]["ms_median"] / leg["fused"]["ms_median"], 2)
        res["legs"].append(leg)
        note("leg %d: fused %.3f ms, chain %.3f ms, equal %s" % (i, leg["fused"]["ms_median"], leg["chain"]["ms_median"], same))
        del u, outs, ref, rows
    res["total_s"] = round(time.time() - t0, 1)
    print(json.dumps(res), flush=True)
    if a.out and a.only is None:
        with open(a.out, "w") as f:
            f.write("%s; %d levels; %d cells, %d edges, nnz = %d (rows of at most %d), maxEdges = %d.\n" % (res["workload"], nlev, nc, ne, rh.nnz, res["longest_row"], me))
            f.write("Device-to-device copy of nCells x L float32: %.3f ms = %.3f TB/s.\n" % (d2d["ms_median"], d2d["tb_s"]))
            f.write("Algorithmic bytes nEdges L e_src + nout nCells L e_dst + nnz (4 + 8 nout); median of %d blocks of %d calls, fused and chain "
                    "alternating.\n\n" % (a.reps, a.batch))
            f.write("| leg | nout | GB | fused ms (min .. max) | share of 8 TB/s | chain ms (min .. max) | share of 8 TB/s | chain / fused | equals the chain |\n")
            f.write("|---|---|---|---|---|---|---|---|---|\n")
            for leg in res["legs"]:
                fu, ch = leg["fused"], leg["chain"]
                f.write("| %s | %d | %.3f | %.3f (%.3f .. %.3f) | %.3f | %.3f (%.3f .. %.3f) | %.3f | %.2f | %s |\n"
                        % (leg["leg"], leg["nout"], leg["alg_bytes"] / 1e9, fu["ms_median"], fu["ms_min"], fu["ms_max"], fu["share_of_8_tb_s"],
                           ch["ms_median"], ch["ms_min"], ch["ms_max"], ch["share_of_8_tb_s"], leg["chain_over_fused"], leg["equals_chain"]))
    for hs in A.values():
        for h in hs:
            h.release()
    rh.release()
    _lib.finalize()


if __name__ == "__main__":
    main()
