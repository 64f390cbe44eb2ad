#!/usr/bin/env python3
"""Conservative Mesh -> Mesh (mpg_regrid_store_conserve_mesh, mpg_regrid_csr_rows_dev) at configuration-4 sizes: the 3 003 042-cell global
geodesic mesh (synth.geodesic_mesh(548)) -> the 3.0 M-cell regional mesh of configuration 4 (a global run feeding a limited-area mesh),
one field of 55 levels, float32 and float64, [cell][lev] in and out.  In ONE process:
    store           the conservative Store on fresh mesh objects (nothing from the handle cache), three rounds: the first Store of a
                    source mesh with its cell-tree build (mpg_handle_store_stats[3]), and a second one (the other normalisation:
                    another cache key) that finds the tree there; pairs clipped, entries, vertex slots
    csr_rows        regrid_csr_rows: the new kernel, one pass
    typed_T         what the library could do before for file order in and out on a CSR handle: regrid_typed(LAYOUT_LEV_FAST) into
                    [lev][cell], then a device transposition (tensor.transpose(...).contiguous()) into [cell][lev] -- the same handle
    d2d_copy        a device-to-device copy of the result's size: the box's own copy rate, the yardstick of the fractions below
A timed block is --batch launches back to back between one pair of HIP events behind one untimed launch; the median per-call ms over
--reps blocks is one round's figure; every leg is measured in three rounds and the BEST OF THE LATER TWO goes out (the first round of a
process carries first-use costs), with all three listed, and with the algorithmic bytes  (U + P) * nlev * e + nnz * 12 + P * 4  (U = the
source cells the handle references, P = destination cells, e = bytes per element) as a fraction of the measured copy rate, as one JSON line.
    python tools/mesh_conserve_probe.py [--reps 7] [--batch 3] [--warmup 2] [--freq 548] [--cells 3000000]"""
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
    ap.add_argument("--freq", type=int, default=548)
    ap.add_argument("--cells", type=int, default=3_000_000)
    a = ap.parse_args()
    import time
    import numpy as np
    import torch
    from mpassit_amd import _lib, regrid as R, synth, workloads
    _lib.init(0)
    t0 = time.time()
    g = workloads.conus_lambert_grid()
    m_reg = synth.regional_mesh_for_lambert(g.proj, 1801, 1061, a.cells)
    m_glo = synth.geodesic_mesh(a.freq)
    nlev = 55
    res = {"what": "mesh_conserve_probe", "src_cells": int(m_glo.nCells), "dst_cells": int(m_reg.nCells), "nlev": nlev,
           "mesh_setup_s": round(time.time() - t0, 1)}

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
        return ms[len(ms) // 2]

    # ---- Stores: fresh mesh objects per round; the first conservative Store of a source mesh also builds its cell tree ------------------
    rows = []
    for _ in range(3):
        src, dst = R.Mesh.from_mpas(m_glo), R.Mesh.from_mpas(m_reg)
        s1 = R.regrid_store_conserve_mesh(src, dst)
        st = s1.store_stats
        row = dict(first_ms=round(s1.store_ms, 3), cell_tree_build_ms=round(st[3] / 1e3, 3), pairs=int(st[1]), entries=int(s1.nnz), slots=int(st[6]))
        s1.release()
        s2 = R.regrid_store_conserve_mesh(src, dst, R.NORM_FRACAREA)
        row["with_tree_ms"] = round(s2.store_ms, 3)
        assert s2.store_stats[3] == 0
        s2.release()
        rows.append(row)
        src.destroy()
        dst.destroy()
    res["store"] = rows

    src_mesh, dst_mesh = R.Mesh.from_mpas(m_glo), R.Mesh.from_mpas(m_reg)
    rh = R.regrid_store_conserve_mesh(src_mesh, dst_mesh)
    U, P, nnz = int(rh.unique_sources().size), rh.n_dst, int(rh.nnz)
    rp = rh.csr()[0]
    frac = rh.dst_frac()
    res.update({"n_src": rh.n_src, "n_dst": P, "unique_src": U, "nnz": nnz, "longest_row": int(np.diff(rp).max()),
                "empty_rows": int((np.diff(rp) == 0).sum()), "frac_min": float(frac.min()), "frac_max_minus_1": float(frac.max() - 1.0),
                "setup_s": round(time.time() - t0, 1)})
    del rp, frac
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    for tag, dt, e in (("f32", torch.float32, 4), ("f64", torch.float64, 8)):
        by = (U + P) * nlev * e + nnz * 12 + P * 4
        src = (torch.rand((rh.n_src, nlev), dtype=torch.float64, device="cuda", generator=gen) - 0.5).to(dt)
        out = torch.empty((1, P, nlev), dtype=dt, device="cuda")
        tmp = torch.empty((1, nlev, 1, P), dtype=dt, device="cuda")
        base = torch.empty((1, P, nlev), dtype=dt, device="cuda")

        def typed_t():
            rh.regrid_typed(src.reshape(-1), nlev=nlev, layout=R.LAYOUT_LEV_FAST, out=tmp)
            base.copy_(tmp.reshape(1, nlev, P).transpose(1, 2))

        legs = {"csr_rows": lambda: rh.regrid_csr_rows(src, nlev=nlev, out=out),
                "typed_T": typed_t,
                "typed_only": lambda: rh.regrid_typed(src.reshape(-1), nlev=nlev, layout=R.LAYOUT_LEV_FAST, out=tmp),
                "d2d_copy": lambda: base.copy_(out)}
        legs["csr_rows"]()
        typed_t()
        torch.cuda.synchronize()
        bits = torch.int32 if e == 4 else torch.int64
        r = {"alg_bytes": by, "csr_rows_equals_typed_T_bits": bool(torch.equal(out.view(bits), base.view(bits)))}
        rounds = {name: [] for name in legs}
        for _ in range(3):
            for name, fn in legs.items():
                rounds[name].append(round(median(fn), 3))
        for name in legs:
            r[name] = {"ms_rounds": rounds[name], "ms": min(rounds[name][1:])}
        copy_rate = 2 * out.numel() * e / (r["d2d_copy"]["ms"] * 1e-3)   # bytes read + written per second
        r["d2d_copy"]["tb_s"] = round(copy_rate / 1e12, 3)
        for name in ("csr_rows", "typed_T"):
            r[name]["alg_tb_s"] = round(by / (r[name]["ms"] * 1e-3) / 1e12, 3)
            r[name]["fraction_of_copy_rate"] = round(by / (r[name]["ms"] * 1e-3) / copy_rate, 3)
        r["csr_rows_speedup_over_typed_T"] = round(r["typed_T"]["ms"] / r["csr_rows"]["ms"], 2)
        res[tag] = r
        del src, out, tmp, base
    print(json.dumps(res), flush=True)
    rh.release()
    src_mesh.destroy()
    dst_mesh.destroy()
    _lib.finalize()


if __name__ == "__main__":
    main()
