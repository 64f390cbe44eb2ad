#!/usr/bin/env python3
"""Mesh -> Mesh (mpg_regrid_store_mesh, mpg_regrid_rows_dev) at configuration-4 sizes: the 3 003 042-cell global geodesic mesh
(synth.geodesic_mesh(548)) -> the 3.0 M-cell regional mesh of configuration 4 (a global run feeding a limited-area mesh: every
destination cell is mapped), one field of 55 levels, float32 and float64, [cell][lev] in and out.  In ONE process:
    store           the bilinear and the nearest Store on fresh mesh objects (nothing from the handle cache), the triangle-BVH build
                    separately (mpg_handle_store_stats[3]: paid by the first bilinear Store of a source mesh only), and the bilinear
                    Store of the reverse pair (regional -> global: most points fall outside the source)
    rows            regrid_rows: the new kernel, one pass
    typed_T         what the library could do before for file order in and out: regrid_typed(LAYOUT_LEV_FAST) into [lev][cell], then a
                    device transposition (tensor.transpose(...).contiguous()) into [cell][lev] -- on the same fixed handle, and on the
                    same weights as a from-weights (CSR) handle
    d2d_copy        a device-to-device copy of the result's size: the box's own copy rate, the yardstick of the fractions below
A timed block is --batch launches back to back between one pair of HIP events behind one untimed launch; the median per-call ms over --reps
blocks goes out with the algorithmic bytes  (U + P) * nlev * e + P * 36  (U = the source cells the handle references, P = destination
cells, e = bytes per element) as a fraction of the measured copy rate, as one JSON line.
    python tools/mesh_to_mesh_probe.py [--reps 7] [--batch 3] [--warmup 2] [--freq 548] [--cells 3000000]"""
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
    res = {"what": "mesh_to_mesh_probe", "src_cells": int(m_glo.nCells), "dst_cells": int(m_reg.nCells), "nlev": nlev,
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
        return ms[len(ms) // 2], ms[0], ms[-1]

    # ---- Stores: fresh mesh objects per round; the first bilinear Store of a source mesh also builds its triangle BVH ----------------
    store = {}
    for name, ms_, md_ in (("global_to_regional", m_glo, m_reg), ("regional_to_global", m_reg, m_glo)):
        rows = []
        for _ in range(3):
            src, dst = R.Mesh.from_mpas(ms_), R.Mesh.from_mpas(md_)
            b1 = R.regrid_store_mesh(src, dst)
            bvh_us = b1.store_stats[3]
            mapped = None
            if not rows:
                mapped = int((b1.weights()[0][:, 0] >= 0).sum())
            first_ms = b1.store_ms
            b1.release()
            _lib.tune("bilinear_linetype", 1)          # another key: a second bilinear Store, the tree already there
            try:
                b2 = R.regrid_store_mesh(src, dst)
            finally:
                _lib.tune("bilinear_linetype", 0)
            n1 = R.regrid_store_mesh(src, dst, R.REGRIDMETHOD_NEAREST_STOD)
            rows.append(dict(bilinear_first_ms=round(first_ms, 3), tri_bvh_build_ms=round(bvh_us / 1e3, 3),
                             bilinear_with_tree_ms=round(b2.store_ms, 3), nearest_with_site_bvh_build_ms=round(n1.store_ms, 3)))
            if mapped is not None:
                rows[-1]["mapped_points"] = mapped
            b2.release()
            n1.release()
            src.destroy()
            dst.destroy()
        store[name] = rows
    res["store"] = store

    src_mesh, dst_mesh = R.Mesh.from_mpas(m_glo), R.Mesh.from_mpas(m_reg)
    rh = R.regrid_store_mesh(src_mesh, dst_mesh)
    U, P = int(rh.unique_sources().size), rh.n_dst
    idx, w = rh.weights()
    keep = idx >= 0
    row = np.broadcast_to(np.arange(1, P + 1, dtype=np.int32)[:, None], idx.shape)[keep]
    csr = R.RouteHandle.from_weights(rh.n_src, P, 1, row, idx[keep] + 1, w[keep])
    del idx, w, keep, row
    res.update({"n_src": rh.n_src, "n_dst": P, "unique_src": U, "setup_s": round(time.time() - t0, 1)})
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    for tag, dt, e in (("f32", torch.float32, 4), ("f64", torch.float64, 8)):
        by = (U + P) * nlev * e + P * 36
        src = (torch.rand((rh.n_src, nlev), dtype=torch.float64, device="cuda", generator=gen) - 0.5).to(dt)
        out = torch.empty((1, P, nlev), dtype=dt, device="cuda")
        tmp = torch.empty((1, nlev, 1, P), dtype=dt, device="cuda")
        base = torch.empty((1, P, nlev), dtype=dt, device="cuda")

        def typed_t(h):
            h.regrid_typed(src.reshape(-1), nlev=nlev, layout=R.LAYOUT_LEV_FAST, out=tmp)
            base.copy_(tmp.reshape(1, nlev, P).transpose(1, 2))

        legs = {"rows": lambda: rh.regrid_rows(src, nlev=nlev, out=out),
                "typed_T_fixed_handle": lambda: typed_t(rh),
                "typed_T_csr_handle": lambda: typed_t(csr),
                "typed_only_fixed_handle": lambda: rh.regrid_typed(src.reshape(-1), nlev=nlev, layout=R.LAYOUT_LEV_FAST, out=tmp),
                "d2d_copy": lambda: base.copy_(out)}
        legs["rows"]()
        typed_t(rh)
        torch.cuda.synchronize()
        r = {"alg_bytes": by, "rows_equals_typed_T_bits": bool(torch.equal(out.view(torch.int32 if e == 4 else torch.int64),
                                                                            base.view(torch.int32 if e == 4 else torch.int64)))}
        for name, fn in legs.items():
            med, lo, hi = median(fn)
            r[name] = {"ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3)}
        copy_rate = 2 * out.numel() * e / (r["d2d_copy"]["ms_median"] * 1e-3)   # bytes read + written per second
        r["d2d_copy"]["tb_s"] = round(copy_rate / 1e12, 3)
        for name in ("rows", "typed_T_fixed_handle", "typed_T_csr_handle"):
            r[name]["alg_tb_s"] = round(by / (r[name]["ms_median"] * 1e-3) / 1e12, 3)
            r[name]["fraction_of_copy_rate"] = round(by / (r[name]["ms_median"] * 1e-3) / copy_rate, 3)
        r["rows_speedup_over_typed_T_fixed"] = round(r["typed_T_fixed_handle"]["ms_median"] / r["rows"]["ms_median"], 2)
        r["rows_speedup_over_typed_T_csr"] = round(r["typed_T_csr_handle"]["ms_median"] / r["rows"]["ms_median"], 2)
        res[tag] = r
        del src, out, tmp, base
    print(json.dumps(res), flush=True)
    csr.release()
    rh.release()
    src_mesh.destroy()
    dst_mesh.destroy()
    _lib.finalize()


if __name__ == "__main__":
    main()
