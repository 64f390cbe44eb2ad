#!/usr/bin/env python3
"""The wind chain turned round (mpg_wind_to_mesh_dev) on configuration 4 turned round: U on the 1801 x 1060 EDGE1 points and V on the
1800 x 1061 EDGE2 points of the 3-km Lambert grid -> earth-relative winds on the 3.0 M cells of the regional mesh, 55 levels, float32 in
and out, both destination layouts.  In ONE process, on ONE pair of bilinear handles and the angles of mesh_rotang:
    fused_cf / fused_lf   wind_to_mesh into [lev][cell] / [cell][lev]
    chain_cf / chain_lf   the only route the library had before: two regrid_to_mesh calls into float64 [lev][cell], the rotation as torch
                          elementwise operations (four products, two sums), the cast to float32 and -- for [cell][lev] -- the
                          transposition (tensor.t().contiguous())
    d2d_copy              a device-to-device copy of the two results' size: the box's own copy rate, the yardstick of the fractions below
A timed block is --batch launches back to back between one pair of HIP events behind one untimed launch; the median per-call ms over --reps
blocks goes out with the algorithmic bytes  L * (U_u + U_v) * e_s + 2 * P * L * e_d + P * (2 * NNZ * 12 + 16)  (U_u / U_v = the grid points
each handle references, P = cells, L = levels, e_s = e_d = 4, NNZ = 4) as a fraction of the measured copy rate, as one JSON line.
    python tools/wind_to_mesh_probe.py [--reps 7] [--batch 3] [--warmup 2] [--out profiles/r18_wind_to_mesh.md]"""
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
    ap.add_argument("--out", default=None, help="also write the record as markdown to this file")
    a = ap.parse_args()
    import time
    import torch
    from mpassit_amd import _lib, regrid as R, workloads
    _lib.init(0)
    t0 = time.time()
    m, g, nlev, desc = workloads.workload("c4_3m_regional")
    res = {"what": "wind_to_mesh_probe", "workload": desc + ", turned round: U (EDGE1) / V (EDGE2) float32 -> mesh cells float32", "nlev": nlev}

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

    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_proj(g, fill_target=False)
    rh_u = R.regrid_store_to_mesh(grid, mesh, staggerloc=R.STAGGERLOC_EDGE1)
    rh_v = R.regrid_store_to_mesh(grid, mesh, staggerloc=R.STAGGERLOC_EDGE2)
    ca, sa = R.mesh_rotang(grid, mesh)
    uu, uv, P = int(rh_u.unique_sources().size), int(rh_v.unique_sources().size), rh_u.n_dst
    by = nlev * (uu + uv) * 4 + 2 * P * nlev * 4 + P * (2 * 4 * 12 + 16)
    res.update({"n_src_u": rh_u.n_src, "n_src_v": rh_v.n_src, "n_dst": P, "unique_src_u": uu, "unique_src_v": uv, "alg_bytes": by,
                "setup_s": round(time.time() - t0, 1)})
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    u = torch.randn((nlev, rh_u.n_src), dtype=torch.float32, device="cuda", generator=gen) * 12.0
    v = torch.randn((nlev, rh_v.n_src), dtype=torch.float32, device="cuda", generator=gen) * 12.0
    cf = tuple(torch.empty((nlev, P), dtype=torch.float32, device="cuda") for _ in range(2))
    lf = tuple(torch.empty((P, nlev), dtype=torch.float32, device="cuda") for _ in range(2))
    a64 = torch.empty((1, nlev, P), dtype=torch.float64, device="cuda")
    b64 = torch.empty((1, nlev, P), dtype=torch.float64, device="cuda")
    ccf = [torch.empty((nlev, P), dtype=torch.float32, device="cuda") for _ in range(2)]
    clf = [torch.empty((P, nlev), dtype=torch.float32, device="cuda") for _ in range(2)]
    un = torch.as_tensor((rh_u.weights()[0][:, 0] < 0) | (rh_v.weights()[0][:, 0] < 0), device="cuda")
    res["unmapped_in_either"] = int(un.sum())

    def chain(lev_fast):
        rh_u.regrid_to_mesh(u, nlev=nlev, out=a64)
        rh_v.regrid_to_mesh(v, nlev=nlev, out=b64)
        x, y = a64[0], b64[0]
        ue = (x * ca - y * sa).to(torch.float32)
        ve = (x * sa + y * ca).to(torch.float32)
        if lev_fast:
            clf[0].copy_(ue.t())
            clf[1].copy_(ve.t())
        else:
            ccf[0].copy_(ue)
            ccf[1].copy_(ve)

    legs = {"fused_cf": lambda: R.wind_to_mesh(rh_u, rh_v, ca, sa, u, v, nlev, layout=R.LAYOUT_CELL_FAST, outs=cf),
            "fused_lf": lambda: R.wind_to_mesh(rh_u, rh_v, ca, sa, u, v, nlev, layout=R.LAYOUT_LEV_FAST, outs=lf),
            "chain_cf": lambda: chain(False),
            "chain_lf": lambda: chain(True),
            "d2d_copy": lambda: (ccf[0].copy_(cf[0]), ccf[1].copy_(cf[1]))}
    legs["fused_cf"]()
    legs["fused_lf"]()
    chain(False)
    torch.cuda.synchronize()
    # the chain's values on the points mapped in both handles (the fused call's +0.0 rule is the wrapper's, not the chain's)
    res["cf_equals_chain_on_mapped_points"] = bool(torch.equal(cf[0][:, ~un], ccf[0][:, ~un]) and torch.equal(cf[1][:, ~un], ccf[1][:, ~un]))
    res["lf_is_cf_transposed"] = bool(torch.equal(lf[0], cf[0].t()) and torch.equal(lf[1], cf[1].t()))
    for name, fn in legs.items():
        med, lo, hi = median(fn)
        res[name] = {"ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3)}
    copy_rate = 2 * 2 * cf[0].numel() * 4 / (res["d2d_copy"]["ms_median"] * 1e-3)   # bytes read + written per second
    res["d2d_copy"]["tb_s"] = round(copy_rate / 1e12, 3)
    for name in ("fused_cf", "fused_lf", "chain_cf", "chain_lf"):
        res[name]["alg_tb_s"] = round(by / (res[name]["ms_median"] * 1e-3) / 1e12, 3)
        res[name]["fraction_of_copy_rate"] = round(by / (res[name]["ms_median"] * 1e-3) / copy_rate, 3)
    res["cf_speedup_over_chain"] = round(res["chain_cf"]["ms_median"] / res["fused_cf"]["ms_median"], 2)
    res["lf_speedup_over_chain"] = round(res["chain_lf"]["ms_median"] / res["fused_lf"]["ms_median"], 2)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# Round 18: wind_to_mesh against the chain it replaces (tools/wind_to_mesh_probe.py)\n\n")
            f.write("%s; %d levels; P = %d cells, %d unmapped in either handle; U_u = %d, U_v = %d referenced grid points.\n"
                    % (res["workload"], nlev, P, res["unmapped_in_either"], uu, uv))
            f.write("Algorithmic bytes L (U_u + U_v) e_s + 2 P L e_d + P (2 NNZ 12 + 16) = %.3f GB; median of %d blocks of %d calls.\n\n"
                    % (by / 1e9, a.reps, a.batch))
            f.write("| leg | ms median | ms min | ms max | algorithmic TB/s | fraction of the copy rate |\n|---|---|---|---|---|---|\n")
            for name in ("fused_cf", "fused_lf", "chain_cf", "chain_lf"):
                r = res[name]
                f.write("| %s | %.3f | %.3f | %.3f | %.3f | %.3f |\n" % (name, r["ms_median"], r["ms_min"], r["ms_max"], r["alg_tb_s"], r["fraction_of_copy_rate"]))
            r = res["d2d_copy"]
            f.write("| d2d_copy (2 x P x L float32) | %.3f | %.3f | %.3f | %.3f | 1 |\n\n" % (r["ms_median"], r["ms_min"], r["ms_max"], r["tb_s"]))
            f.write("Fused over chain: [lev][cell] %.2fx, [cell][lev] %.2fx.  [lev][cell] equals the chain on the points mapped in both handles: %s; "
                    "[cell][lev] is its transposition: %s.\n" % (res["cf_speedup_over_chain"], res["lf_speedup_over_chain"],
                                                               res["cf_equals_chain_on_mapped_points"], res["lf_is_cf_transposed"]))
    rh_u.release()
    rh_v.release()
    mesh.destroy()
    grid.destroy()
    _lib.finalize()


if __name__ == "__main__":
    main()
