#!/usr/bin/env python3
"""Handle composition (mpg_handle_compose, mpg_compose_weights_dev) at configuration 4's sizes, in ONE process on one card:

  winds    u on the about 9.0 M edges of the 3.0 M-cell regional mesh -> earth-relative winds on the 1800 x 1060 Lambert grid, 55 levels,
           float32 file-order u in, float32 [lev][ny * nx] planes out.  composite: compose(mesh -> grid bilinear, reconstruct_store),
           compose_weights of reconstruct_weights' two planes, ONE wind_reconstruct.  chain (existing calls, what the parent runs):
           wind_reconstruct at the cells, then one regrid_typed per component -- through [cell][lev] and through [lev][cell] intermediates.
  scalar   a 3600 x 1800 global lat-lon field -> the same mesh (periodic Grid -> Mesh, rows of 4) -> the same grid.  composite: one
           regrid_typed.  chain: regrid_csr_to_mesh, then regrid_typed.

Per case: the build (mpg_handle_store_ms, and wall time with its allocations and read-backs), nnz and the longest row of the composite,
mpg_compose_weights_dev, and the two applies in alternating blocks, both warm: --batch launches between one pair of HIP events behind one
untimed launch, the median per-call ms over --reps blocks with min and max, the algorithmic bytes and their share of 8 TB/s.  The float32
results of both routes are compared (how many differ, by how much), and on --check-levels levels in float64 the difference is held to
(L_A + L_B + L_C + 8) 2^-53 |A| (|B| |x|) per point, the bound of tests/test_compose_gpu.py.  One JSON line; --out writes markdown too.
Run it under a time limit of its own:   timeout -k 10 1100 python tools/compose_probe.py [--out profiles/r24_compose_measured.md]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12
EPS = 2.0 ** -53


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="c4_3m_regional", help="tiny: the same cases at a size for a quick look")
    ap.add_argument("--check-levels", type=int, default=2)
    ap.add_argument("--only", default=None, help="winds or scalar")
    ap.add_argument("--out", default=None, help="also write the record as markdown to this file")
    a = ap.parse_args()
    import time
    import numpy as np
    import torch
    from mpassit_amd import _lib, regrid as R, synth, target_grid as tg, workloads
    _lib.init(0)
    t0 = time.time()
    m, g, nlev, desc = workloads.workload(a.workload)
    tiny = a.workload == "tiny"
    res = {"what": "compose_probe", "workload": desc, "nlev": nlev, "cases": []}
    CF, LF = R.LAYOUT_CELL_FAST, R.LAYOUT_LEV_FAST

    def note(what):
        print("[%6.1f s] %s" % (time.time() - t0, what), file=sys.stderr, flush=True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        e0.record()
        for _ in range(a.batch):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.batch

    def stats(ms, nbytes=None):
        ms = sorted(ms)
        d = {"ms_median": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3)}
        if nbytes is not None:
            d["alg_bytes"] = int(nbytes)
            d["share_of_8_tb_s"] = round(nbytes / (d["ms_median"] * 1e-3) / PEAK, 3)
        return d

    def interleaved(routes):
        for _ in range(a.warmup):
            for fn in routes.values():
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in routes}
        for _ in range(a.reps):
            for k, fn in routes.items():
                t[k].append(timed(fn))
        torch.cuda.synchronize()
        return t

    def build(outer, inner):
        torch.cuda.synchronize()
        w0 = time.time()
        c = R.compose(outer, inner)
        wall = (time.time() - w0) * 1e3
        w0 = time.time()
        c2 = R.compose(outer, inner)                  # a second build: the pool's blocks and the code object are there
        wall2 = (time.time() - w0) * 1e3
        ms2 = c2.store_ms
        c2.release()
        rowptr = c.csr()[0]
        return c, {"nnz": c.nnz, "longest_row": int(np.diff(rowptr).max()), "mean_row": round(c.nnz / max(1, int((np.diff(rowptr) > 0).sum())), 2),
                   "build_gpu_ms": round(c.store_ms, 3), "build_wall_ms": round(wall, 1), "second_build_gpu_ms": round(ms2, 3),
                   "second_build_wall_ms": round(wall2, 1), "nnz_outer": outer.nnz if outer.nnz_per_row == 0 else outer.nnz_per_row * outer.n_dst,
                   "nnz_inner": inner.nnz}

    def compare32(x, y):
        bits = lambda t: t.contiguous().view(torch.int32)
        return {"float32_values": int(x.numel()), "differ": int((bits(x) != bits(y)).sum()), "max_abs_diff": float((x.double() - y.double()).abs().max())}

    def abs_handle(h, vals=None):
        """the handle with |values| (vals: other values on the same pattern), from-weights"""
        if h.nnz_per_row:
            idx, w = h.weights()
            rowptr, col, val = tg.fixed_to_csr(idx, w)
        else:
            rowptr, col, val = h.csr()
        val = np.abs(val if vals is None else vals)
        row = np.repeat(np.arange(1, h.n_dst + 1, dtype=np.int32), np.diff(rowptr))
        return R.RouteHandle.from_weights(h.n_src, h.nx_dst, h.ny_dst, row, (col + 1).astype(np.int32), val), int(np.diff(rowptr).max())

    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
    outer = R.regrid_store(mesh, grid, R.REGRIDMETHOD_BILINEAR)
    P, nc = outer.n_dst, int(m.nCells)
    note("mesh (%d cells), grid (%d points) and the Mesh -> Grid bilinear Store (%.2f ms)" % (nc, P, outer.store_ms))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(24)

    # ---- winds: edges -> grid ------------------------------------------------------------------------------------------------------------
    if a.only in (None, "winds"):
        me_ = synth.mesh_edges(m)
        n_on, eoc = synth.edges_on_cell(me_)
        ne, maxe = int(me_.nEdges), int(eoc.shape[1])
        rec = R.reconstruct_store(n_on, eoc, ne)
        coeffs = torch.rand((nc, maxe, 3), dtype=torch.float64, device="cuda", generator=gen) - 0.5
        m2 = R.reconstruct_weights(rec, coeffs, R.sphere_frames(m.lonCell, m.latCell))
        note("edges (%d), edgesOnCell, reconstruct_store and its two planes" % ne)
        c, case = build(outer, rec)
        case.update({"case": "winds: u on %d edges -> (zonal, meridional) on %d grid points" % (ne, P), "n_src": ne, "n_mid": nc, "n_dst": P})
        note("composite: nnz %d, longest row %d, build %.2f ms GPU / %.1f ms wall" % (c.nnz, case["longest_row"], c.store_ms, case["build_wall_ms"]))
        mc = R.compose_weights(c, outer, rec, m2)
        tw = [timed(lambda: R.compose_weights(c, outer, rec, m2)) for _ in range(a.reps)]
        case["compose_weights_2_planes"] = stats(tw, 2 * 8 * (rec.nnz + c.nnz) + 4 * (c.nnz + rec.nnz) + 12 * case["nnz_outer"])
        u = torch.randn((ne, nlev), dtype=torch.float32, device="cuda", generator=gen) * 12.0           # file order
        out_c = [torch.empty((nlev, P), dtype=torch.float32, device="cuda") for _ in range(2)]
        out_r = [torch.empty((1, nlev, g.ny, g.nx), dtype=torch.float32, device="cuda") for _ in range(2)]
        out_l = [torch.empty((1, nlev, g.ny, g.nx), dtype=torch.float32, device="cuda") for _ in range(2)]
        mid_r = [torch.empty((nc, nlev), dtype=torch.float32, device="cuda") for _ in range(2)]
        mid_l = [torch.empty((nlev, nc), dtype=torch.float32, device="cuda") for _ in range(2)]

        def composite():
            R.wind_reconstruct(c, mc, u, nlev, src_layout=LF, layout=CF, outs=out_c)

        def chain_rows():                             # [cell][lev] intermediates, the file order the flagship Regrid reads
            R.wind_reconstruct(rec, m2, u, nlev, src_layout=LF, layout=LF, outs=mid_r)
            for k in range(2):
                outer.regrid_typed(mid_r[k], nlev=nlev, layout=LF, out=out_r[k])

        def chain_planes():                           # [lev][cell] intermediates
            R.wind_reconstruct(rec, m2, u, nlev, src_layout=LF, layout=CF, outs=mid_l)
            for k in range(2):
                outer.regrid_typed(mid_l[k], nlev=nlev, layout=CF, out=out_l[k])

        t = interleaved({"composite": composite, "chain_rows": chain_rows, "chain_planes": chain_planes})
        b_comp = ne * nlev * 4 + 2 * P * nlev * 4 + c.nnz * (4 + 16)
        b_chain = ne * nlev * 4 + 2 * nc * nlev * 4 + rec.nnz * (4 + 16) + 2 * (nc * nlev * 4 + P * nlev * 4 + P * 3 * 12)
        case["composite"] = stats(t["composite"], b_comp)
        case["chain_cell_lev_intermediates"] = stats(t["chain_rows"], b_chain)
        case["chain_lev_cell_intermediates"] = stats(t["chain_planes"], b_chain)
        case["intermediate_bytes_removed"] = 2 * 2 * nc * nlev * 4
        case["float32_against_chain"] = compare32(torch.stack(out_c).reshape(-1), torch.stack([o.reshape(nlev, P) for o in out_r]).reshape(-1))
        note("winds: composite %.3f ms, chain %.3f / %.3f ms" % (case["composite"]["ms_median"], case["chain_cell_lev_intermediates"]["ms_median"],
                                                             case["chain_lev_cell_intermediates"]["ms_median"]))
        del out_c, out_r, out_l, mid_r, mid_l
        if a.check_levels > 0:                        # float64 on a few levels: the difference against the per-point bound
            L = a.check_levels
            u64 = u[:, :L].double().contiguous()
            comp = torch.stack(R.wind_reconstruct(c, mc, u64, L, src_layout=LF, layout=CF))
            cells = R.wind_reconstruct(rec, m2, u64, L, src_layout=LF, layout=CF)
            chain = torch.stack([outer.regrid_typed(x.contiguous(), nlev=L, out_dtype=torch.float64).reshape(L, P) for x in cells])
            absA, la = abs_handle(outer)
            lc = case["longest_row"]
            worst = 0.0
            for k in range(2):
                absB, lb = abs_handle(rec, m2[k].cpu().numpy())
                S = absA.regrid_typed(absB.regrid_typed(u64.abs().t().contiguous(), nlev=L).reshape(L, nc).contiguous(), nlev=L).reshape(L, P)
                bound = (la + lb + lc + 8) * EPS * S
                d = (comp[k] - chain[k]).abs()
                worst = max(worst, float((d / bound.clamp_min(1e-300)).max()))
                absB.release()
            absA.release()
            case["float64_check"] = {"levels": L, "max_abs_diff": float((comp - chain).abs().max()), "largest_diff_over_bound": round(worst, 4),
                                     "within_bound": worst <= 1.0}
            note("winds: float64 on %d levels, largest |diff| / bound %.4f" % (L, worst))
            del comp, cells, chain
        res["cases"].append(case)
        del u, mc, m2, coeffs
        c.release()
        rec.release()

    # ---- scalar: global grid -> mesh -> grid -------------------------------------------------------------------------------------------
    if a.only in (None, "scalar"):
        gg = tg.define_target_grid_params("lat-lon", nx=361 if tiny else 3601, ny=181 if tiny else 1801, stand_lon=0.0, is_regional=False)
        per = R.Grid.from_target(gg)
        inner = R.regrid_store_periodic_to_mesh(per, mesh)
        ns = inner.n_src
        note("periodic %d x %d grid -> mesh Store: nnz %d (%.2f ms)" % (gg.nx, gg.ny, inner.nnz, inner.store_ms))
        c, case = build(outer, inner)
        case.update({"case": "scalar: %d x %d global lat-lon -> %d mesh cells -> %d grid points" % (gg.nx, gg.ny, nc, P), "n_src": ns, "n_mid": nc, "n_dst": P})
        note("composite: nnz %d, longest row %d, build %.2f ms GPU / %.1f ms wall" % (c.nnz, case["longest_row"], c.store_ms, case["build_wall_ms"]))
        own = torch.as_tensor(inner.csr()[2], device="cuda").reshape(1, -1)
        tw = [timed(lambda: R.compose_weights(c, outer, inner, own)) for _ in range(a.reps)]
        case["compose_weights_1_plane"] = stats(tw, 8 * (inner.nnz + c.nnz) + 4 * (c.nnz + inner.nnz) + 12 * case["nnz_outer"])
        x = torch.randn((nlev, ns), dtype=torch.float32, device="cuda", generator=gen) * 12.0
        out_c = torch.empty((1, nlev, g.ny, g.nx), dtype=torch.float32, device="cuda")
        out_x = torch.empty((1, nlev, g.ny, g.nx), dtype=torch.float32, device="cuda")
        mid = torch.empty((1, nlev, nc), dtype=torch.float32, device="cuda")

        def composite():
            c.regrid_typed(x, nlev=nlev, layout=CF, out=out_c)

        def chain():
            inner.regrid_csr_to_mesh(x, nlev=nlev, layout=CF, out=mid)
            outer.regrid_typed(mid, nlev=nlev, layout=CF, out=out_x)

        t = interleaved({"composite": composite, "chain": chain})
        case["composite"] = stats(t["composite"], ns * nlev * 4 + P * nlev * 4 + c.nnz * 12 + 4 * P)
        case["chain"] = stats(t["chain"], ns * nlev * 4 + nc * nlev * 4 + inner.nnz * 12 + 4 * nc + nc * nlev * 4 + P * nlev * 4 + P * 3 * 12)
        case["intermediate_bytes_removed"] = 2 * nc * nlev * 4
        case["float32_against_chain"] = compare32(out_c.reshape(-1), out_x.reshape(-1))
        note("scalar: composite %.3f ms, chain %.3f ms" % (case["composite"]["ms_median"], case["chain"]["ms_median"]))
        if a.check_levels > 0:
            L = a.check_levels
            x64 = x[:L].double().contiguous()
            comp = c.regrid_typed(x64, nlev=L).reshape(L, P)
            chain64 = outer.regrid_typed(inner.regrid_csr_to_mesh(x64, nlev=L).reshape(L, nc).contiguous(), nlev=L).reshape(L, P)
            absA, la = abs_handle(outer)
            absB, lb = abs_handle(inner)
            S = absA.regrid_typed(absB.regrid_typed(x64.abs(), nlev=L).reshape(L, nc).contiguous(), nlev=L).reshape(L, P)
            bound = (la + lb + case["longest_row"] + 8) * EPS * S
            worst = float(((comp - chain64).abs() / bound.clamp_min(1e-300)).max())
            case["float64_check"] = {"levels": L, "max_abs_diff": float((comp - chain64).abs().max()), "largest_diff_over_bound": round(worst, 4),
                                     "within_bound": worst <= 1.0}
            note("scalar: float64 on %d levels, largest |diff| / bound %.4f" % (L, worst))
            absA.release()
            absB.release()
        res["cases"].append(case)
        c.release()
        inner.release()
        per.destroy()
    res["total_s"] = round(time.time() - t0, 1)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("%s; %d levels.  Median of %d blocks of %d calls, the routes alternating, one warm-up of each.\n\n" % (desc, nlev, a.reps, a.batch))
            for case in res["cases"]:
                f.write("%s\n\n" % case["case"])
                f.write("- composite: nnz %d (outer %d, inner %d), longest row %d, mean non-empty row %.2f\n" % (
                    case["nnz"], case["nnz_outer"], case["nnz_inner"], case["longest_row"], case["mean_row"]))
                f.write("- build: %.3f ms GPU, %.1f ms wall; a second build %.3f ms GPU, %.1f ms wall\n" % (
                    case["build_gpu_ms"], case["build_wall_ms"], case["second_build_gpu_ms"], case["second_build_wall_ms"]))
                f.write("\n| route | ms (min .. max) | GB | share of 8 TB/s |\n|---|---|---|---|\n")
                for k, v in case.items():
                    if isinstance(v, dict) and "ms_median" in v:
                        f.write("| %s | %.3f (%.3f .. %.3f) | %.3f | %.3f |\n" % (k, v["ms_median"], v["ms_min"], v["ms_max"], v["alg_bytes"] / 1e9, v["share_of_8_tb_s"]))
                f.write("\n- float32 results against the chain: %s\n" % json.dumps(case["float32_against_chain"]))
                if "float64_check" in case:
                    f.write("- float64 against the chain and the per-point bound: %s\n" % json.dumps(case["float64_check"]))
                f.write("- intermediate bytes a call no longer writes and reads back: %.3f GB\n\n" % (case["intermediate_bytes_removed"] / 1e9))
    outer.release()
    mesh.destroy()
    grid.destroy()
    _lib.finalize()


if __name__ == "__main__":
    main()
