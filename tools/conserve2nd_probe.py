#!/usr/bin/env python3
"""Second-order conservative regridding (mpg_handle_conserve2nd) in ONE process on one card: Mesh -> Grid at configuration 4's sizes (the
3.0 M-cell regional mesh onto its 1800 x 1060 Lambert grid) and one Mesh -> Mesh pair (geodesic_mesh(100) onto global_voronoi_mesh(60000)).

  store    the first-order conservative Store (its own mpg_handle_store_ms, a Store from scratch), then mpg_handle_conserve2nd on its
           handle: GPU time of the call, the median of --reps calls with min and max, and the ratio of the two -- the piece pass re-does
           the Store's clip; pairs clipped, sources with / without a passing stencil, stencil entries; the entry count and the longest row
           beside the input's.
  regrid   55 levels, float32, [lev][cell] sources through the second-order handle beside the first-order one (both CSR), alternating:
           the median per-call ms with min and max.

One JSON line; --out writes markdown too.  Run it under a time limit of its own:
    timeout -k 10 900 python tools/conserve2nd_probe.py [--out profiles/r30_conserve2nd_measured.md]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stat(v):
    return {"ms_median": round(sorted(v)[len(v) // 2], 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)}


def _case(R, torch, name, first, src, dst, reps, batch, nlev, note):
    ms, out = [], None
    for _ in range(reps + 1):                      # the first call loads the module and builds the transposed index: not counted
        if out is not None:
            out.release()
        out = R.conserve_2nd(first, src, dst)
        ms.append(out.store_ms)
    st = out.store_stats
    rp1, rp2 = first.csr()[0], out.csr()[0]
    med = sorted(ms[1:])[len(ms[1:]) // 2]
    res = {"first_order_store_ms": round(first.store_ms, 3), "conserve2nd": _stat(ms[1:]), "conserve2nd_first_call_ms": round(ms[0], 3),
           "ratio_to_store": round(med / max(first.store_ms, 1e-9), 2), "rows": first.n_dst, "pairs_clipped": st[1], "stencils_pass": st[2],
           "stencils_fail": st[3], "stencil_entries": st[4], "nnz_first": first.nnz, "nnz_second": out.nnz,
           "entries_per_row": [round(first.nnz / max(first.n_dst, 1), 2), round(out.nnz / max(out.n_dst, 1), 2)],
           "longest_row": [int((rp1[1:] - rp1[:-1]).max()), st[6]], "ns_per_pair": round(med * 1e6 / max(st[1], 1), 2)}
    note("%s: Store %.3f ms, conserve2nd %.3f ms (%.2f x), %d -> %d entries, longest %d -> %d" % (
        name, first.store_ms, med, res["ratio_to_store"], first.nnz, out.nnz, res["longest_row"][0], st[6]))
    x = torch.randn((nlev, first.n_src), dtype=torch.float32, device="cuda")
    routes = {"first_order": lambda: first.regrid_typed(x, nlev=nlev, layout=R.LAYOUT_CELL_FAST, out_dtype=torch.float32),
              "second_order": lambda: out.regrid_typed(x, nlev=nlev, layout=R.LAYOUT_CELL_FAST, out_dtype=torch.float32)}
    for fn in routes.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            e0.record()
            for _ in range(batch):
                fn()
            e1.record()
            e1.synchronize()
            t[k].append(e0.elapsed_time(e1) / batch)
    res["regrid"] = {k: _stat(v) for k, v in t.items()}
    res["regrid"]["ratio"] = round(res["regrid"]["second_order"]["ms_median"] / res["regrid"]["first_order"]["ms_median"], 2)
    note("%s regrid: first order %.3f ms, second order %.3f ms" % (name, res["regrid"]["first_order"]["ms_median"],
                                                                   res["regrid"]["second_order"]["ms_median"]))
    out.release()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="the same at sizes for a quick look (20 000 cells under 181 x 107; geodesic_mesh(20) onto 3 000 Voronoi cells)")
    ap.add_argument("--out", default=None, help="also write the record as markdown to this file")
    a = ap.parse_args()
    import torch
    from mpassit_amd import _lib, regrid as R, synth, workloads
    _lib.init(0)
    t0 = time.time()

    def note(what):
        print("[%6.1f s] %s" % (time.time() - t0, what), file=sys.stderr, flush=True)

    nxs, nys, ncells, over = (181, 107, 20000, dict(dx=30000.0, dy=30000.0)) if a.small else (1801, 1061, 3_000_000, {})
    fa, nb = (20, 3000) if a.small else (100, 60000)
    nlev = 55
    res = {"what": "conserve2nd_probe", "nlev": nlev}
    note("building the mesh")
    g = workloads.conus_lambert_grid(nx=nxs, ny=nys, **over)
    m = synth.regional_mesh_for_lambert(g.proj, nxs, nys, ncells)
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
    note("mesh (%d cells) and grid (%d x %d mass points)" % (m.nCells, g.nx, g.ny))
    first = R.regrid_store(mesh, grid, R.REGRIDMETHOD_CONSERVE)
    res["mesh_to_grid"] = dict(cells=int(m.nCells), grid=[g.nx, g.ny], **_case(R, torch, "Mesh -> Grid", first, mesh, grid, a.reps, a.batch, nlev, note))
    first.release()
    mesh.destroy()
    grid.destroy()
    ma, mb = synth.geodesic_mesh(fa), synth.global_voronoi_mesh(nb, seed=7)
    src, dst = R.Mesh.from_mpas(ma), R.Mesh.from_mpas(mb)
    note("a geodesic mesh of %d cells onto a Voronoi mesh of %d" % (ma.nCells, mb.nCells))
    first = R.regrid_store_conserve_mesh(src, dst)
    res["mesh_to_mesh"] = dict(src_cells=int(ma.nCells), dst_cells=int(mb.nCells),
                               **_case(R, torch, "Mesh -> Mesh", first, src, dst, a.reps, a.batch, nlev, note))
    first.release()
    src.destroy()
    dst.destroy()
    res["total_s"] = round(time.time() - t0, 1)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("%d levels; medians of %d.\n\n```json\n%s\n```\n" % (nlev, a.reps, json.dumps(res, indent=1)))
    _lib.finalize()


if __name__ == "__main__":
    main()
