#!/usr/bin/env python3
"""Periodic Grid -> Mesh (mpg_regrid_store_periodic_to_mesh) on a global analysis taken onto MPAS cells: the 1440 x 720 CENTER points of a
global 0.25-degree lat-lon grid -> synth.geodesic_mesh(548) (3.0 M cells).  In ONE process:
    store      the periodic bilinear Store by the index route and by the walk (tune store_boxes 0), fresh grid / mesh objects per Store;
               beside it mpg_regrid_store_to_mesh on the same coordinates handed over as a NON-periodic grid (arrays: the pyramid; arrays
               with the projection attached: the index route) -- the call a user had before, which leaves the seam column and the caps unmapped
    apply      regrid_csr_to_mesh of 55 float32 levels into [lev][cell] and [cell][lev] on the new (CSR) handle; beside it regrid_to_mesh on
               the non-periodic twin's 4-slot handle
Every figure is GPU time between HIP events (the Stores: mpg_handle_store_ms), the best of the later two of three rounds; one JSON line.
    python tools/periodic_to_mesh_probe.py [--freq 548] [--nx 1440] [--ny 720] [--nlev 55]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--freq", type=int, default=548)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--ny", type=int, default=720)
    ap.add_argument("--nlev", type=int, default=55)
    ap.add_argument("--batch", type=int, default=3)
    a = ap.parse_args()
    import time
    import numpy as np
    import torch
    from mpassit_amd import _lib, regrid as R, synth, target_grid as tg
    _lib.init(0)
    t0 = time.time()
    m = synth.geodesic_mesh(a.freq)
    g = tg.define_target_grid_params("lat-lon", nx=a.nx + 1, ny=a.ny + 1, stand_lon=0.0, is_regional=False)
    assert g.lon.shape == (a.ny, a.nx)
    nlev = a.nlev
    res = {"what": "periodic_to_mesh_probe", "grid": "%d x %d global lat-lon" % (a.nx, a.ny), "mesh": "geodesic_mesh(%d), %d cells" % (a.freq, m.nCells),
           "nlev": nlev, "setup_s": round(time.time() - t0, 1)}

    def later_best(ms):
        return {"ms_first": round(ms[0], 3), "ms_later_min": round(min(ms[1:]), 3)}

    # ---- Stores: fresh objects per Store, so that nothing comes from the handle cache ---------------------------------------------------
    store = {}
    for name, boxes in (("periodic_index", 1), ("periodic_walk", 0)):
        ms = []
        for _ in range(3):
            mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
            _lib.tune("store_boxes", boxes)
            try:
                h = R.regrid_store_periodic_to_mesh(grid, mesh)
            finally:
                _lib.tune("store_boxes", 1)
            ms.append(h.store_ms)
            st = h.store_stats
            store[name] = dict(store_path=h.store_path, took_walk=st[1], points=st[2], cap_points=st[3], seam_points=st[4], nnz=h.nnz)
            h.release()
            mesh.destroy()
            grid.destroy()
        store[name].update(later_best(ms))
    for name, attach in (("non_periodic_pyramid", False), ("non_periodic_index", True)):
        ms = []
        try:
            for _ in range(3):
                mesh, grid = R.Mesh.from_mpas(m), R.Grid(g.lon, g.lat, g.lon_c, g.lat_c, g.lon_u, g.lat_u, g.lon_v, g.lat_v)
                if attach:
                    grid.attach_proj(g.proj)
                h = R.regrid_store_to_mesh(grid, mesh)
                ms.append(h.store_ms)
                store[name] = dict(store_path=h.store_path, took_walk=h.store_stats[1], points=h.store_stats[2],
                                   unmapped=int((h.weights()[0][:, 0] < 0).sum()))
                h.release()
                mesh.destroy()
                grid.destroy()
            store[name].update(later_best(ms))
        except _lib.MpgError as e:
            store[name] = {"not_measured": str(e)}
    res["store"] = store

    # ---- applies ------------------------------------------------------------------------------------------------------------------------
    mesh, grid, plain = R.Mesh.from_mpas(m), R.Grid.from_target(g), R.Grid(g.lon, g.lat)
    rh, fx = R.regrid_store_periodic_to_mesh(grid, mesh), R.regrid_store_to_mesh(plain, mesh)
    P = rh.n_dst
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    src = torch.rand((nlev, rh.n_src), dtype=torch.float32, device="cuda", generator=gen) - 0.5
    out_cf = torch.empty((1, nlev, P), dtype=torch.float32, device="cuda")
    out_lf = torch.empty((1, P, nlev), dtype=torch.float32, device="cuda")
    legs = {"csr_to_mesh_cf": lambda: rh.regrid_csr_to_mesh(src, nlev=nlev, layout=R.LAYOUT_CELL_FAST, out=out_cf),
            "csr_to_mesh_lf": lambda: rh.regrid_csr_to_mesh(src, nlev=nlev, layout=R.LAYOUT_LEV_FAST, out=out_lf),
            "twin_to_mesh_cf": lambda: fx.regrid_to_mesh(src, nlev=nlev, layout=R.LAYOUT_CELL_FAST, out=out_cf),
            "twin_to_mesh_lf": lambda: fx.regrid_to_mesh(src, nlev=nlev, layout=R.LAYOUT_LEV_FAST, out=out_lf)}
    rounds = {k: [] for k in legs}
    for _ in range(3):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            e0.record()
            for _ in range(a.batch):
                fn()
            e1.record()
            e1.synchronize()
            rounds[name].append(e0.elapsed_time(e1) / a.batch)
    res["apply"] = {k: later_best(v) for k, v in rounds.items()}
    # the same values on the points both handles map (the CSR sum runs in column order, the 4-slot sum in corner order)
    legs["csr_to_mesh_cf"]()
    a_new = out_cf.clone()
    legs["twin_to_mesh_cf"]()
    both = torch.as_tensor(fx.weights()[0][:, 0] >= 0, device="cuda")
    res["max_abs_diff_on_common_points"] = float((a_new[0][:, both] - out_cf[0][:, both]).abs().max())
    print(json.dumps(res), flush=True)
    rh.release()
    fx.release()
    for obj in (mesh, grid, plain):
        obj.destroy()
    _lib.finalize()


if __name__ == "__main__":
    main()
