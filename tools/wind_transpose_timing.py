"""The adjoint of the wind chain on the README's 1800 x 1060 Lambert grid, 55 levels, rotated, float64: the fused
mpg_wind_destagger_transpose_dev against its three-call chain (two mpg_regrid_transpose_dev + mpg_rotate_winds_transpose_dev), every
array device-resident and allocated ahead.  Checks first that the two give the same bits, then times both in one process, alternating,
after a warm-up of each: medians of device-event times.  Prints one JSON line (ms per call, the ratio, algorithmic bytes, fraction of
the 8 TB/s HBM peak); exit status 1 when the bits differ or the fused call is slower than its chain.
    python tools/wind_transpose_timing.py [--nx 1800 --ny 1060 --nlev 55 --reps 20 --f32]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=1800)
    ap.add_argument("--ny", type=int, default=1060)
    ap.add_argument("--nlev", type=int, default=55)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--f32", action="store_true", help="float32 gradients of U and V")
    args = ap.parse_args()
    import torch
    from mpassit_amd import _lib, regrid as R, target_grid as T
    _lib.init(0)
    t = T.define_target_grid_params("lambert", args.nx + 1, args.ny + 1, dx=3000.0, dy=3000.0, ref_lat=38.5, ref_lon=-97.5, truelat1=38.5,
                                    truelat2=38.5, stand_lon=-97.5)
    grid = R.Grid.from_target(t)
    nlev, NP = args.nlev, t.nx * t.ny
    dt = torch.float32 if args.f32 else torch.float64
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    gu = (torch.rand((nlev, t.ny, t.nx + 1), dtype=torch.float64, device="cuda", generator=gen) * 2 - 1).to(dt)
    gv = (torch.rand((nlev, t.ny + 1, t.nx), dtype=torch.float64, device="cuda", generator=gen) * 2 - 1).to(dt)
    cosa = torch.as_tensor(np.ascontiguousarray(t.cosa), device="cuda")
    sina = torch.as_tensor(np.ascontiguousarray(t.sina), device="cuda")
    rh_u, rh_v = R.regrid_store_grid(grid, R.STAGGERLOC_EDGE1), R.regrid_store_grid(grid, R.STAGGERLOC_EDGE2)
    fu, fv, cu, cv = (torch.empty((nlev, t.ny, t.nx), dtype=torch.float64, device="cuda") for _ in range(4))

    def chain():
        rh_u.regrid_transpose(gu, nlev=nlev, out=cu)
        rh_v.regrid_transpose(gv, nlev=nlev, out=cv)
        R.rotate_winds_cgrid_transpose(cosa, sina, cu, cv)

    def fused():
        R.wind_destagger_transpose(rh_u, rh_v, cosa, sina, gu, gv, nlev, outs=(fu, fv))

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    for fn in (chain, fused, chain, fused):      # the first calls build the transposed indices and load the code objects
        fn()
    torch.cuda.synchronize()
    same = bool((cu.view(torch.int64) == fu.view(torch.int64)).all()) and bool((cv.view(torch.int64) == fv.view(torch.int64)).all())
    tc, tf = [], []
    for _ in range(max(20, args.reps)):
        tc.append(once(chain))
        tf.append(once(fused))
    tc.sort()
    tf.sort()
    c_med, f_med = tc[len(tc) // 2], tf[len(tf) // 2]
    es = 4 if args.f32 else 8
    st_u, st_v = rh_u.transpose_stats(), rh_v.transpose_stats()
    once_bytes = 2 * (NP + 1) * 4 + 4 * (rh_u.n_dst + rh_v.n_dst) * 12 + NP * 16      # both transposed indices (at most 4 entries per point) and the angles
    lev_fused = (rh_u.n_dst + rh_v.n_dst) * es + 2 * NP * 8                           # gU and gV gathered once, both results stored
    lev_chain = lev_fused + 4 * NP * 8                                                 # the rotation reads and rewrites both
    alg_f, alg_c = nlev * lev_fused + once_bytes, nlev * lev_chain + once_bytes + 2 * NP * 8
    print(json.dumps({"grid": "%dx%d Lambert 3 km" % (t.nx, t.ny), "nlev": nlev, "src": "f32" if args.f32 else "f64", "rotated": True, "reps": len(tc),
                      "bits_equal": same, "chain_ms": round(c_med, 4), "chain_ms_min": round(tc[0], 4), "fused_ms": round(f_med, 4),
                      "fused_ms_min": round(tf[0], 4), "fused_over_chain": round(f_med / c_med, 4), "speedup": round(c_med / f_med, 3),
                      "alg_bytes_per_level_fused": lev_fused, "alg_bytes_per_level_chain": lev_chain, "alg_bytes_fused": alg_f, "alg_bytes_chain": alg_c,
                      "fused_frac_of_8TBs": round(alg_f / (f_med * 1e-3) / 8e12, 4), "chain_frac_of_8TBs": round(alg_c / (c_med * 1e-3) / 8e12, 4),
                      "max_entries_per_source": [int(st_u[1]), int(st_v[1])]}))
    for rh in (rh_u, rh_v):
        rh.release()
    grid.destroy()
    _lib.finalize()
    return 0 if (same and f_med <= c_med) else 1


if __name__ == "__main__":
    sys.exit(main())
