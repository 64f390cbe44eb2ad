"""Writes tests/golden/contract_patterns.npz: the exported patterns (Pattern.of: idx / w, or rowptr / col / val) of the four small Stores
of tests/test_contract_gpu.py -- the tiny mesh under the 19 x 11 Lambert grid (bilinear, nearest, conservative) and the periodic
72 x 36 grid CENTER -> EDGE2.  Needs a GPU: the Stores are the library's.  Run from the repository root after a Store changed on purpose:

    python tests/golden/make_contract_patterns.py

tests/test_contract_ref.py reads the file on the CPU; tests/test_contract_gpu.py checks that the live Stores still give it."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import _contract_ref as cr                                                    # noqa: E402
from mpassit_amd import _lib, regrid as R, target_grid as T, workloads        # noqa: E402

LAMBERT = dict(ref_lat=38.5, ref_lon=-97.5, truelat1=38.5, truelat2=38.5, stand_lon=-97.5)


def main():
    _lib.init(0)
    mesh = R.Mesh.from_mpas(workloads.workload("tiny")[0])
    narrow = R.Grid.from_target(T.define_target_grid_params("lambert", 19, 11, dx=300000.0, dy=300000.0, **LAMBERT))
    periodic = R.Grid.from_target(T.define_target_grid_params("lat-lon", nx=73, ny=37, stand_lon=0.0, is_regional=False))
    handles = (("narrow 3", R.regrid_store(mesh, narrow, R.REGRIDMETHOD_BILINEAR)),
               ("narrow 1", R.regrid_store(mesh, narrow, R.REGRIDMETHOD_NEAREST_STOD)),
               ("narrow csr", R.regrid_store(mesh, narrow, R.REGRIDMETHOD_CONSERVE)),
               ("pole 4", R.regrid_store_grid(periodic, R.STAGGERLOC_EDGE2)))
    assert tuple(n for n, _ in handles) == cr.GOLDEN_NAMES
    out = {}
    for name, rh in handles:
        p = cr.Pattern.of(rh)
        out[name + "/shape"] = np.array([p.n_src, p.n_dst, p.nnz], np.int64)
        for attr in (("idx", "w") if p.nnz else ("rowptr", "col", "val")):
            out[name + "/" + attr] = getattr(p, attr)
        rh.release()
    np.savez_compressed(cr.GOLDEN, **out)
    print("wrote", cr.GOLDEN)
    _lib.finalize()


if __name__ == "__main__":
    main()
