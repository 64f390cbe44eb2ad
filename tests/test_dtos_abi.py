"""CPU checks of the nearest-destination-to-source Store: the header declares mpg_regrid_store_nearest_dtos and mpg_handle_get_src_nearest
with the agreed argument lists and the two enums -- the new section behind mpg_regrid_store_conserve_grid_to_grid and before the output
epilogues -- and states the contract; _lib lists, binds and exports both; the kernel file, dtos.h and the shared knn_src.h are part of the
build and keep their promises; the Python wrapper and the numpy mirror have the agreed signatures; the Fortran module has matching
bind(C) interfaces and constants (which the driver does not use)."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORE, NEAREST = "mpg_regrid_store_nearest_dtos", "mpg_handle_get_src_nearest"
ARGS = {
    STORE: ["const mpg_points *src", "const mpg_points *dst", "int norm", "const uint8_t *src_mask_dev", "const uint8_t *dst_mask_dev",
            "mpg_handle *out"],
    NEAREST: ["mpg_handle rh", "int32_t *nearest_host"],
}


def _header(strip_comments=True):
    txt = open(os.path.join(ROOT, "include", "mpassit_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S) if strip_comments else txt


def test_header_declares_the_calls_and_the_enums():
    txt = _header()
    for name, want in ARGS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, name + " is not declared"
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want
    assert re.search(r"enum\s*\{\s*MPG_REGRIDMETHOD_NEAREST_DTOS\s*=\s*5\s*\}", txt)
    assert re.search(r"enum\s*\{\s*MPG_DTOS_SUM\s*=\s*0\s*,\s*MPG_DTOS_MEAN\s*=\s*1\s*\}", txt)
    full = _header(strip_comments=False)
    at = full.index("int " + STORE + "(")
    assert full.index("int mpg_regrid_store_conserve_grid_to_grid(") < full.index("---- nearest destination to source") < at
    assert at < full.index("int " + NEAREST + "(") < full.index("---- output epilogues")
    # the five earlier method numbers stay what they were
    for name, v in (("BILINEAR", 0), ("CONSERVE", 1), ("NEAREST_STOD", 2), ("PATCH", 3), ("CONSERVE_2ND", 4)):
        assert re.search(r"MPG_REGRIDMETHOD_%s\s*=\s*%d\b" % (name, v), txt)


def test_header_states_the_contract():
    txt = _header(strip_comments=False)
    i = txt.index("int " + STORE + "(")
    doc = " ".join(txt[max(0, i - 9000):i].replace("\n *", "\n").split())
    doc = doc[doc.rindex("---- nearest destination to source"):]
    for phrase in ("ESMF_REGRIDMETHOD_NEAREST_DTOS", "scatters", "No source is lost",
                   # the point sets
                   "exactly one of mesh / grid is non-NULL", "Sources are the QUERIES", "cells, vertices or edges", "mpg_mesh_set_edges",
                   "point pyramid", "MPG_MESHLOC_ELEMENT", "site BVH built whole", "j * snx + i",
                   # the rule, the tie rule
                   "smallest (d2, id) in lexicographic order", "dist2_nofma", "stored unit vectors", "A tie goes to the lower destination id",
                   "nearest(s) = -1", "non-zero = masked", "NULL = no mask",
                   # the handle, the row order, both norms
                   "an ordinary CSR handle", "MPG_REGRIDMETHOD_NEAREST_DTOS", "in ascending source id", "summation order",
                   "MPG_DTOS_SUM (ESMF's rule): every value is 1.0", "MPG_DTOS_MEAN", "1.0 / (double)len(d)", "rounded once", "an empty row",
                   "writes +0.0", "fill value", "always present", "no dst_frac", "longest row is recorded", "sources mapped", "non-empty rows",
                   "mpg_handle_store_ms", "mpg_handle_get_src_nearest", "4 bytes per source",
                   # determinism and ownership
                   "no atomic decides a stored byte", "fresh objects", "not cached", "mpg_handle_release", "drains the Store worker",
                   # the refusals
                   "names mpg_regrid_store_nearest_dtos", "MPG_ERR_INVALID_ARG", "NULL argument", "both or neither", "norm",
                   "stagger without coordinates", "mesh without edges", "MPG_ERR_UNSUPPORTED", "MPG_MESHLOC_NODE", "MPG_MESHLOC_EDGE",
                   "mpg_mesh_create_window", "source window", "MPG_ERR_OVERFLOW", "beyond int32", "Empty input is success", "all-empty pattern",
                   # the consumers
                   "mpg_regrid_typed", "mpg_regrid_csr_to_mesh_dev", "mpg_regrid_csr_rows_dev", "mpg_regrid_masked_dev", "mpg_regrid_transpose_dev",
                   "mpg_handle_compose", "nearest gather in the other direction", "MPG_MASKRULE_AUTO", "would not re-route its sources"):
        assert phrase in doc, phrase


def test_lib_lists_binds_and_exports_them():
    from mpassit_amd import _lib, build
    for name in ARGS:
        assert name in _lib.SYMBOLS
    assert "k_store_dtos.hip" in build.SOURCES and "dtos.h" in build.HEADERS and "knn_src.h" in build.HEADERS
    for f in ("k_store_dtos.hip", "dtos.h", "knn_src.h"):
        assert os.path.exists(os.path.join(build.CSRC, f))
    build.build()
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    for name in ARGS:
        assert hasattr(lib, name)
        assert re.search(r" T %s\b" % name, out)
    assert list(_lib._STORE_NEAREST_DTOS_PROTO._argtypes_) == [C.POINTER(_lib.Points), C.POINTER(_lib.Points), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert list(_lib._HANDLE_GET_SRC_NEAREST_PROTO._argtypes_) == [C.c_void_p, C.c_void_p]
    assert _lib._STORE_NEAREST_DTOS_PROTO._restype_ is C.c_int and _lib._HANDLE_GET_SRC_NEAREST_PROTO._restype_ is C.c_int
    assert callable(_lib.regrid_store_nearest_dtos) and callable(_lib.handle_get_src_nearest)
    assert (_lib.REGRIDMETHOD_NEAREST_DTOS, _lib.DTOS_SUM, _lib.DTOS_MEAN) == (5, 0, 1)
    # the warm-up anchor, the drain, the one added line of mpg_handle_mask, and the kernel file's promises
    api = open(os.path.join(build.CSRC, "mpg_api.hip")).read()
    body = api[api.index("int " + STORE + "("):api.index("int " + NEAREST + "(")]
    assert re.search(r"X\(k_store_dtos\)", api) and "store_worker_drain();" in body and "mpg_k_store_dtos(" in body
    mask = api[api.index("int mpg_handle_mask("):api.index("int mpg_handle_patch(")]
    assert "MPG_REGRIDMETHOD_NEAREST_DTOS" in mask and "mpg_regrid_store_nearest_dtos" in mask
    kern = open(os.path.join(build.CSRC, "k_store_dtos.hip")).read()
    for word in ("mpg_anchor_k_store_dtos", "dtos_nearest(", "dtos_nearest_masked(", "dtos_value(", "mpg_scan_excl_i32", "mpg_sum_i32_i64",
                 "mpg_sort_pairs_u64_i32", "mpg_k_morton", "boxdist2_nofma", "mpg_k_build_bvh(dst_mesh, s, true)", '#include "knn_src.h"'):
        assert word in kern, word
    code = re.sub(r"//[^\n]*", "", kern)
    # integer atomics count and take a maximum; none returns a slot: nothing is placed by arrival order
    assert not re.search(r"=\s*atomic\w+\s*\(", code) and not re.search(r"atomic(Exch|CAS)\s*\(", code)
    assert not re.search(r"atomicAdd\s*\(\s*&?\s*\(?\s*(float|double)", code)
    dtos = open(os.path.join(build.CSRC, "dtos.h")).read()
    assert "KBest<1>" in dtos and "knn_search(" in dtos and "knn_search_masked(" in dtos and "hip/hip_runtime.h" not in dtos and "TW_FN" in dtos
    assert "1.0 / (double)len" in dtos
    # the searched sets live in ONE header: moved out of k_extrapolate.hip, not copied
    shared = open(os.path.join(build.CSRC, "knn_src.h")).read()
    ex = open(os.path.join(build.CSRC, "k_extrapolate.hip")).read()
    for s in ("struct ExMeshSrc", "struct ExGridSrc"):
        assert shared.count(s) == 1 and s not in ex and s not in kern
    assert '#include "knn_src.h"' in ex
    leaves = re.findall(r"void leaf_masked\(.*?\n  \}", shared, flags=re.S)
    assert len(leaves) == 2
    for leaf in leaves:
        assert leaf.index("mask[") < leaf.index("dist2_nofma"), "the mask is tested before a distance is computed"


def test_python_signatures():
    from mpassit_amd import regrid as R, target_grid as tg
    sig = inspect.signature(R.regrid_store_nearest_dtos)
    assert list(sig.parameters) == ["src", "dst", "norm", "src_mask", "dst_mask", "src_loc", "dst_loc"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == {"norm": R.DTOS_SUM, "src_mask": None, "dst_mask": None, "src_loc": None, "dst_loc": None}
    for name in ("regrid_store_nearest_dtos", "REGRIDMETHOD_NEAREST_DTOS", "DTOS_SUM", "DTOS_MEAN"):
        assert name in R.__all__
    assert (R.REGRIDMETHOD_NEAREST_DTOS, R.DTOS_SUM, R.DTOS_MEAN) == (5, 0, 1) == (5, tg.DTOS_SUM, tg.DTOS_MEAN)
    assert list(inspect.signature(R.RouteHandle.src_nearest).parameters) == ["self"]
    assert list(inspect.signature(tg.nearest_dtos_rows).parameters) == ["src_xyz", "dst_xyz", "norm", "src_mask", "dst_mask"]


def _fortran_interface(src, name):
    m = re.search(r"function\s+%s\s*\(([^)]*)\)\s*&?\s*bind\s*\(\s*C\s*,\s*name\s*=\s*['\"]%s['\"]\s*\)(.*?)end\s+function" % (name, name),
                  src, flags=re.S | re.I)
    assert m, name + " has no bind(C) interface in mpg_mod.F90"
    return [a.strip().lower() for a in m.group(1).replace("&", " ").split(",")], m.group(2).lower()


def test_fortran_binds_them():
    src = open(os.path.join(ROOT, "mpassit_amd", "fortran", "mpg_mod.F90")).read()
    low = src.lower()
    assert re.search(r"mpg_regridmethod_nearest_dtos\s*=\s*5\b", low) and re.search(r"mpg_dtos_sum\s*=\s*0\s*,\s*mpg_dtos_mean\s*=\s*1\b", low)
    args, body = _fortran_interface(src, STORE)
    assert args == ["src", "dst", "norm", "src_mask_dev", "dst_mask_dev", "out"]
    assert re.search(r"type\(mpg_points\),\s*intent\(in\)\s*::\s*src,\s*dst", body) and re.search(r"integer\(c_int\),\s*value\s*::\s*norm\b", body)
    assert re.search(r"type\(c_ptr\),\s*value\s*::\s*src_mask_dev,\s*dst_mask_dev", body) and re.search(r"type\(c_ptr\),\s*intent\(out\)\s*::\s*out\b", body)
    args, body = _fortran_interface(src, NEAREST)
    assert args == ["rh", "nearest_host"]
    assert re.search(r"type\(c_ptr\),\s*value\s*::\s*rh\b", body) and re.search(r"integer\(c_int32_t\),\s*intent\(out\)\s*::\s*nearest_host\(\*\)", body)
    # the driver does not use them
    drv = open(os.path.join(ROOT, "mpassit_amd", "fortran", "mpassit_driver.F90")).read().lower()
    assert "nearest_dtos" not in drv
