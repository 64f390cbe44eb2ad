"""CPU checks of the extrapolation calls: the header declares mpg_handle_extrapolate, mpg_mesh_get_xyz and mpg_grid_get_xyz with the agreed
argument lists and the two structs -- the new section behind mpg_compose_weights_dev and before the output epilogues, the getters behind
mpg_mesh_get_triangles -- and states the contract; _lib lists, binds and exports the three; the kernel file and knn.h are part of the
build and keep their promises; the Python wrappers and the numpy mirror have the agreed signatures; the Fortran module has matching
bind(C) types and interfaces (which the driver does not use)."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAP, MESH_XYZ, GRID_XYZ = "mpg_handle_extrapolate", "mpg_mesh_get_xyz", "mpg_grid_get_xyz"
ARGS = {
    EXTRAP: ["mpg_handle rh", "const mpg_points *src", "const mpg_points *dst", "const mpg_extrap_opts *opts", "mpg_handle *out"],
    MESH_XYZ: ["mpg_mesh mesh", "int meshloc", "double *xyz_host"],
    GRID_XYZ: ["mpg_grid grid", "int staggerloc", "double *xyz_host"],
}


def _header(strip_comments=True):
    txt = open(os.path.join(ROOT, "include", "mpassit_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S) if strip_comments else txt


def test_header_declares_the_calls_and_the_structs():
    txt = _header()
    for name, want in ARGS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, name + " is not declared"
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want
        assert len(want) <= 14
    assert re.search(r"enum\s*\{\s*MPG_EXTRAPMETHOD_NEAREST_STOD\s*=\s*1\s*,\s*MPG_EXTRAPMETHOD_NEAREST_IDAVG\s*=\s*2\s*\}", txt)
    assert re.search(r"#define\s+MPG_EXTRAP_MAX_PNTS\s+8\b", txt)
    pts = re.search(r"typedef\s+struct\s+mpg_points\s*\{(.*?)\}\s*mpg_points\s*;", txt, flags=re.S).group(1)
    assert [" ".join(f.split()) for f in pts.split(";") if f.strip()] == ["mpg_mesh mesh", "int meshloc", "mpg_grid grid", "int staggerloc"]
    opts = re.search(r"typedef\s+struct\s+mpg_extrap_opts\s*\{(.*?)\}\s*mpg_extrap_opts\s*;", txt, flags=re.S).group(1)
    assert [" ".join(f.split()) for f in opts.split(";") if f.strip()] == ["int method", "int num_src_pnts", "double dist_exponent"]
    full = _header(strip_comments=False)
    at = full.index("int " + EXTRAP + "(")
    assert full.index("int mpg_compose_weights_dev(") < full.index("---- extrapolation") < at < full.index("---- output epilogues")
    tri = full.index("int mpg_mesh_get_triangles(")
    assert tri < full.index("int " + MESH_XYZ + "(") < full.index("int " + GRID_XYZ + "(") < full.index("int mpg_handle_unique_sources(")


def test_header_states_the_contract():
    txt = _header(strip_comments=False)
    i = txt.index("int " + EXTRAP + "(")
    doc = " ".join(txt[max(0, i - 9000):i].replace("\n *", "\n").split())
    doc = doc[doc.rindex("---- extrapolation"):]
    for phrase in ("extrapMethod", "extrapNumSrcPnts", "extrapDistExponent", "an ordinary handle",
                   # the point sets
                   "exactly one of mesh / grid is non-NULL", "MPG_MESHLOC_ELEMENT", "site BVH built whole", "point pyramid", "cells, vertices or edges",
                   "Mesh -> Grid, Mesh -> Mesh, Grid -> Mesh and Grid -> Grid",
                   # the rows and the neighbours
                   "slot 0's index < 0", "an empty row", "copied verbatim", "dist2_nofma", "stored unit vectors", "K = min(N, n_src)",
                   "lexicographic (d2, id)", "j * snx + i", "Ties go to the lower id", "including the last",
                   # the values
                   "one entry (c0, 1.0)", "d2_0 == 0.0", "r_i = d2_0 / d2_i", "t_i = r_i when e == 2.0", "pow(r_i, 0.5 * e)", "from left to right",
                   "w_i = t_i / S", "rounded on its own", "fp contract(off)", "(1/d^e) / sum(1/d^e)", "Nothing overflows".lower(), "underflow to weight 0",
                   "ascending (d2, id) order", "summation order", "target_grid.extrapolate_rows",
                   # the output
                   "n_src, n_dst, nx_dst, ny_dst and method", "not cached", "owns its arrays", "mpg_handle_release", "no dst_frac",
                   "mpg_handle_store_ms", "mpg_handle_store_stats", "rows filled", "STOD always, IDAVG when N <= S", "slots 0 .. k - 1",
                   "repeats entry 0's id with weight +0.0", "stays without one", "staged kernels", "slot order", "weight 1.0", "stored order",
                   "longest row is recorded", "Nothing unmapped is success",
                   # determinism, blocking, refusals
                   "same bytes from run to run", "no floating-point atomics", "drains the Store worker", "mpg_handle_get_csr",
                   "names mpg_handle_extrapolate", "MPG_ERR_INVALID_ARG", "NULL argument", "both or neither", "unknown method",
                   "1..MPG_EXTRAP_MAX_PNTS", "not finite or <= 0", "both numbers are printed", "node-located handle",
                   "location other than ELEMENT", "mesh without edges", "MPG_ERR_UNSUPPORTED", "mpg_handle_pole_count > 0",
                   "localized or rebased", "source window", "MPG_ERR_OVERFLOW", "2^31 - 2 entries", "leaks nothing"):
        assert phrase in doc or phrase in doc.lower(), phrase
    g = txt.index("int " + MESH_XYZ + "(")
    assert "stored unit vectors" in txt[g - 600:g] and "[3][n]" in txt[g - 600:g + 200]


def test_lib_lists_binds_and_exports_them():
    from mpassit_amd import _lib, build
    for name in ARGS:
        assert name in _lib.SYMBOLS
    assert "k_extrapolate.hip" in build.SOURCES and "knn.h" in build.HEADERS
    assert os.path.exists(os.path.join(build.CSRC, "k_extrapolate.hip")) and os.path.exists(os.path.join(build.CSRC, "knn.h"))
    build.build()
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    for name in ARGS:
        assert hasattr(lib, name)
        assert re.search(r" T %s\b" % name, out)
    assert [f[0] for f in _lib.Points._fields_] == ["mesh", "meshloc", "grid", "staggerloc"]
    assert [f[1] for f in _lib.Points._fields_] == [C.c_void_p, C.c_int, C.c_void_p, C.c_int] and C.sizeof(_lib.Points) == 32
    assert [f[0] for f in _lib.ExtrapOpts._fields_] == ["method", "num_src_pnts", "dist_exponent"]
    assert [f[1] for f in _lib.ExtrapOpts._fields_] == [C.c_int, C.c_int, C.c_double] and C.sizeof(_lib.ExtrapOpts) == 16
    at = _lib._HANDLE_EXTRAPOLATE_PROTO._argtypes_
    assert list(at) == [C.c_void_p, C.POINTER(_lib.Points), C.POINTER(_lib.Points), C.POINTER(_lib.ExtrapOpts), C.c_void_p]
    assert _lib._HANDLE_EXTRAPOLATE_PROTO._restype_ is C.c_int
    for proto in (_lib._MESH_GET_XYZ_PROTO, _lib._GRID_GET_XYZ_PROTO):
        assert list(proto._argtypes_) == [C.c_void_p, C.c_int, C.c_void_p] and proto._restype_ is C.c_int
    assert callable(_lib.handle_extrapolate) and callable(_lib.mesh_get_xyz) and callable(_lib.grid_get_xyz)
    assert (_lib.EXTRAPMETHOD_NEAREST_STOD, _lib.EXTRAPMETHOD_NEAREST_IDAVG, _lib.EXTRAP_MAX_PNTS) == (1, 2, 8)
    # the warm-up anchor and the kernel file's promises
    api = open(os.path.join(build.CSRC, "mpg_api.hip")).read()
    assert re.search(r"X\(k_extrapolate\)", api) and "store_worker_drain();" in api[api.index("int mpg_handle_extrapolate("):api.index("mpg_k_extrapolate(rh")]
    kern = open(os.path.join(build.CSRC, "k_extrapolate.hip")).read()
    assert "mpg_anchor_k_extrapolate" in kern and "mpg_scan_excl_i32" in kern and "knn_search" in kern and "knn_weights" in kern
    for inst in ("k_ex_knn<Src, 1>", "k_ex_knn<Src, 2>", "k_ex_knn<Src, 4>", "k_ex_knn<Src, 8>", "dist2_nofma", "boxdist2_nofma", "mpg_k_build_bvh(src_mesh, s, true)"):
        assert inst in kern, inst
    code = re.sub(r"//[^\n]*", "", kern)
    assert not re.search(r"atomic(Add|Exch|CAS)\s*\(", code) and "__shared__" not in code       # (one integer atomicMax: the longest row)
    knn = open(os.path.join(build.CSRC, "knn.h")).read()
    assert "fp contract(off)" in knn and "walk_nearest" in knn and "hip/hip_runtime.h" not in knn and "TW_FN" in knn


def test_python_signatures():
    from mpassit_amd import regrid as R, target_grid as tg
    sig = inspect.signature(R.extrapolate)
    assert list(sig.parameters) == ["rh", "src", "dst", "method", "num_src_pnts", "dist_exponent", "src_loc", "dst_loc"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == {"method": R.EXTRAPMETHOD_NEAREST_STOD, "num_src_pnts": 8, "dist_exponent": 2.0, "src_loc": None, "dst_loc": None}
    for name in ("extrapolate", "EXTRAPMETHOD_NEAREST_STOD", "EXTRAPMETHOD_NEAREST_IDAVG", "EXTRAP_MAX_PNTS"):
        assert name in R.__all__
    assert list(inspect.signature(R.Mesh.xyz).parameters) == ["self", "meshloc"] and list(inspect.signature(R.Grid.xyz).parameters) == ["self", "staggerloc"]
    assert inspect.signature(R.Mesh.xyz).parameters["meshloc"].default == R.MESHLOC_ELEMENT
    assert inspect.signature(R.Grid.xyz).parameters["staggerloc"].default == R.STAGGERLOC_CENTER
    assert list(inspect.signature(tg.extrapolate_rows).parameters) == ["src_xyz", "dst_xyz", "unmapped", "method", "num_src_pnts", "dist_exponent"]
    assert (tg.EXTRAPMETHOD_NEAREST_STOD, tg.EXTRAPMETHOD_NEAREST_IDAVG) == (R.EXTRAPMETHOD_NEAREST_STOD, R.EXTRAPMETHOD_NEAREST_IDAVG)


def _fortran_interface(src, name):
    m = re.search(r"function\s+%s\s*\(([^)]*)\)\s*&?\s*bind\s*\(\s*C\s*,\s*name\s*=\s*['\"]%s['\"]\s*\)(.*?)end\s+function" % (name, name),
                  src, flags=re.S | re.I)
    assert m, name + " has no bind(C) interface in mpg_mod.F90"
    return [a.strip().lower() for a in m.group(1).replace("&", " ").split(",")], m.group(2).lower(), m.start()


def test_fortran_binds_them():
    src = open(os.path.join(ROOT, "mpassit_amd", "fortran", "mpg_mod.F90")).read()
    low = src.lower()
    assert re.search(r"type\s*,\s*bind\(c\)\s*::\s*mpg_points(.*?)end\s+type\s+mpg_points", low, flags=re.S)
    body = re.search(r"type\s*,\s*bind\(c\)\s*::\s*mpg_points(.*?)end\s+type\s+mpg_points", low, flags=re.S).group(1)
    order = [body.index(k) for k in (":: mesh", ":: meshloc", ":: grid", ":: staggerloc")]
    assert order == sorted(order) and body.count("type(c_ptr)") == 2 and body.count("integer(c_int)") == 2
    body = re.search(r"type\s*,\s*bind\(c\)\s*::\s*mpg_extrap_opts(.*?)end\s+type\s+mpg_extrap_opts", low, flags=re.S).group(1)
    order = [body.index(k) for k in (":: method", ":: num_src_pnts", ":: dist_exponent")]
    assert order == sorted(order) and "real(c_double) :: dist_exponent" in body
    assert re.search(r"mpg_extrapmethod_nearest_stod\s*=\s*1\s*,\s*mpg_extrapmethod_nearest_idavg\s*=\s*2", low) and re.search(r"mpg_extrap_max_pnts\s*=\s*8", low)
    beside = re.search(r"end\s+function\s+mpg_compose_weights_dev", src).end()
    args, body, at = _fortran_interface(src, EXTRAP)
    assert args == ["rh", "src", "dst", "opts", "out"]
    assert re.search(r"type\(c_ptr\),\s*value\s*::\s*rh\b", body) and re.search(r"type\(mpg_points\),\s*intent\(in\)\s*::\s*src,\s*dst", body)
    assert re.search(r"type\(mpg_extrap_opts\),\s*intent\(in\)\s*::\s*opts", body) and re.search(r"type\(c_ptr\),\s*intent\(out\)\s*::\s*out", body)
    assert "mpg_points" in body.split("\n")[1] and "mpg_extrap_opts" in body.split("\n")[1], "the types are imported"
    assert beside < at < src.index("function mpg_dev_alloc"), "after mpg_compose_weights_dev, before mpg_dev_alloc"
    for name, loc in ((MESH_XYZ, "meshloc"), (GRID_XYZ, "staggerloc")):
        args, body, at2 = _fortran_interface(src, name)
        assert args == [name.split("_")[1], loc, "xyz_host"]
        assert re.search(r"integer\(c_int\),\s*value\s*::\s*%s\b" % loc, body) and re.search(r"type\(c_ptr\),\s*value\s*::.*\bxyz_host\b", body)
        assert at < at2 < src.index("function mpg_dev_alloc")
    for f in ("interp_mod.F90", "mpassit_driver.F90"):
        txt = open(os.path.join(ROOT, "mpassit_amd", "fortran", f)).read()
        for name in ARGS:
            assert name not in txt
