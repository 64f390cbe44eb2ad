"""CPU checks of the three calls of the Cartesian-vector wind Regrid: the header declares mpg_sphere_frames_dev,
mpg_wind_vector_weights_dev and mpg_wind_vector_dev with the agreed argument lists, between mpg_wind_csr_to_edges_dev and the output
epilogues, and states the frames, the blocks and the value rule; the CSR wind calls' caveat names the new call; _lib lists and binds the
three, the built library exports them, the kernel file is part of the build, the Python wrappers have the agreed signatures, and the
Fortran module has matching bind(C) interfaces (which the driver does not use)."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES, WEIGHTS, APPLY = "mpg_sphere_frames_dev", "mpg_wind_vector_weights_dev", "mpg_wind_vector_dev"
ARGS = {
    FRAMES: ["int64_t n", "const double *lon_dev", "const double *lat_dev", "const double *c_dev", "const double *s_dev", "double *frames_dev",
             "void *hip_stream"],
    WEIGHTS: ["mpg_handle rh", "const double *src_frames_dev", "const double *dst_frames_dev", "double *m_dev", "void *hip_stream"],
    APPLY: ["mpg_handle rh", "const double *m_dev", "const void *u_dev", "const void *v_dev", "int src_type", "int64_t u_level_stride",
            "int64_t v_level_stride", "int nlev", "void *r0_dev", "void *r1_dev", "int dst_type", "int dst_layout", "void *hip_stream"],
}


def _header(strip_comments=True):
    txt = open(os.path.join(ROOT, "include", "mpassit_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S) if strip_comments else txt


def _doc(name, start):
    txt = _header(strip_comments=False)
    i = txt.index("int " + name + "(")
    doc = " ".join(txt[max(0, i - 9000):i].replace("\n *", "\n").split())
    return doc[doc.rindex(start):]


def test_header_declares_the_three_calls():
    txt = _header()
    for name, want in ARGS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, name + " is not declared"
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want
    assert len(ARGS[APPLY]) == 13
    full = _header(strip_comments=False)
    at = [full.index("int " + n + "(") for n in (FRAMES, WEIGHTS, APPLY)]
    assert full.index("int mpg_wind_csr_to_edges_dev(") < at[0] < at[1] < at[2] < full.index("---- output epilogues")
    assert at[2] < full.index("int mpg_dev_alloc(")


def test_header_states_the_contract():
    doc = _doc(FRAMES, "A wind as a VECTOR")
    for phrase in ("vectorRegrid", "one 2 x 2 block per CSR entry", "once per (handle, frames)", "hipGraph", "atomics",
                   "do not look at the mesh or the grid",
                   # frames
                   "[6][n]", "D0x D0y D0z D1x D1y D1z", "east = (-sin lon, cos lon, 0)", "north = (-sin lat cos lon, -sin lat sin lon, cos lat)",
                   "D0 = c east + s north", "D1 = c north - s east", "fp contract(off)", "radians", "angleEdge", "mpg_mesh_edge_rotang_dev",
                   "Exactly one NULL -> MPG_ERR_INVALID_ARG", "before the n == 0 success",
                   # blocks
                   "[6][n_src]", "[6][n_dst]", "[4][nnz]", "m00 m01 m10 m11", "CSR entry order", "The same bits as numpy",
                   "m00 = val[q] * ((e.x*D0.x + e.y*D0.y) + e.z*D0.z)", "m01 = val[q] * ((n.x*D0.x + n.y*D0.y) + n.z*D0.z)",
                   "nothing contracted", "4 * nnz doubles", "mpg_handle_info", "writes nothing",
                   # apply
                   "r1_dev may be NULL", "only the planes m00, m01 are read", "acc_kl = fma(m_kl[q], (double)src_l[col[q]], acc_kl)",
                   "in stored order", "whatever LDS chunk", "o0 = fma(acc00, 1.0, 0.0) + fma(acc01, 1.0, 0.0)",
                   "o1 = fma(acc10, 1.0, 0.0) + fma(acc11, 1.0, 0.0)", "one rounding to the destination type",
                   "mpg_regrid_csr_to_mesh_dev of a from-weights handle", "scale 1 and offset 0", "added once", "(TD)(+0.0)",
                   "both layouts", "dense and pitched sources", "from call to call", "0 = dense",
                   # refusals
                   "MPG_ERR_UNSUPPORTED", "mpg_handle_get_weights -> mpg_handle_from_weights", "mpg_handle_pole_count > 0", "MPG_TYPE_BE",
                   "MPG_ERR_INVALID_ARG", "nlev < 1", "a level stride below n_src", "aliasing", "m_dev", "MPG_ERR_OVERFLOW",
                   "MPG_POLEMETHOD_ALLAVG", "which is a wind"):
        assert phrase in doc, phrase
    # the caveat of the CSR wind calls now names the call that answers it
    old = _doc("mpg_wind_csr_to_mesh_dev", "Winds through CSR handles")
    assert "mpg_wind_vector_dev" in old and "is not built" not in old
    for phrase in ("MPG_POLEMETHOD_ALLAVG", "row mean of each wind COMPONENT", "not a wind", "MPG_POLEMETHOD_NONE"):
        assert phrase in old, phrase


def test_lib_lists_binds_and_exports_them():
    from mpassit_amd import _lib, build
    for name in ARGS:
        assert name in _lib.SYMBOLS
    assert "k_wind_vector.hip" in build.SOURCES and "k_wind_csr.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "k_wind_vector.hip"))
    build.build()
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    for name in ARGS:
        assert hasattr(lib, name)
        assert re.search(r" T %s\b" % name, out)
    at = _lib._SPHERE_FRAMES_PROTO._argtypes_
    assert len(at) == 7 and at[0] is C.c_int64 and all(a is C.c_void_p for a in at[1:]) and _lib._SPHERE_FRAMES_PROTO._restype_ is C.c_int
    at = _lib._WIND_VECTOR_WEIGHTS_PROTO._argtypes_
    assert len(at) == 5 and all(a is C.c_void_p for a in at) and _lib._WIND_VECTOR_WEIGHTS_PROTO._restype_ is C.c_int
    at = _lib._WIND_VECTOR_PROTO._argtypes_
    assert len(at) == 13 and _lib._WIND_VECTOR_PROTO._restype_ is C.c_int
    assert at[5] is C.c_int64 and at[6] is C.c_int64, "the level strides are 64-bit"
    assert [at[i] for i in (4, 7, 10, 11)] == [C.c_int] * 4
    assert all(at[i] is C.c_void_p for i in (0, 1, 2, 3, 8, 9, 12))
    assert callable(_lib.sphere_frames_dev) and callable(_lib.wind_vector_weights_dev) and callable(_lib.wind_vector_dev)
    # the warm-up anchor and the kernel's LDS chunk
    api = open(os.path.join(build.CSRC, "mpg_api.hip")).read()
    assert re.search(r"X\(k_wind_vector\)", api)
    assert "mpg_anchor_k_wind_vector" in open(os.path.join(build.CSRC, "k_wind_vector.hip")).read()


def test_python_signatures():
    from mpassit_amd import regrid as R, target_grid as tg
    sig = inspect.signature(R.sphere_frames)
    assert list(sig.parameters) == ["lon", "lat", "c", "s"] and sig.parameters["c"].default is None and sig.parameters["s"].default is None
    assert list(inspect.signature(R.wind_vector_weights).parameters) == ["rh", "src_frames", "dst_frames"]
    sig = inspect.signature(R.wind_vector)
    assert list(sig.parameters) == ["rh", "m", "u", "v", "nlev", "layout", "out_dtype", "second", "outs"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["layout"], d["out_dtype"], d["second"], d["outs"]) == (R.LAYOUT_CELL_FAST, None, True, None)
    assert d["nlev"] is inspect.Parameter.empty
    sig = inspect.signature(R.wind_vector_autograd)
    assert list(sig.parameters) == ["rh", "m", "u", "v", "nlev", "layout", "second"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["layout"], d["second"]) == (R.LAYOUT_CELL_FAST, True)
    for name in ("sphere_frames", "wind_vector_weights", "wind_vector", "wind_vector_autograd"):
        assert name in R.__all__
    # the numpy mirror stands next to rotang_at
    assert list(inspect.signature(tg.sphere_frames_at).parameters) == ["lon", "lat", "c", "s"]
    assert list(inspect.signature(tg.wind_vector_blocks).parameters) == ["rowptr", "col", "val", "src_frames", "dst_frames"]


def _fortran_interface(src, name):
    m = re.search(r"function\s+%s\s*\(([^)]*)\)\s*&?\s*bind\s*\(\s*C\s*,\s*name\s*=\s*['\"]%s['\"]\s*\)(.*?)end\s+function" % (name, name),
                  src, flags=re.S | re.I)
    assert m, name + " has no bind(C) interface in mpg_mod.F90"
    return [a.strip().lower() for a in m.group(1).replace("&", " ").split(",")], m.group(2).lower(), m.start()


def test_fortran_binds_them():
    src = open(os.path.join(ROOT, "mpassit_amd", "fortran", "mpg_mod.F90")).read()
    ints = {FRAMES: [], WEIGHTS: [], APPLY: ["src_type", "nlev", "dst_type", "dst_layout"]}
    int64s = {FRAMES: ["n"], WEIGHTS: [], APPLY: ["u_level_stride", "v_level_stride"]}
    beside = re.search(r"end\s+function\s+mpg_wind_csr_to_edges_dev", src).end()
    for name, decl in ARGS.items():
        names = [a.split()[-1].lstrip("*") for a in decl]
        args, body, at = _fortran_interface(src, name)
        assert args == names
        for a in ints[name]:
            assert re.search(r"integer\(c_int\),\s*value\s*::.*\b%s\b" % a, body), a
        for a in int64s[name]:
            assert re.search(r"integer\(c_int64_t\),\s*value\s*::.*\b%s\b" % a, body), a
        for a in [x for x in names if x not in ints[name] + int64s[name]]:
            assert re.search(r"type\(c_ptr\),\s*value\s*::.*\b%s\b" % a, body), a
        assert beside < at < src.index("function mpg_dev_alloc"), "after mpg_wind_csr_to_edges_dev, before mpg_dev_alloc"
    for f in ("interp_mod.F90", "mpassit_driver.F90"):
        txt = open(os.path.join(ROOT, "mpassit_amd", "fortran", f)).read()
        for name in ARGS:
            assert name not in txt
