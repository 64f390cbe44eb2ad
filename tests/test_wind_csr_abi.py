"""CPU checks of the two wind calls for CSR handles: the header declares mpg_wind_csr_to_mesh_dev and mpg_wind_csr_to_edges_dev with
the argument lists of their fixed-handle twins, between mpg_wind_to_edges_dev and the output epilogues, and states the value rule; the
two fixed-handle calls' comments name them; _lib lists and binds both, the built library exports them, the kernel file is part of the
build, the Python wrappers have the agreed signatures, and the Fortran module has matching bind(C) interfaces (which the driver does
not use)."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH, EDGES = "mpg_wind_csr_to_mesh_dev", "mpg_wind_csr_to_edges_dev"
ARGS = {
    MESH: ["mpg_handle rh_u", "mpg_handle rh_v", "const double *cosa_dev", "const double *sina_dev", "const void *u_dev", "const void *v_dev",
           "int src_type", "int64_t u_level_stride", "int64_t v_level_stride", "int nlev", "void *ue_dev", "void *ve_dev", "int dst_type",
           "int dst_layout", "void *hip_stream"],
    EDGES: ["mpg_handle rh_u", "mpg_handle rh_v", "const double *cn_dev", "const double *sn_dev", "const void *u_dev", "const void *v_dev",
            "int src_type", "int64_t u_level_stride", "int64_t v_level_stride", "int nlev", "void *un_dev", "void *ut_dev", "int dst_type",
            "int dst_layout", "void *hip_stream"],
}


def _header(strip_comments=True):
    txt = open(os.path.join(ROOT, "include", "mpassit_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S) if strip_comments else txt


def _doc(name, start):
    txt = _header(strip_comments=False)
    i = txt.index("int " + name + "(")
    doc = " ".join(txt[max(0, i - 9000):i].replace("\n *", "\n").split())
    return doc[doc.rindex(start):]


def test_header_declares_both_calls():
    txt = _header()
    for name, want in ARGS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, name + " is not declared"
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want
    full = _header(strip_comments=False)
    assert full.index("int mpg_wind_to_edges_dev(") < full.index("int " + MESH + "(") < full.index("int " + EDGES + "(") < full.index("---- output epilogues")
    assert full.index("int " + EDGES + "(") < full.index("int mpg_dev_alloc(")


def test_header_states_the_rule():
    doc = _doc(MESH, "Winds through CSR handles")
    for phrase in ("acc = fma(val[q]", "in stored order", "whatever LDS chunk", "a = fma(acc_u, 1.0, 0.0)",
                   "mpg_regrid_csr_to_mesh_dev(rh_u, dst F64, scale 1, offset 0)", "b = fma(acc_v, 1.0, 0.0)",
                   "ue = a * ca - b * sa ; ve = a * sa + b * ca", "un = a * cn + b * sn ; ut = b * cn - a * sn", "ut_dev != NULL",
                   "one rounding to the destination type", "row is empty in either handle", "(TD)(+0.0)", "-0.0", "hipGraph", "No atomics",
                   "rh_u == rh_v", "ONE run", "nnz_per_row 0", "mpg_regrid_store_periodic_to_mesh", "mpg_handle_from_weights",
                   "do not look at the mesh", "REQUIRED", "0 = dense", "MPG_ERR_UNSUPPORTED", "mpg_wind_to_mesh_dev / mpg_wind_to_edges_dev",
                   "mpg_handle_pole_count > 0", "MPG_TYPE_BE", "MPG_ERR_INVALID_ARG", "exactly one NULL angle", "a level stride below n_src",
                   "aliasing", "MPG_ERR_OVERFLOW", "mpg_wind_csr_to_mesh / mpg_wind_csr_to_edges",
                   "MPG_POLEMETHOD_ALLAVG", "row mean of each wind COMPONENT", "not a wind", "MPG_POLEMETHOD_NONE"):
        assert phrase in doc, phrase
    # the two fixed-handle calls keep refusing CSR handles and name the call that takes them
    old = _doc("mpg_wind_to_mesh_dev", "The wind chain turned round")
    assert "CSR handles" in old and "pole caps" in old and MESH in old and "out of scope" not in old
    old = _doc("mpg_wind_to_edges_dev", "Winds onto mesh EDGES")
    assert "CSR handles" in old and "pole caps" in old and EDGES in old and "out of scope" not in old
    # the periodic Store's comment names the edge location
    store = _doc("mpg_regrid_store_periodic_to_mesh", "Periodic Grid -> Mesh: ESMF_FieldRegridStore")
    assert "MPG_MESHLOC_EDGE" in store and "mpg_mesh_set_edges" in store


def test_lib_lists_binds_and_exports_them():
    from mpassit_amd import _lib, build
    for name in ARGS:
        assert name in _lib.SYMBOLS
    assert "k_wind_csr.hip" in build.SOURCES and "k_wind_pair.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "k_wind_csr.hip"))
    build.build()
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    for name in ARGS:
        assert hasattr(lib, name)
        assert re.search(r" T %s\b" % name, out)
    for proto in (_lib._WIND_CSR_TO_MESH_PROTO, _lib._WIND_CSR_TO_EDGES_PROTO):
        at = proto._argtypes_
        assert len(at) == 15 and proto._restype_ is C.c_int
        assert at[7] is C.c_int64 and at[8] is C.c_int64, "the level strides are 64-bit"
        assert [at[i] for i in (6, 9, 12, 13)] == [C.c_int] * 4
        assert all(at[i] is C.c_void_p for i in (0, 1, 2, 3, 4, 5, 10, 11, 14))
    assert callable(_lib.wind_csr_to_mesh_dev) and callable(_lib.wind_csr_to_edges_dev)


def test_python_signatures():
    from mpassit_amd import regrid as R
    sig = inspect.signature(R.wind_csr_to_mesh)
    assert list(sig.parameters) == ["rh_u", "rh_v", "cosa", "sina", "u", "v", "nlev", "layout", "out_dtype", "outs"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["layout"], d["out_dtype"], d["outs"]) == (R.LAYOUT_CELL_FAST, None, None) and d["nlev"] is inspect.Parameter.empty
    sig = inspect.signature(R.wind_csr_to_edges)
    assert list(sig.parameters) == ["rh_u", "rh_v", "cn", "sn", "u", "v", "nlev", "layout", "out_dtype", "tangential", "outs"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["layout"], d["out_dtype"], d["tangential"], d["outs"]) == (R.LAYOUT_CELL_FAST, None, False, None)
    assert d["nlev"] is inspect.Parameter.empty and d["cn"] is inspect.Parameter.empty
    # the differentiable ops have the signatures of their fixed twins
    assert inspect.signature(R.wind_csr_to_mesh_autograd) == inspect.signature(R.wind_to_mesh_autograd)
    assert inspect.signature(R.wind_csr_to_edges_autograd) == inspect.signature(R.wind_to_edges_autograd)
    for name in ("wind_csr_to_mesh", "wind_csr_to_edges", "wind_csr_to_mesh_autograd", "wind_csr_to_edges_autograd"):
        assert name in R.__all__
    assert "MESHLOC_EDGE" in inspect.getdoc(R.regrid_store_periodic_to_mesh)
    assert list(inspect.signature(R.regrid_store_periodic_to_mesh).parameters) == ["src_grid", "dst_mesh", "meshloc", "pole_method"]


def _fortran_interface(src, name):
    m = re.search(r"function\s+%s\s*\(([^)]*)\)\s*&?\s*bind\s*\(\s*C\s*,\s*name\s*=\s*['\"]%s['\"]\s*\)(.*?)end\s+function" % (name, name),
                  src, flags=re.S | re.I)
    assert m, name + " has no bind(C) interface in mpg_mod.F90"
    return [a.strip().lower() for a in m.group(1).replace("&", " ").split(",")], m.group(2).lower(), m.start()


def test_fortran_binds_them():
    src = open(os.path.join(ROOT, "mpassit_amd", "fortran", "mpg_mod.F90")).read()
    want = {MESH: ["rh_u", "rh_v", "cosa_dev", "sina_dev", "u_dev", "v_dev", "src_type", "u_level_stride", "v_level_stride", "nlev", "ue_dev",
                   "ve_dev", "dst_type", "dst_layout", "hip_stream"],
            EDGES: ["rh_u", "rh_v", "cn_dev", "sn_dev", "u_dev", "v_dev", "src_type", "u_level_stride", "v_level_stride", "nlev", "un_dev",
                    "ut_dev", "dst_type", "dst_layout", "hip_stream"]}
    beside = re.search(r"end\s+function\s+mpg_wind_to_edges_dev", src).end()
    for name, names in want.items():
        args, body, at = _fortran_interface(src, name)
        assert args == names
        for a in ("src_type", "nlev", "dst_type", "dst_layout"):
            assert re.search(r"integer\(c_int\),\s*value\s*::.*\b%s\b" % a, body), a
        for a in ("u_level_stride", "v_level_stride"):
            assert re.search(r"integer\(c_int64_t\),\s*value\s*::.*\b%s\b" % a, body), a
        for a in [x for x in names if x not in ("src_type", "nlev", "dst_type", "dst_layout", "u_level_stride", "v_level_stride")]:
            assert re.search(r"type\(c_ptr\),\s*value\s*::.*\b%s\b" % a, body), a
        assert beside < at < src.index("function mpg_dev_alloc"), "beside mpg_wind_to_edges_dev"
    # the driver and interp_mod do not use them: the reference's job takes no wind back to the mesh
    for f in ("interp_mod.F90", "mpassit_driver.F90"):
        txt = open(os.path.join(ROOT, "mpassit_amd", "fortran", f)).read()
        for name in ARGS:
            assert name not in txt
