"""CPU checks of the winds onto mesh edges: the header declares mpg_mesh_set_edges, mpg_mesh_edge_count, mpg_mesh_edge_rotang_dev and
mpg_wind_to_edges_dev with their exact argument lists, the enum value MPG_MESHLOC_EDGE = 2 and the value rule, _lib lists and binds the
four, the built library exports them, the Python wrappers have the agreed signatures, and the Fortran module has matching bind(C)
interfaces (which the driver does not use)."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SET, COUNT, ROTANG, WIND = "mpg_mesh_set_edges", "mpg_mesh_edge_count", "mpg_mesh_edge_rotang_dev", "mpg_wind_to_edges_dev"
ARGS = {
    SET: ["mpg_mesh mesh", "int64_t nEdges", "const double *latEdge", "const double *lonEdge", "const double *angleEdge"],
    COUNT: ["mpg_mesh mesh", "int64_t *nEdges"],
    ROTANG: ["mpg_grid grid", "mpg_mesh mesh", "double *cn_dev", "double *sn_dev", "void *hip_stream"],
    WIND: ["mpg_handle rh_u", "mpg_handle rh_v", "const double *cn_dev", "const double *sn_dev", "const void *u_dev", "const void *v_dev",
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


def test_header_declares_the_calls():
    txt = _header()
    for name, want in ARGS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, name + " is not declared"
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want
    assert re.search(r"enum\s*\{\s*MPG_MESHLOC_ELEMENT\s*=\s*0\s*,\s*MPG_MESHLOC_NODE\s*=\s*1\s*,\s*MPG_MESHLOC_EDGE\s*=\s*2\s*\}\s*;", txt)
    full = _header(strip_comments=False)
    # after mpg_mesh_rotang_dev, before the output epilogues; the edges next to the mesh constructors
    assert full.index("int mpg_mesh_rotang_dev(") < full.index("int " + ROTANG + "(") < full.index("int " + WIND + "(") < full.index("int mpg_dev_alloc(")
    assert full.index("int " + WIND + "(") < full.index("---- output epilogues")
    assert full.index("int mpg_mesh_create_window(") < full.index("int " + SET + "(") < full.index("int " + COUNT + "(") < full.index("int mpg_grid_create(")


def test_header_states_the_rule():
    doc = _doc(WIND, "Winds onto mesh EDGES")
    for phrase in ("a = fma(wsum_fixed<NNZ>(w_u, U[idx_u]), 1.0, 0.0)", "exactly mpg_regrid_to_mesh_dev(rh_u, dst F64, scale 1, offset 0)",
                   "b = fma(wsum_fixed<NNZ>(w_v, V[idx_v]), 1.0, 0.0)", "un = a * cn + b * sn", "two products and one sum, each rounded",
                   "ut = b * cn - a * sn", "only when ut_dev != NULL", "90 degrees counter-clockwise of the normal", "store (TD)un [, (TD)ut]",
                   "one rounding to the destination type", "either handle", "(TD)(+0.0) in every result", "hipGraph", "MPG_TYPE_BE",
                   "CSR handles", "pole caps", "No atomics", "MPG_ERR_UNSUPPORTED", "MPG_ERR_INVALID_ARG", "MPG_ERR_OVERFLOW", "rh_u == rh_v",
                   "u_level_stride", "MPG_LAYOUT_LEV_FAST [edge][lev]", "u(nEdges, nVertLevels)", "REQUIRED", "cos / sin of angleEdge",
                   "does not look at the mesh", "mpg_wind_to_edges"):
        assert phrase in doc, phrase
    doc = _doc(ROTANG, "The same angles for the mesh's EDGES")
    for phrase in ("phi = angleEdge - alpha", "one float64 subtraction", "-hemi * cone * wrap180(lon - stand_lon)", "atan2(y, x)",
                   "grid == NULL gives alpha = 0", "pass a NULL grid", "mpg_mesh_set_edges", "allocates nothing"):
        assert phrase in doc, phrase
    doc = _doc(SET, "The mesh's EDGES")
    for phrase in ("radians", "bit for bit", "may be NULL", "edges are already set", "MPG_ERR_OVERFLOW", "mpg_mesh_create_window",
                   "DESTINATION location only", "freed with the mesh", "|lat| > pi/2", "nEdges < 1"):
        assert phrase in doc, phrase


def test_lib_lists_binds_and_exports_them():
    from mpassit_amd import _lib, build
    for name in ARGS:
        assert name in _lib.SYMBOLS
    assert _lib.MESHLOC_EDGE == 2
    assert "k_wind_pair.hip" in build.SOURCES
    build.build()
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    for name in ARGS:
        assert hasattr(lib, name)
        assert re.search(r" T %s\b" % name, out)
    at = _lib._WIND_TO_EDGES_PROTO._argtypes_
    assert len(at) == 15 and _lib._WIND_TO_EDGES_PROTO._restype_ is C.c_int
    assert at[7] is C.c_int64 and at[8] is C.c_int64, "the level strides are 64-bit"
    assert [at[i] for i in (6, 9, 12, 13)] == [C.c_int] * 4
    assert all(at[i] is C.c_void_p for i in (0, 1, 2, 3, 4, 5, 10, 11, 14))
    at = _lib._MESH_EDGE_ROTANG_PROTO._argtypes_
    assert len(at) == 5 and all(a is C.c_void_p for a in at) and _lib._MESH_EDGE_ROTANG_PROTO._restype_ is C.c_int
    at = _lib._MESH_SET_EDGES_PROTO._argtypes_
    assert len(at) == 5 and at[1] is C.c_int64, "nEdges is 64-bit"
    assert len(_lib._MESH_EDGE_COUNT_PROTO._argtypes_) == 2
    for f in ("mesh_set_edges", "mesh_edge_count", "mesh_edge_rotang_dev", "wind_to_edges_dev"):
        assert callable(getattr(_lib, f))


def test_python_signatures():
    from mpassit_amd import regrid as R, synth, target_grid as tg
    sig = inspect.signature(R.wind_to_edges)
    assert list(sig.parameters) == ["rh_u", "rh_v", "cn", "sn", "u", "v", "nlev", "layout", "out_dtype", "tangential", "outs"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["layout"], d["out_dtype"], d["tangential"], d["outs"]) == (R.LAYOUT_CELL_FAST, None, False, None)
    assert d["nlev"] is inspect.Parameter.empty and d["cn"] is inspect.Parameter.empty
    assert list(inspect.signature(R.mesh_edge_rotang).parameters) == ["grid", "mesh"]
    sig = inspect.signature(R.wind_to_edges_autograd)
    assert list(sig.parameters) == ["rh_u", "rh_v", "cn", "sn", "u", "v", "nlev", "layout", "tangential"]
    assert sig.parameters["layout"].default == R.LAYOUT_CELL_FAST and sig.parameters["tangential"].default is False
    sig = inspect.signature(R.Mesh.set_edges)
    assert list(sig.parameters) == ["self", "latEdge", "lonEdge", "angleEdge"] and sig.parameters["angleEdge"].default is None
    assert R.MESHLOC_EDGE == 2
    for name in ("MESHLOC_EDGE", "mesh_edge_rotang", "wind_to_edges", "wind_to_edges_autograd"):
        assert name in R.__all__
    assert list(inspect.signature(tg.edge_rotang_at).parameters) == ["proj", "lon_deg", "angle_edge"]
    assert list(inspect.signature(synth.mesh_edges).parameters) == ["m"]


def _fortran_interface(src, name):
    m = re.search(r"function\s+%s\s*\(([^)]*)\)\s*&?\s*bind\s*\(\s*C\s*,\s*name\s*=\s*['\"]%s['\"]\s*\)(.*?)end\s+function" % (name, name),
                  src, flags=re.S | re.I)
    assert m, name + " has no bind(C) interface in mpg_mod.F90"
    return [a.strip().lower() for a in m.group(1).replace("&", " ").split(",")], m.group(2).lower()


def test_fortran_binds_them():
    src = open(os.path.join(ROOT, "mpassit_amd", "fortran", "mpg_mod.F90")).read()
    assert re.search(r"MPG_MESHLOC_EDGE\s*=\s*2", src)
    args, body = _fortran_interface(src, WIND)
    assert args == ["rh_u", "rh_v", "cn_dev", "sn_dev", "u_dev", "v_dev", "src_type", "u_level_stride", "v_level_stride", "nlev", "un_dev",
                    "ut_dev", "dst_type", "dst_layout", "hip_stream"]
    for a in ("src_type", "nlev", "dst_type", "dst_layout"):
        assert re.search(r"integer\(c_int\),\s*value\s*::.*\b%s\b" % a, body), a
    for a in ("u_level_stride", "v_level_stride"):
        assert re.search(r"integer\(c_int64_t\),\s*value\s*::.*\b%s\b" % a, body), a
    for a in ("rh_u", "rh_v", "cn_dev", "sn_dev", "u_dev", "v_dev", "un_dev", "ut_dev", "hip_stream"):
        assert re.search(r"type\(c_ptr\),\s*value\s*::.*\b%s\b" % a, body), a
    args, body = _fortran_interface(src, ROTANG)
    assert args == ["grid", "mesh", "cn_dev", "sn_dev", "hip_stream"]
    for a in args:
        assert re.search(r"type\(c_ptr\),\s*value\s*::.*\b%s\b" % a, body), a
    args, body = _fortran_interface(src, SET)
    assert args == ["mesh", "nedges", "latedge", "lonedge", "angleedge"]
    assert re.search(r"integer\(c_int64_t\),\s*value\s*::.*\bnedges\b", body)
    for a in ("mesh", "latedge", "lonedge", "angleedge"):
        assert re.search(r"type\(c_ptr\),\s*value\s*::.*\b%s\b" % a, body), a
    args, body = _fortran_interface(src, COUNT)
    assert args == ["mesh", "nedges"] and re.search(r"integer\(c_int64_t\),\s*intent\(out\)\s*::.*\bnedges\b", body)
    # the driver and interp_mod do not use them: the reference's job takes no wind back to the mesh
    for f in ("interp_mod.F90", "mpassit_driver.F90"):
        txt = open(os.path.join(ROOT, "mpassit_amd", "fortran", f)).read()
        for name in ARGS:
            assert name not in txt
