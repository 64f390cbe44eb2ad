"""CPU checks of the conservative Grid -> Mesh boundary: the header declares mpg_regrid_store_conserve_to_mesh, mpg_handle_get_dst_frac
and mpg_regrid_csr_to_mesh_dev with their exact argument lists and states the rule, _lib lists and binds them, the built library
exports them, the Python wrappers have the agreed signatures and the Fortran module has matching bind(C) interfaces (which the
driver does not use)."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORE, FRAC, APPLY = "mpg_regrid_store_conserve_to_mesh", "mpg_handle_get_dst_frac", "mpg_regrid_csr_to_mesh_dev"
STORE_ARGS = ["mpg_grid src", "mpg_mesh dst", "int norm_type", "mpg_handle *out"]
FRAC_ARGS = ["mpg_handle rh", "double *frac_host"]
APPLY_ARGS = ["mpg_handle rh", "const void *src_dev", "int src_type", "int64_t src_level_stride", "int nlev", "int nfields", "void *dst_dev",
              "int dst_type", "int dst_layout", "double scale", "double offset", "void *hip_stream"]


def _header(strip_comments=True):
    txt = open(os.path.join(ROOT, "include", "mpassit_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S) if strip_comments else txt


def _doc(name, start):
    txt = _header(strip_comments=False)
    i = txt.index("int " + name + "(")
    doc = " ".join(txt[max(0, i - 9000):i].split())
    return doc[doc.rindex(start):]


def test_header_declares_the_calls_after_the_fixed_slot_apply():
    txt = _header()
    for name, want in ((STORE, STORE_ARGS), (FRAC, FRAC_ARGS), (APPLY, APPLY_ARGS)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, name + " is not declared"
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want
        assert m.start() > txt.index("int mpg_regrid_to_mesh_dev(")
    assert re.search(r"enum\s*\{\s*MPG_NORM_DSTAREA\s*=\s*0\s*,\s*MPG_NORM_FRACAREA\s*=\s*1\s*\}", txt)


def test_header_states_the_rule():
    doc = _doc(STORE, "Conservative Store onto a mesh")
    for phrase in ("MPG_NORM_DSTAREA", "w = I / area(c)", "MPG_NORM_FRACAREA", "w = I / sum_g I", "I <= 1e-14 * area(c)", "j * nx + i",
                   "ny_dst = 1", "verticesOnCell", "empty row", "ascending g", "mpg_handle_get_dst_frac", "B = D_c^-1 A^T D_g",
                   "columns ascending", "same bytes from run to run", "store_boxes", "MPG_GRID_PERIODIC_I", "mpg_mesh_create_window",
                   "maxEdges > 12", "MPG_ERR_OVERFLOW", "MPG_ERR_INVALID_ARG", "unknown norm_type", "There is no _begin variant",
                   "mpg_mesh_set_source_window", "mpg_regrid_masked_dev", "mpg_regrid_transpose_dev", "mpg_handle_get_csr"):
        assert phrase in doc, phrase
    doc = _doc(APPLY, "CSR Regrid in mesh order")
    for phrase in ("hipGraph", "MPG_LAYOUT_LEV_FAST [cell][lev]", "mpg_regrid_typed_dev", "MPG_TYPE_BE", "MPG_ERR_UNSUPPORTED: a fixed handle",
                   "mpg_regrid_to_mesh_dev serves those", "pole caps", "src_level_stride", "No atomics", "fma(val[q], src[col[q]], acc)",
                   "stored order", "empty row", "mpg_handle_from_weights", "Contract by identity, no tolerance",
                   "allocates nothing and synchronises nothing"):
        assert phrase in doc, phrase
    # the two refusing calls point here
    txt = " ".join(_header(strip_comments=False).split())
    assert "Store of its own, with its normalisation argument: mpg_regrid_store_conserve_to_mesh" in txt
    assert "CSR handles are served by mpg_regrid_csr_to_mesh_dev" in txt
    # ... and the new comments stay out of the way of the older tests' comment search
    for name in (STORE, APPLY):
        for start in ("Grid -> Mesh: ESMF_FieldRegridStore", "Regrid onto a mesh", "Transpose Regrid"):
            own = _doc(name, "Conservative Store onto a mesh" if name == STORE else "CSR Regrid in mesh order")
            assert start not in own, (name, start)


def test_lib_lists_binds_and_exports_them():
    from mpassit_amd import _lib, build
    for name in (STORE, FRAC, APPLY):
        assert name in _lib.SYMBOLS
    assert (_lib.MPG_NORM_DSTAREA, _lib.MPG_NORM_FRACAREA) == (0, 1)
    build.build()
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    for name in (STORE, FRAC, APPLY):
        assert hasattr(lib, name)
        assert re.search(r" T %s\b" % name, out)
    assert len(_lib._STORE_CONSERVE_TO_MESH_PROTO._argtypes_) == 4 and _lib._STORE_CONSERVE_TO_MESH_PROTO._restype_ is C.c_int
    assert _lib._STORE_CONSERVE_TO_MESH_PROTO._argtypes_[2] is C.c_int
    at = _lib._CSR_TO_MESH_PROTO._argtypes_
    assert len(at) == 12 and _lib._CSR_TO_MESH_PROTO._restype_ is C.c_int
    assert at[3] is C.c_int64 and at[9] is C.c_double and at[10] is C.c_double
    assert callable(_lib.regrid_store_conserve_to_mesh) and callable(_lib.regrid_csr_to_mesh_dev) and callable(_lib.handle_get_dst_frac)


def test_python_signatures():
    from mpassit_amd import regrid as R
    sig = inspect.signature(R.regrid_store_conserve_to_mesh)
    assert list(sig.parameters) == ["src_grid", "dst_mesh", "norm"]
    assert sig.parameters["norm"].default == R.NORM_DSTAREA == 0 and R.NORM_FRACAREA == 1
    sig = inspect.signature(R.RouteHandle.regrid_csr_to_mesh)
    assert list(sig.parameters) == ["self", "src", "nlev", "nfields", "layout", "out_dtype", "scale", "offset", "out"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["nlev"], d["nfields"], d["layout"], d["out_dtype"], d["scale"], d["offset"], d["out"]) == (1, 1, R.LAYOUT_CELL_FAST, None, 1.0, 0.0, None)
    assert list(inspect.signature(R.RouteHandle.dst_frac).parameters) == ["self"]
    sig = inspect.signature(R.regrid_csr_to_mesh_autograd)
    assert list(sig.parameters) == ["rh", "src", "nlev", "nfields", "layout"]
    assert sig.parameters["layout"].default == R.LAYOUT_CELL_FAST
    for name in ("regrid_store_conserve_to_mesh", "regrid_csr_to_mesh_autograd", "NORM_DSTAREA", "NORM_FRACAREA"):
        assert name in R.__all__


def _fortran_interface(src, name):
    m = re.search(r"function\s+%s\s*\(([^)]*)\)\s*&?\s*bind\s*\(\s*C\s*,\s*name\s*=\s*['\"]%s['\"]\s*\)(.*?)end\s+function" % (name, name),
                  src, flags=re.S | re.I)
    assert m, name + " has no bind(C) interface in mpg_mod.F90"
    return [a.strip().lower() for a in m.group(1).replace("&", " ").split(",")], m.group(2).lower()


def test_fortran_binds_them():
    src = open(os.path.join(ROOT, "mpassit_amd", "fortran", "mpg_mod.F90")).read()
    args, body = _fortran_interface(src, STORE)
    assert args == ["src", "dst", "norm_type", "rh"]
    assert re.search(r"integer\(c_int\),\s*value\s*::.*\bnorm_type\b", body)
    for a in ("src", "dst"):
        assert re.search(r"type\(c_ptr\),\s*value\s*::.*\b%s\b" % a, body), a
    assert re.search(r"type\(c_ptr\),\s*intent\(out\)\s*::\s*rh\b", body)
    args, body = _fortran_interface(src, FRAC)
    assert args == ["rh", "frac_host"]
    assert re.search(r"type\(c_ptr\),\s*value\s*::.*\brh\b", body) and re.search(r"real\(c_double\),\s*intent\(out\)\s*::\s*frac_host\(\*\)", body)
    args, body = _fortran_interface(src, APPLY)
    assert args == ["rh", "src_dev", "src_type", "src_level_stride", "nlev", "nfields", "dst_dev", "dst_type", "dst_layout", "scale", "offset",
                    "hip_stream"]
    for a in ("src_type", "nlev", "nfields", "dst_type", "dst_layout"):
        assert re.search(r"integer\(c_int\),\s*value\s*::.*\b%s\b" % a, body), a
    assert re.search(r"integer\(c_int64_t\),\s*value\s*::.*\bsrc_level_stride\b", body)
    assert re.search(r"real\(c_double\),\s*value\s*::.*\bscale\b.*\boffset\b", body)
    for a in ("rh", "src_dev", "dst_dev", "hip_stream"):
        assert re.search(r"type\(c_ptr\),\s*value\s*::.*\b%s\b" % a, body), a
    assert re.search(r"mpg_norm_dstarea\s*=\s*0\s*,\s*mpg_norm_fracarea\s*=\s*1", src.lower())
    for f in ("interp_mod.F90", "mpassit_driver.F90"):
        txt = open(os.path.join(ROOT, "mpassit_amd", "fortran", f)).read()
        assert STORE not in txt and APPLY not in txt and FRAC not in txt
