"""CPU checks of the periodic Grid -> Mesh boundary: the header declares mpg_regrid_store_periodic_to_mesh and the pole method enum and
states the rule, _lib lists and binds the call, the built library exports it, regrid.py has the agreed wrapper, the Fortran module has a
matching bind(C) interface, and the old call's comment names the new one."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORE = "mpg_regrid_store_periodic_to_mesh"
STORE_ARGS = ["mpg_grid src", "mpg_mesh dst", "int dst_meshloc", "int pole_method", "mpg_handle *out"]


def _header(strip_comments=True):
    txt = open(os.path.join(ROOT, "include", "mpassit_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S) if strip_comments else txt


def _doc(name, start):
    txt = _header(strip_comments=False)
    i = txt.index("int " + name + "(")
    doc = " ".join(txt[max(0, i - 9000):i].split())
    return doc[doc.rindex(start):]


def test_header_declares_the_call_and_the_enum():
    txt = _header()
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % STORE, txt)
    assert m, STORE + " is not declared"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == STORE_ARGS
    assert re.search(r"enum\s*\{\s*MPG_POLEMETHOD_NONE\s*=\s*0\s*,\s*MPG_POLEMETHOD_ALLAVG\s*=\s*1\s*\}\s*;", txt)


def test_header_states_the_rule():
    doc = _doc(STORE, "Periodic Grid -> Mesh: ESMF_FieldRegridStore")
    for phrase in ("MPG_GRID_PERIODIC_I", "j * nx + i", "(a + 1) mod nx", "quad id = b * nx + a", "lowest quad id", "grid_inside_tol_exp",
                   "the bits mpg_regrid_store_to_mesh produces", "only when no quad passed", "MPG_POLEMETHOD_ALLAVG", "MPG_POLEMETHOD_NONE",
                   "0 .. nx - 1 for the row-0 end", "nx .. 2 nx - 1 for the row-(ny - 1) end", "the lowest passing id wins",
                   "sign of the mean z of that end's CENTER row", "(A, B, N) at the north pole", "(B, A, S) at the south pole", "numbered north to south",
                   "in the same hemisphere are refused", "wr = t_pole / nx", "t_A + wr",
                   "MPG_GRID_NO_SOUTH_POLE", "MPG_GRID_NO_NORTH_POLE", "an empty row", "NPNTAVG", "TEETH", "EDGE / CORNER columns",
                   "nnz_per_row 0", "mpg_handle_pole_count gives 0", "no dst fraction", "exactly 4 entries, zeros included", "exactly nx",
                   "columns ascend within a row", "No atomic decides a stored byte", "store_boxes", "mpg_handle_store_path",
                   "MPG_ERR_INVALID_ARG", "nx < 3 or ny < 2", "MPG_ERR_UNSUPPORTED", "mpg_mesh_create_window", "MPG_ERR_OVERFLOW", "nnz >= 2^31",
                   "mpg_mesh_set_source_window passes these handles by", "There is no _begin variant", "[3] points mapped by a cap",
                   "[4] points mapped by a seam quad", "mpg_regrid_csr_to_mesh_dev", "mpg_regrid_csr_rows_dev", "mpg_regrid_transpose_dev",
                   "mpg_handle_get_csr"):
        assert phrase in doc, phrase
    # the old call's comment keeps its refusal and names the new call
    old = _doc("mpg_regrid_store_to_mesh", "Grid -> Mesh: ESMF_FieldRegridStore")
    assert "MPG_GRID_PERIODIC_I" in old and STORE in old


def test_lib_lists_binds_and_exports_it():
    from mpassit_amd import _lib, build
    assert STORE in _lib.SYMBOLS
    assert (_lib.POLEMETHOD_NONE, _lib.POLEMETHOD_ALLAVG) == (0, 1) == (_lib.MPG_POLEMETHOD_NONE, _lib.MPG_POLEMETHOD_ALLAVG)
    build.build()
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    assert hasattr(lib, STORE) and re.search(r" T %s\b" % STORE, out)
    at = _lib._STORE_PERIODIC_TO_MESH_PROTO._argtypes_
    assert len(at) == 5 and _lib._STORE_PERIODIC_TO_MESH_PROTO._restype_ is C.c_int and at[2] is C.c_int and at[3] is C.c_int
    assert callable(_lib.regrid_store_periodic_to_mesh)


def test_python_signature():
    from mpassit_amd import regrid as R
    sig = inspect.signature(R.regrid_store_periodic_to_mesh)
    assert list(sig.parameters) == ["src_grid", "dst_mesh", "meshloc", "pole_method"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["meshloc"], d["pole_method"]) == (R.MESHLOC_ELEMENT, R.POLEMETHOD_ALLAVG)
    assert (R.POLEMETHOD_NONE, R.POLEMETHOD_ALLAVG) == (0, 1)
    for name in ("regrid_store_periodic_to_mesh", "POLEMETHOD_NONE", "POLEMETHOD_ALLAVG"):
        assert name in R.__all__


def test_fortran_binds_it():
    src = open(os.path.join(ROOT, "mpassit_amd", "fortran", "mpg_mod.F90")).read()
    m = re.search(r"function\s+%s\s*\(([^)]*)\)\s*&?\s*bind\s*\(\s*C\s*,\s*name\s*=\s*['\"]%s['\"]\s*\)(.*?)end\s+function" % (STORE, STORE),
                  src, flags=re.S | re.I)
    assert m, STORE + " has no bind(C) interface in mpg_mod.F90"
    args, body = [a.strip().lower() for a in m.group(1).replace("&", " ").split(",")], m.group(2).lower()
    assert args == ["src", "dst", "dst_meshloc", "pole_method", "rh"]
    for a in ("dst_meshloc", "pole_method"):
        assert re.search(r"integer\(c_int\),\s*value\s*::.*\b%s\b" % a, body), a
    for a in ("src", "dst"):
        assert re.search(r"type\(c_ptr\),\s*value\s*::.*\b%s\b" % a, body), a
    assert re.search(r"type\(c_ptr\),\s*intent\(out\)\s*::\s*rh\b", body)
    assert src.index("mpg_regrid_store_to_mesh") < m.start() < src.index("function mpg_regrid_store_conserve_mesh"), "beside the other Grid -> Mesh Stores"
