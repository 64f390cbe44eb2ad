"""CPU checks of the conservative Mesh -> Mesh boundary: the header declares mpg_regrid_store_conserve_mesh and mpg_regrid_csr_rows_dev
with their exact argument lists and states the rules, _lib lists and binds both, the built library exports them, the Python wrappers
have the agreed signatures and refuse bad arguments before any device call, the Fortran module has matching bind(C) interfaces, the new
sources are built and anchored -- and the phrases the older boundary tests rely on are still where they look for them."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORE, APPLY = "mpg_regrid_store_conserve_mesh", "mpg_regrid_csr_rows_dev"
STORE_ARGS = ["mpg_mesh src", "mpg_mesh dst", "int norm_type", "mpg_handle *out"]
APPLY_ARGS = ["mpg_handle rh", "const void *src_dev", "int src_type", "int nlev", "int nfields", "void *dst_dev", "int dst_type", "double scale",
              "double offset", "void *hip_stream"]


def _header(strip_comments=True):
    txt = open(os.path.join(ROOT, "include", "mpassit_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S) if strip_comments else txt


def _doc(name, start):
    txt = _header(strip_comments=False)
    i = txt.index("int " + name + "(")
    doc = " ".join(re.sub(r"\n \*(?!/)", " ", txt[max(0, i - 9000):i]).split())   # (the comment's line leaders dropped: a phrase may wrap)
    return doc[doc.rindex(start):]


def test_header_declares_both_calls_after_the_rows_apply():
    txt = _header()
    for name, want in ((STORE, STORE_ARGS), (APPLY, APPLY_ARGS)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, name + " is not declared"
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want
        assert m.start() > txt.index("int mpg_regrid_rows_dev(")
    # one block: the two declarations follow each other
    assert re.search(r"int\s+%s\s*\([^)]*\)\s*;\s*int\s+%s\s*\(" % (STORE, APPLY), txt)


def test_header_states_the_rules():
    doc = _doc(STORE, "Conservative Mesh -> Mesh: ESMF_FieldRegridStore")
    for phrase in ("verticesOnCell", "great-circle sides", "subject polygon", "sign of its own fan area", "sides in listed order",
                   "a x (b - a)", "1e-15 * |n|", "|b - a|^2 < 1e-24", "clamped at 0", "no floating-point contraction",
                   "MPG_NORM_DSTAREA: w = I / area(d)", "MPG_NORM_FRACAREA: w = I / sum_s I", "I <= 1e-14 * area(d)", "empty row",
                   "ascending s", "mpg_handle_get_dst_frac", "nnz_per_row 0", "ny_dst = 1", "the same bytes", "no atomic decides a stored byte",
                   "no pair with I > 0 is removed", "mpg_mesh_create_window", "maxEdges > 12", "MPG_ERR_OVERFLOW", "MPG_ERR_INVALID_ARG",
                   "unknown norm_type", "src == dst is allowed", "256 * norm_type", "mpg_mesh_set_source_window on the SOURCE mesh",
                   "EITHER mesh is destroyed", "There is no _begin variant", "[1] pairs clipped", "[3] microseconds", "[6] vertex slots",
                   "mpg_regrid_csr_rows_dev"):
        assert phrase in doc, phrase
    doc = _doc(APPLY, "mpg_regrid_csr_rows_dev: the CSR Regrid of rows onto rows")
    for phrase in ("[n_src][nlev]", "[n_dst][nlev]", "ANY CSR handle without pole caps", "mpg_handle_from_weights",
                   "MPG_ERR_UNSUPPORTED: a fixed handle (mpg_regrid_rows_dev serves those); MPG_TYPE_BE", "nlev < 1", "nfields < 1",
                   "Contract by identity, no tolerance", "fma(val[q], src[col[q] * nlev + k], acc)", "stored order",
                   "element [p][k] has the bits of element [k][p]", "MPG_LAYOUT_LEV_FAST", "(dst type) fma(0.0, scale, offset)", "nfields batching",
                   "No atomics", "allocates nothing and synchronises nothing", "hipGraph from the first call"):
        assert phrase in doc, phrase


def test_older_phrases_are_still_in_place():
    """The refusing calls keep their words and name the new calls; the new block stays out of the older tests' comment searches."""
    txt = " ".join(_header(strip_comments=False).split())
    old = _doc("mpg_regrid_store_mesh", "Mesh -> Mesh: ESMF_FieldRegridStore")
    assert "MPG_ERR_UNSUPPORTED: MPG_REGRIDMETHOD_CONSERVE" in old and "Voronoi cell against Voronoi cell" in old and STORE in old
    old = _doc("mpg_regrid_rows_dev", "Regrid from rows to rows")
    assert "MPG_ERR_UNSUPPORTED: MPG_TYPE_BE; CSR handles" in old and APPLY in old
    assert "Store of its own, with its normalisation argument: mpg_regrid_store_conserve_to_mesh" in txt
    assert "CSR handles are served by mpg_regrid_csr_to_mesh_dev" in txt
    for start in ("Grid -> Mesh: ESMF_FieldRegridStore", "Regrid onto a mesh", "Transpose Regrid", "Conservative Store onto a mesh",
                  "CSR Regrid in mesh order", "Regrid from rows to rows"):
        assert start not in _doc(STORE, "Conservative Mesh -> Mesh: ESMF_FieldRegridStore"), start
    api = open(os.path.join(ROOT, "mpassit_amd", "csrc", "mpg_api.hip")).read()
    refusal = " ".join(api[api.index("int mpg_regrid_store_mesh("):api.index("int mpg_handle_get_dst_frac(")].split())
    for phrase in ("Voronoi cell against Voronoi cell is not built", "mpg_regrid_store_conserve_to_mesh", STORE):
        assert phrase in refusal.replace('" "', ""), phrase
    frac = " ".join(api[api.index("int mpg_handle_get_dst_frac("):api.index("int mpg_handle_release(")].split()).replace('" "', "")
    assert "the handle has no destination fraction (mpg_regrid_store_conserve_to_mesh stores one" in frac and STORE in frac


def test_lib_lists_binds_and_exports_them():
    from mpassit_amd import _lib, build
    assert STORE in _lib.SYMBOLS and APPLY in _lib.SYMBOLS
    build.build()
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    for name in (STORE, APPLY):
        assert hasattr(lib, name)
        assert re.search(r" T %s\b" % name, out)
    at = _lib._STORE_CONSERVE_MESH_PROTO._argtypes_
    assert len(at) == 4 and at[2] is C.c_int and _lib._STORE_CONSERVE_MESH_PROTO._restype_ is C.c_int
    at = _lib._CSR_ROWS_PROTO._argtypes_
    assert len(at) == 10 and _lib._CSR_ROWS_PROTO._restype_ is C.c_int
    assert at[3] is C.c_int and at[7] is C.c_double and at[8] is C.c_double and at[9] is C.c_void_p
    assert callable(_lib.regrid_store_conserve_mesh) and callable(_lib.regrid_csr_rows_dev)


def test_python_signatures():
    from mpassit_amd import regrid as R
    sig = inspect.signature(R.regrid_store_conserve_mesh)
    assert list(sig.parameters) == ["src_mesh", "dst_mesh", "norm"] and sig.parameters["norm"].default == R.NORM_DSTAREA
    sig = inspect.signature(R.RouteHandle.regrid_csr_rows)
    assert list(sig.parameters) == ["self", "src", "nlev", "nfields", "out_dtype", "scale", "offset", "out"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["nlev"], d["nfields"], d["out_dtype"], d["scale"], d["offset"], d["out"]) == (1, 1, None, 1.0, 0.0, None)
    sig = inspect.signature(R.regrid_csr_rows_autograd)
    assert list(sig.parameters) == ["rh", "src", "nlev", "nfields"]
    assert (sig.parameters["nlev"].default, sig.parameters["nfields"].default) == (1, 1)
    assert "regrid_store_conserve_mesh" in R.__all__ and "regrid_csr_rows_autograd" in R.__all__


def test_wrappers_reject_bad_arguments_before_any_device_call():
    """No GPU, no mpg_init: every one of these must fail in Python, with a message of its own (a call that reached the library would
    raise MpgError 'mpg_init has not been called')."""
    import torch
    from mpassit_amd import regrid as R

    class NotAMesh:
        _h = None

    fake = R.Mesh.__new__(R.Mesh)             # a Mesh object without a device mesh behind it
    fake._h = C.c_void_p()
    with pytest.raises(TypeError, match="Mesh objects"):
        R.regrid_store_conserve_mesh(NotAMesh(), fake)
    with pytest.raises(TypeError, match="Mesh objects"):
        R.regrid_store_conserve_mesh(fake, None)
    for bad in (2, -1, None):
        with pytest.raises(ValueError, match="norm"):
            R.regrid_store_conserve_mesh(fake, fake, norm=bad)
    rh = R.RouteHandle.__new__(R.RouteHandle)  # a handle's bookkeeping without a device handle behind it
    rh._h, rh.n_src, rh.n_dst, rh.nx_dst, rh.ny_dst, rh.nnz_per_row = C.c_void_p(), 10, 7, 7, 1, 0
    with pytest.raises(ValueError, match="CUDA tensor"):
        rh.regrid_csr_rows(np.zeros((10, 2)), nlev=2)
    with pytest.raises(ValueError, match="CUDA tensor"):
        rh.regrid_csr_rows(torch.zeros((10, 2), dtype=torch.float64), nlev=2)


def test_fortran_binds_them():
    src = open(os.path.join(ROOT, "mpassit_amd", "fortran", "mpg_mod.F90")).read()

    def interface(name):
        m = re.search(r"function\s+%s\s*\(([^)]*)\)\s*&?\s*bind\s*\(\s*C\s*,\s*name\s*=\s*['\"]%s['\"]\s*\)(.*?)end\s+function" % (name, name),
                      src, flags=re.S | re.I)
        assert m, name + " has no bind(C) interface in mpg_mod.F90"
        return [a.strip().lower() for a in m.group(1).replace("&", " ").split(",")], m.group(2).lower()

    args, body = interface(STORE)
    assert args == ["src", "dst", "norm_type", "rh"]
    assert re.search(r"integer\(c_int\),\s*value\s*::.*\bnorm_type\b", body)
    for a in ("src", "dst"):
        assert re.search(r"type\(c_ptr\),\s*value\s*::.*\b%s\b" % a, body), a
    assert re.search(r"type\(c_ptr\),\s*intent\(out\)\s*::\s*rh\b", body)
    args, body = interface(APPLY)
    assert args == ["rh", "src_dev", "src_type", "nlev", "nfields", "dst_dev", "dst_type", "scale", "offset", "hip_stream"]
    for a in ("src_type", "nlev", "nfields", "dst_type"):
        assert re.search(r"integer\(c_int\),\s*value\s*::.*\b%s\b" % a, body), a
    assert re.search(r"real\(c_double\),\s*value\s*::.*\bscale\b.*\boffset\b", body)
    for a in ("rh", "src_dev", "dst_dev", "hip_stream"):
        assert re.search(r"type\(c_ptr\),\s*value\s*::.*\b%s\b" % a, body), a


def test_kernel_sources_are_built_and_anchored():
    from mpassit_amd import build
    assert "k_store_conserve_mesh.hip" in build.SOURCES and "k_apply_csr_rows.hip" in build.SOURCES and "conserve_clip.h" in build.HEADERS
    csrc = os.path.join(ROOT, "mpassit_amd", "csrc")
    api = open(os.path.join(csrc, "mpg_api.hip")).read()
    assert "X(k_store_conserve_mesh)" in api and "X(k_apply_csr_rows)" in api
    store = open(os.path.join(csrc, "k_store_conserve_mesh.hip")).read()
    assert "#pragma clang fp contract(off)" in store, "geometry translation units are compiled without floating-point contraction"
    assert store.index("#pragma clang fp contract(off)") < store.index('#include "conserve_clip.h"')
    # the clip step and the cell area live in ONE place, used by both conservative translation units
    shared = open(os.path.join(csrc, "conserve_clip.h")).read()
    old = open(os.path.join(csrc, "k_store_conserve.hip")).read()
    for name in ("struct LdsPoly", "int clip_halfspace_lds(", "double cell_fan_area("):
        assert name in shared and name not in old and name not in store, name
    assert '#include "conserve_clip.h"' in old
    rows = open(os.path.join(csrc, "k_apply_csr_rows.hip")).read()
    assert "atomic" not in rows.split("#include")[-1], "the CSR rows Regrid uses no atomics"
    assert '#include "apply_mesh.h"' in rows and "apply_mesh.h" in build.HEADERS
    helpers = open(os.path.join(csrc, "apply_mesh.h")).read()
    assert "atomic" not in helpers.split("#include")[-1], "nor do the helpers it shares with the other mesh-order kernels"
    assert "xcd_remap" in rows and "stream_store_lane" in rows and "int64_t" in rows
