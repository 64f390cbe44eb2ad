"""CPU checks of the transpose Regrid's boundary: the header declares mpg_regrid_transpose_dev / mpg_handle_transpose_stats with
their documented signatures, _lib binds them, and the Fortran module has matching bind(C) interfaces."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpg_regrid_transpose_dev", "mpg_handle_transpose_stats", "mpg_handle_transpose_build_ms")


def _decl(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpassit_amd.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, name + " is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_signatures():
    assert _decl("mpg_regrid_transpose_dev") == [
        "mpg_handle rh", "const void *src_dev", "int src_type", "int64_t src_level_stride", "int nlev", "int nfields",
        "void *dst_dev", "int dst_type", "int dst_layout", "void *hip_stream"]
    assert _decl("mpg_handle_transpose_stats") == ["mpg_handle rh", "int64_t *n_referenced", "int64_t *max_per_source"]
    assert _decl("mpg_handle_transpose_build_ms") == ["mpg_handle rh", "float *ms"]


def test_lib_binds_them():
    from mpassit_amd import _lib, build
    for n in NAMES:
        assert n in _lib.SYMBOLS
    build.build()
    lib = _lib.load()
    for n in NAMES:
        assert hasattr(lib, n)


def test_header_says_adjoint_not_inverse():
    txt = open(os.path.join(ROOT, "include", "mpassit_amd.h")).read()
    i = txt.index("int mpg_regrid_transpose_dev")
    assert "ADJOINT" in txt[i - 3000:i] and "not an inverse" in txt[i - 3000:i]


def _fortran_interface(name):
    src = open(os.path.join(ROOT, "mpassit_amd", "fortran", "mpg_mod.F90")).read()
    m = re.search(r"function\s+%s\s*\(([^)]*)\)\s*&?\s*bind\s*\(\s*C\s*,\s*name\s*=\s*['\"]%s['\"]\s*\)(.*?)end\s+function" % (name, name),
                  src, flags=re.S | re.I)
    assert m, name + " has no bind(C) interface in mpg_mod.F90"
    return [a.strip().lower() for a in m.group(1).replace("&", " ").split(",")], m.group(2).lower()


def test_fortran_interfaces_match():
    args, body = _fortran_interface("mpg_regrid_transpose_dev")
    assert len(args) == 10
    for a in ("src_type", "nlev", "nfields", "dst_type", "dst_layout"):
        assert re.search(r"integer\(c_int\),\s*value\s*::.*\b%s\b" % a, body), a
    assert re.search(r"integer\(c_int64_t\),\s*value\s*::.*\bsrc_level_stride\b", body)
    for a in ("rh", "src_dev", "dst_dev", "hip_stream"):
        assert re.search(r"type\(c_ptr\),\s*value\s*::.*\b%s\b" % a, body), a
    args, body = _fortran_interface("mpg_handle_transpose_stats")
    assert len(args) == 3
    assert re.search(r"integer\(c_int64_t\)\s*::.*\bn_referenced\b", body) and re.search(r"integer\(c_int64_t\)\s*::.*\bmax_per_source\b", body)
