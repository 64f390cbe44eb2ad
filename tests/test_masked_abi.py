"""CPU checks of the masked Regrid's boundary: the header declares mpg_regrid_masked_dev, mpg_mask_opts and the two flags and states
the contract, _lib lists and binds the symbol, the built library exports it, and the Fortran module has a matching bind(C) type and
interface."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mpg_regrid_masked_dev"


def _header(strip_comments=True):
    txt = open(os.path.join(ROOT, "include", "mpassit_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S) if strip_comments else txt


def test_header_declares_call_struct_and_flags():
    txt = _header()
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, txt)
    assert m, NAME + " is not declared"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == [
        "mpg_handle rh", "const void *src_dev", "int src_type", "int src_layout", "int nlev", "int nfields", "void *dst_dev", "int dst_type",
        "int64_t dst_level_stride", "const mpg_mask_opts *opts", "void *hip_stream"]
    s = re.search(r"typedef\s+struct\s+mpg_mask_opts\s*\{(.*?)\}\s*mpg_mask_opts\s*;", txt, flags=re.S)
    assert s, "mpg_mask_opts is not declared"
    fields = [" ".join(f.split()) for f in s.group(1).split(";") if f.strip()]
    assert fields == ["int flags", "double missing_value", "const uint8_t *src_mask_dev", "double min_valid_frac", "double fill_value",
                      "double scale, offset"]
    assert re.search(r"enum\s*\{\s*MPG_MISSING_NAN\s*=\s*1\s*,\s*MPG_MISSING_VALUE\s*=\s*2\s*\}", txt)


def test_header_states_the_contract():
    txt = _header(strip_comments=False)
    i = txt.index("int " + NAME)
    doc = " ".join(txt[i - 6000:i].split())
    doc = doc[doc.rindex("Masked Regrid"):]
    assert "Bit identity with the unmasked Regrid when nothing is missing" in doc
    assert "fill_value for unmapped points" in doc
    assert re.search(r"MPG_ERR_UNSUPPORTED: MPG_TYPE_BE on either side, and handles with pole caps", doc)
    for word in ("Wt", "Wv", "min_valid_frac", "src_mask_dev", "hipGraph", "No atomics"):
        assert word in doc, word


def test_lib_lists_binds_and_exports_it():
    from mpassit_amd import _lib, build
    assert NAME in _lib.SYMBOLS
    build.build()
    lib = _lib.load()
    assert hasattr(lib, NAME)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T %s\b" % NAME, out)
    # the ctypes mirror of the struct has the C layout: int, pad, double, pointer, 4 doubles
    assert C.sizeof(_lib.MaskOpts) == 56
    assert [f[0] for f in _lib.MaskOpts._fields_] == ["flags", "missing_value", "src_mask_dev", "min_valid_frac", "fill_value", "scale", "offset"]
    assert _lib.MaskOpts.missing_value.offset == 8 and _lib.MaskOpts.src_mask_dev.offset == 16 and _lib.MaskOpts.offset.offset == 48
    assert (_lib.MISSING_NAN, _lib.MISSING_VALUE) == (1, 2)
    assert len(_lib._MASKED_PROTO._argtypes_) == 11 and _lib._MASKED_PROTO._restype_ is C.c_int


def test_python_method_signature():
    import inspect
    from mpassit_amd import regrid as R
    sig = inspect.signature(R.RouteHandle.regrid_masked)
    assert list(sig.parameters) == ["self", "src", "nlev", "nfields", "layout", "missing", "src_mask", "min_valid_frac", "fill_value",
                                    "out_dtype", "scale", "offset", "out"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["missing"] == "nan" and d["min_valid_frac"] == 0.5 and d["fill_value"] != d["fill_value"] and d["src_mask"] is None
    assert d["scale"] == 1.0 and d["offset"] == 0.0 and d["layout"] == R.LAYOUT_CELL_FAST


def test_fortran_binds_it():
    src = open(os.path.join(ROOT, "mpassit_amd", "fortran", "mpg_mod.F90")).read()
    m = re.search(r"function\s+%s\s*\(([^)]*)\)\s*&?\s*bind\s*\(\s*C\s*,\s*name\s*=\s*['\"]%s['\"]\s*\)(.*?)end\s+function" % (NAME, NAME),
                  src, flags=re.S | re.I)
    assert m, NAME + " has no bind(C) interface in mpg_mod.F90"
    args, body = [a.strip().lower() for a in m.group(1).replace("&", " ").split(",")], m.group(2).lower()
    assert args == ["rh", "src_dev", "src_type", "src_layout", "nlev", "nfields", "dst_dev", "dst_type", "dst_level_stride", "opts", "hip_stream"]
    for a in ("src_type", "src_layout", "nlev", "nfields", "dst_type"):
        assert re.search(r"integer\(c_int\),\s*value\s*::.*\b%s\b" % a, body), a
    assert re.search(r"integer\(c_int64_t\),\s*value\s*::.*\bdst_level_stride\b", body)
    for a in ("rh", "src_dev", "dst_dev", "hip_stream"):
        assert re.search(r"type\(c_ptr\),\s*value\s*::.*\b%s\b" % a, body), a
    assert re.search(r"type\(mpg_mask_opts\)[^\n]*::\s*opts\b", body) and not re.search(r"type\(mpg_mask_opts\)\s*,\s*value", body)
    t = re.search(r"type\s*,\s*bind\s*\(\s*c\s*\)\s*::\s*mpg_mask_opts(.*?)end\s+type", src, flags=re.S | re.I)
    assert t, "mpg_mask_opts has no bind(C) type in mpg_mod.F90"
    names = re.findall(r"::\s*([a-z_, ]+?)\s*(?:!|\n)", t.group(1).lower())
    assert [n.strip() for n in names] == ["flags", "missing_value", "src_mask_dev", "min_valid_frac", "fill_value", "scale, offset"]
    # the driver and interp_mod do not use the masked call: the reference's job has no masked field
    for f in ("interp_mod.F90", "mpassit_driver.F90"):
        assert NAME not in open(os.path.join(ROOT, "mpassit_amd", "fortran", f)).read()
