"""CPU checks of the adjoint of the masked Regrid: the header declares mpg_regrid_masked_transpose_dev with the agreed 14 arguments
directly after mpg_regrid_masked_dev and states the contract; _lib lists and binds it, the built library exports it, the kernel file is
part of the build with its warm-up anchor and without contraction, the segment sum is still one text, the Python wrappers have the agreed
signatures, and the Fortran module has a matching bind(C) interface (which the driver does not use)."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, FORWARD = "mpg_regrid_masked_transpose_dev", "mpg_regrid_masked_dev"
ARGS = ["mpg_handle rh", "const void *g_dev", "int g_type", "int64_t g_level_stride", "const void *src_dev", "int src_type", "int src_layout",
        "int nlev", "int nfields", "void *dst_dev", "int dst_type", "const mpg_mask_opts *opts", "double *work_dev", "void *hip_stream"]


def _header(strip_comments=True):
    txt = open(os.path.join(ROOT, "include", "mpassit_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S) if strip_comments else txt


def test_header_declares_the_call():
    txt = _header()
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, txt)
    assert m, NAME + " is not declared"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == ARGS
    assert len(ARGS) == 14, "test_null_args_gpu.py calls every export with 14 zeros"
    # directly after the forward: no other declaration in between
    between = txt[txt.index("int " + FORWARD + "("):txt.index("int " + NAME + "(")]
    assert between.count(";") == 1


def test_header_states_the_contract():
    txt = _header(strip_comments=False)
    i = txt.index("int " + NAME + "(")
    doc = " ".join(txt[max(0, i - 9000):i].replace("\n *", "\n").split())
    doc = doc[doc.rindex("The adjoint of the masked Regrid"):]
    for phrase in ("[nfields][nlev][plane of n_dst]", "0 = dense", "below n_dst -> MPG_ERR_INVALID_ARG", "The pad is never read",
                   "read only to decide validity", "never enter a product", "fully overwritten", "MPG_TYPE_F64 or MPG_TYPE_F32 on each of g, src and dst",
                   "one rounding at the store", "fill_value and offset are ignored", "float64 workspace of nfields * nlev * n_dst elements",
                   "its contents on return are part of the contract", "must not alias g_dev, src_dev or dst_dev",
                   "Contract by identity, no tolerance", "nothing is contracted", "word for word", "same order, same expressions",
                   "Wv > 0 && Wv >= min_valid_frac * Wt is bit-exact",
                   "defined(p, k) ? ((double)g[k][p] * scale) * (Wt / Wv) : +0.0", "two separately rounded products", "a select, never a product with 0",
                   "reaches no source", "fma(w_j, h[k][row_j], acc) from +0.0", "ascending (destination point, slot) order",
                   "the chain of mpg_regrid_transpose_dev", "w_j = 1.0", "src_mask[c] == 0 and src(c, k) not missing under flags",
                   "ok(c, k) ? (dst type) acc : +0.0", "a source no entry references gets +0.0",
                   "Identity with the unmasked transpose", "Wt / Wv == 1.0", "h equals (double)g bit for bit",
                   "equals mpg_regrid_transpose_dev into the same type and layout bit for bit",
                   "derivative of the forward with respect to every valid source element", "exactly +0.0 at every invalid one",
                   "scale included", "not an inverse", "No floating-point atomics", "across nfields batching", "the two layouts",
                   "float32 / float64 inputs that hold the same values",
                   "MPG_ERR_UNSUPPORTED for MPG_TYPE_BE on any side and for handles with pole caps", "NULL rh, opts, g_dev, src_dev, dst_dev or work_dev",
                   "nlev or nfields < 1", "outside [0, 1] or NaN", "MPG_MISSING_VALUE with a NaN missing_value", "unknown flag bits",
                   "A refused call writes nothing", "the first call on a handle builds its transposed index", "hipGraph"):
        assert phrase in doc, phrase


def test_lib_lists_binds_and_exports_it():
    from mpassit_amd import _lib, build
    assert NAME in _lib.SYMBOLS
    assert "k_transpose_masked.hip" in build.SOURCES and "masked_par.h" in build.HEADERS and "transpose_seg.h" in build.HEADERS
    for f in ("k_transpose_masked.hip", "masked_par.h"):
        assert os.path.exists(os.path.join(build.CSRC, f))
    build.build()
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    assert hasattr(lib, NAME) and re.search(r" T %s\b" % NAME, out)
    at = _lib._REGRID_MASKED_TRANSPOSE_PROTO._argtypes_
    assert len(at) == 14 and _lib._REGRID_MASKED_TRANSPOSE_PROTO._restype_ is C.c_int
    assert at[3] is C.c_int64, "the level stride is 64-bit"
    assert all(at[i] is C.c_int for i in (2, 5, 6, 7, 8, 10)) and all(at[i] is C.c_void_p for i in (0, 1, 4, 9, 12, 13))
    assert at[11] is C.POINTER(_lib.MaskOpts)
    assert callable(_lib.regrid_masked_transpose_dev)
    # the warm-up anchor; no contraction anywhere in the file; MaskPar / mk_missing and the segment sum are one text each
    api = open(os.path.join(build.CSRC, "mpg_api.hip")).read()
    assert re.search(r"X\(k_transpose_masked\)", api)
    assert re.search(r"\bint mpg_k_transpose_masked\(", open(os.path.join(build.CSRC, "mpg_internal.h")).read())
    kern = open(os.path.join(build.CSRC, "k_transpose_masked.hip")).read()
    assert "mpg_anchor_k_transpose_masked" in kern and '#include "transpose_seg.h"' in kern and '#include "masked_par.h"' in kern
    assert kern.index("#pragma clang fp contract(off)") < kern.index("__device__"), "the pragma covers the whole file"
    for k in ("k_mratio_cf", "k_mratio_lf", "k_mratio_csr", "k_trm_short_cf", "k_trm_short_lf", "k_trm_long", "mpg_k_transpose_build"):
        assert k in kern, k
    assert "atomic" not in re.sub(r"//.*", "", kern)
    fwd = open(os.path.join(build.CSRC, "k_apply_masked.hip")).read()
    par = open(os.path.join(build.CSRC, "masked_par.h")).read()
    assert '#include "masked_par.h"' in fwd
    for pat in (r"struct MaskPar\s*\{", r"__device__ __forceinline__ bool mk_missing\("):
        assert len(re.findall(pat, par)) == 1 and not re.search(pat, fwd + kern), pat + " is defined once, in the header"
    seg = open(os.path.join(build.CSRC, "transpose_seg.h")).read()
    old = open(os.path.join(build.CSRC, "k_transpose.hip")).read()
    wind = open(os.path.join(build.CSRC, "k_wind_transpose.hip")).read()
    for fn in ("tr_load_seg", "tr_seg_regs", "tr_seg_mem"):
        assert len(re.findall(r"__device__ __forceinline__ \w+ %s\(" % fn, seg)) == 1, fn
        assert not re.search(r"__device__ __forceinline__ \w+ %s\(" % fn, old + wind + kern), fn + " is defined once, in the header"


def test_python_signatures():
    from mpassit_amd import regrid as R
    sig = inspect.signature(R.RouteHandle.regrid_masked_transpose)
    assert list(sig.parameters) == ["self", "grad", "src", "nlev", "nfields", "layout", "missing", "src_mask", "min_valid_frac", "scale", "out_dtype",
                                    "out", "work"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["nlev"], d["nfields"], d["layout"], d["missing"], d["src_mask"], d["min_valid_frac"], d["scale"], d["out_dtype"], d["out"], d["work"]) == (
        1, 1, R.LAYOUT_CELL_FAST, "nan", None, 0.5, 1.0, None, None, None)
    assert d["grad"] is inspect.Parameter.empty and d["src"] is inspect.Parameter.empty
    sig = inspect.signature(R.regrid_masked_autograd)
    assert list(sig.parameters) == ["rh", "src", "nlev", "nfields", "layout", "missing", "src_mask", "min_valid_frac", "fill_value"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["nlev"], d["nfields"], d["layout"], d["missing"], d["src_mask"], d["min_valid_frac"]) == (1, 1, R.LAYOUT_CELL_FAST, "nan", None, 0.5)
    assert d["fill_value"] != d["fill_value"], "fill_value defaults to NaN"
    assert "regrid_masked_autograd" in R.__all__
    doc = " ".join(R.regrid_masked_autograd.__doc__.split())
    assert "is 0, not NaN" in doc and "is ignored" in doc
    # regrid_masked keeps its signature, and both calls parse `missing` with one helper
    assert list(inspect.signature(R.RouteHandle.regrid_masked).parameters) == [
        "self", "src", "nlev", "nfields", "layout", "missing", "src_mask", "min_valid_frac", "fill_value", "out_dtype", "scale", "offset", "out"]
    for fn in (R.RouteHandle.regrid_masked, R.RouteHandle.regrid_masked_transpose):
        assert "_parse_missing(" in inspect.getsource(fn)


def test_fortran_binds_it():
    src = open(os.path.join(ROOT, "mpassit_amd", "fortran", "mpg_mod.F90")).read()
    m = re.search(r"function\s+%s\s*\(([^)]*)\)\s*&?\s*bind\s*\(\s*C\s*,\s*name\s*=\s*['\"]%s['\"]\s*\)(.*?)end\s+function" % (NAME, NAME),
                  src, flags=re.S | re.I)
    assert m, NAME + " has no bind(C) interface in mpg_mod.F90"
    args, body = [a.strip().lower() for a in m.group(1).replace("&", " ").split(",")], m.group(2).lower()
    names = [a.split()[-1].lstrip("*") for a in ARGS]
    assert args == names
    ints, int64s, structs = ["g_type", "src_type", "src_layout", "nlev", "nfields", "dst_type"], ["g_level_stride"], ["opts"]
    for a in ints:
        assert re.search(r"integer\(c_int\),\s*value\s*::.*\b%s\b" % a, body), a
    for a in int64s:
        assert re.search(r"integer\(c_int64_t\),\s*value\s*::.*\b%s\b" % a, body), a
    assert re.search(r"type\(mpg_mask_opts\),\s*intent\(in\)\s*::\s*opts\b", body), "opts goes by reference, as in the forward's interface"
    for a in [x for x in names if x not in ints + int64s + structs]:
        assert re.search(r"type\(c_ptr\),\s*value\s*::.*\b%s\b" % a, body), a
    assert re.search(r"end\s+function\s+%s\b" % FORWARD, src).end() < m.start(), "beside mpg_regrid_masked_dev"
    gap = src[re.search(r"end\s+function\s+%s\b" % FORWARD, src).end():m.start()]
    assert "function" not in re.sub(r"!.*", "", gap), "directly beside it"
    for f in ("interp_mod.F90", "mpassit_driver.F90"):
        assert NAME not in open(os.path.join(ROOT, "mpassit_amd", "fortran", f)).read()
