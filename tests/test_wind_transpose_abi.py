"""CPU checks of the adjoint of the wind chain: the header declares mpg_rotate_winds_transpose_dev and mpg_wind_destagger_transpose_dev
with the agreed argument lists, directly after mpg_wind_destagger and before "The wind chain turned round", and states the contract;
_lib lists and binds the two, the built library exports them, the kernel file is part of the build with its warm-up anchor, the Python
wrappers have the agreed signatures, and the Fortran module has matching bind(C) interfaces (which the driver does not use)."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROTATE, FUSED = "mpg_rotate_winds_transpose_dev", "mpg_wind_destagger_transpose_dev"
ARGS = {
    ROTATE: ["int64_t npts", "int nlev", "const double *cosa_dev", "const double *sina_dev", "double *gu_dev", "double *gv_dev", "void *hip_stream"],
    FUSED: ["mpg_handle rh_edge1", "mpg_handle rh_edge2", "const double *cosa_dev", "const double *sina_dev", "const void *gu_dev",
            "const void *gv_dev", "int src_type", "int64_t src_level_stride", "int nlev", "const double *gumass_rot_dev",
            "const double *gvmass_rot_dev", "double *gumass_dev", "double *gvmass_dev", "void *hip_stream"],
}


def _header(strip_comments=True):
    txt = open(os.path.join(ROOT, "include", "mpassit_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S) if strip_comments else txt


def _doc(name, start):
    txt = _header(strip_comments=False)
    i = txt.index("int " + name + "(")
    doc = " ".join(txt[max(0, i - 9000):i].replace("\n *", "\n").split())
    return doc[doc.rindex(start):]


def test_header_declares_the_two_calls():
    txt = _header()
    for name, want in ARGS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, name + " is not declared"
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want
    assert len(ARGS[FUSED]) == 14, "test_null_args_gpu.py calls every export with 14 zeros"
    full = _header(strip_comments=False)
    at = [full.index("int " + n + "(") for n in (ROTATE, FUSED)]
    assert full.index("int mpg_wind_destagger(") < at[0] < at[1] < full.index("The wind chain turned round") < full.index("int mpg_wind_to_mesh_dev(")
    # directly after: no other declaration in between
    between = _header()[_header().index("int mpg_wind_destagger("):_header().index("int " + ROTATE + "(")]
    assert between.count(";") == 1


def test_header_states_the_contract():
    doc = _doc(ROTATE, "The ADJOINT of the wind chain")
    for phrase in ("in place", "[nlev][npts]", "contract by identity", "reverse mode of interp.F90:737-748", "tana = sa / ca", "den = ca + sa * tana",
                   "a = gvn / ca", "t = a * sa", "b = gun - t", "guo = b / den", "p = guo * tana", "gvo = a + p", "rounded once",
                   "nothing contracted", "ca == +-0.0", "IEEE 754", "bit for bit"):
        assert phrase in doc, phrase
    doc = _doc(FUSED, "The adjoint of mpg_wind_destagger_dev")
    for phrase in ("ONE pass", "CENTER -> EDGE1 / CENTER -> EDGE2 pair of one grid", "same test as mpg_wind_destagger_dev", "MPG_ERR_UNSUPPORTED",
                   "[nlev][ny][nx+1]", "[nlev][ny+1][nx]", "MPG_TYPE_F64 or MPG_TYPE_F32", "0 = dense", "ONE stride for both", "at least the larger plane",
                   "mpg_wind_destagger_pitched_dev", "its pad is never read", "dense, fully overwritten",
                   "mpg_regrid_transpose_dev contract", "ascending (destination point, slot)", "fma chain from +0.0", "+0.0 for a source no entry references",
                   "never read", "one add; no add when the pointer is NULL", "gumass = s1 iff rh_edge1 is given", "gvmass = s2 iff rh_edge2 is given",
                   "pole term of the transpose contract is added last",
                   "MPG_ERR_INVALID_ARG", "both handles NULL", "cosa without sina", "a rotation without both handles", "without a rotation", "nlev < 1",
                   "a stride below the larger plane", "an output pointer equal to an input pointer", "a NULL array that is needed",
                   "MPG_TYPE_BE", "a rotation together with pole caps", "4 GiB or more",
                   "two mpg_regrid_transpose_dev calls into float64, then the optional adds, then mpg_rotate_winds_transpose_dev",
                   "across float32 / float64 inputs that hold the same values", "No floating-point atomics",
                   "the first call on a handle builds its transposed index", "hipGraph"):
        assert phrase in doc, phrase


def test_lib_lists_binds_and_exports_them():
    from mpassit_amd import _lib, build
    for name in ARGS:
        assert name in _lib.SYMBOLS
    assert "k_wind_transpose.hip" in build.SOURCES and "k_transpose.hip" in build.SOURCES and "transpose_seg.h" in build.HEADERS
    assert os.path.exists(os.path.join(build.CSRC, "k_wind_transpose.hip")) and os.path.exists(os.path.join(build.CSRC, "transpose_seg.h"))
    build.build()
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    for name in ARGS:
        assert hasattr(lib, name)
        assert re.search(r" T %s\b" % name, out)
    at = _lib._ROTATE_WINDS_TRANSPOSE_PROTO._argtypes_
    assert len(at) == 7 and at[0] is C.c_int64 and at[1] is C.c_int and all(a is C.c_void_p for a in at[2:])
    assert _lib._ROTATE_WINDS_TRANSPOSE_PROTO._restype_ is C.c_int
    at = _lib._WIND_DESTAGGER_TRANSPOSE_PROTO._argtypes_
    assert len(at) == 14 and _lib._WIND_DESTAGGER_TRANSPOSE_PROTO._restype_ is C.c_int
    assert at[7] is C.c_int64, "the level stride is 64-bit"
    assert at[6] is C.c_int and at[8] is C.c_int
    assert all(at[i] is C.c_void_p for i in (0, 1, 2, 3, 4, 5, 9, 10, 11, 12, 13))
    assert callable(_lib.rotate_winds_transpose_dev) and callable(_lib.wind_destagger_transpose_dev)
    # the warm-up anchor; the kernel is compiled without contraction; the segment sum is one text for both transposes
    api = open(os.path.join(build.CSRC, "mpg_api.hip")).read()
    assert re.search(r"X\(k_wind_transpose\)", api)
    kern = open(os.path.join(build.CSRC, "k_wind_transpose.hip")).read()
    assert "mpg_anchor_k_wind_transpose" in kern and "#pragma clang fp contract(off)" in kern and '#include "transpose_seg.h"' in kern
    old = open(os.path.join(build.CSRC, "k_transpose.hip")).read()
    assert '#include "transpose_seg.h"' in old
    seg = open(os.path.join(build.CSRC, "transpose_seg.h")).read()
    for fn in ("tr_load_seg", "tr_seg_regs", "tr_seg_mem"):
        assert re.search(r"__device__ __forceinline__ \w+ %s\(" % fn, seg), fn
        assert not re.search(r"__device__ __forceinline__ \w+ %s\(" % fn, old + kern), fn + " is defined once, in the header"
    assert "k_rotate_t" in open(os.path.join(build.CSRC, "k_apply.hip")).read()


def test_python_signatures():
    from mpassit_amd import regrid as R, target_grid as tg
    assert list(inspect.signature(R.rotate_winds_cgrid_transpose).parameters) == ["cosa", "sina", "gu", "gv"]
    sig = inspect.signature(R.wind_destagger_transpose)
    assert list(sig.parameters) == ["rh_u", "rh_v", "cosa", "sina", "gu", "gv", "nlev", "g_umass_rot", "g_vmass_rot", "outs"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["g_umass_rot"], d["g_vmass_rot"], d["outs"]) == (None, None, None) and d["nlev"] is inspect.Parameter.empty
    sig = inspect.signature(R.wind_destagger_autograd)
    assert list(sig.parameters) == ["rh_u", "rh_v", "cosa", "sina", "umass", "vmass", "nlev", "out_dtype", "keep_mass"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["out_dtype"], d["keep_mass"]) == (None, False)
    for name in ("rotate_winds_cgrid_transpose", "wind_destagger_transpose", "wind_destagger_autograd"):
        assert name in R.__all__
    assert list(inspect.signature(tg.rotate_winds_transpose_at).parameters) == ["cosa", "sina", "gu", "gv"]


def _fortran_interface(src, name):
    m = re.search(r"function\s+%s\s*\(([^)]*)\)\s*&?\s*bind\s*\(\s*C\s*,\s*name\s*=\s*['\"]%s['\"]\s*\)(.*?)end\s+function" % (name, name),
                  src, flags=re.S | re.I)
    assert m, name + " has no bind(C) interface in mpg_mod.F90"
    return [a.strip().lower() for a in m.group(1).replace("&", " ").split(",")], m.group(2).lower(), m.start()


def test_fortran_binds_them():
    src = open(os.path.join(ROOT, "mpassit_amd", "fortran", "mpg_mod.F90")).read()
    ints = {ROTATE: ["nlev"], FUSED: ["src_type", "nlev"]}
    int64s = {ROTATE: ["npts"], FUSED: ["src_level_stride"]}
    beside = re.search(r"end\s+function\s+mpg_wind_destagger\b", src).end()
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
        assert beside < at < src.index("function mpg_wind_to_mesh_dev"), "beside mpg_wind_destagger"
    for f in ("interp_mod.F90", "mpassit_driver.F90"):
        txt = open(os.path.join(ROOT, "mpassit_amd", "fortran", f)).read()
        for name in ARGS:
            assert name not in txt
