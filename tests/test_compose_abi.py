"""CPU checks of the two calls of handle composition: the header declares mpg_handle_compose and mpg_compose_weights_dev with the agreed
argument lists, between mpg_wind_reconstruct_dev and the output epilogues, and states the shape, the pattern, the value rule and the
refusals; _lib lists and binds the two, the built library exports them, the kernel file and the checks header are part of the build, the
Python wrappers and the numpy mirror have the agreed signatures, and the Fortran module has matching bind(C) interfaces (which the driver
does not use)."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPOSE, WEIGHTS = "mpg_handle_compose", "mpg_compose_weights_dev"
ARGS = {
    COMPOSE: ["mpg_handle outer", "mpg_handle inner", "mpg_handle *out"],
    WEIGHTS: ["mpg_handle composed", "mpg_handle outer", "mpg_handle inner", "int nplanes", "const double *inner_m_dev", "double *m_dev",
              "void *hip_stream"],
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
    full = _header(strip_comments=False)
    at = [full.index("int " + n + "(") for n in (COMPOSE, WEIGHTS)]
    assert full.index("int mpg_wind_reconstruct_dev(") < at[0] < at[1] < full.index("---- output epilogues")
    assert at[1] < full.index("int mpg_dev_alloc(")


def test_header_states_the_contract():
    doc = _doc(COMPOSE, "---- handle composition")
    for phrase in ("C = A . B", "an ordinary CSR handle", "mpg_regrid_typed_dev", "mpg_regrid_csr_to_mesh_dev", "mpg_regrid_csr_rows_dev",
                   "mpg_regrid_masked_dev", "mpg_regrid_transpose_dev", "mpg_wind_vector_weights_dev", "mpg_wind_reconstruct_dev",
                   "mpg_handle_get_csr",
                   # the shape
                   "n_dst_B == n_src_A", "n_src = n_src_B", "n_dst, nx_dst and ny_dst are those of outer", "Always a CSR handle", "method -1",
                   "not cached", "mpg_handle_release", "longest row", "owns its arrays", "released right after the call",
                   "No destination fraction", "blocking", "reads the entry count back", "mpg_handle_store_ms",
                   "orders itself after whatever produced the two handles",
                   # the operands and the pattern
                   "fixed (3, 4 or 1 slots per row) or CSR", "idx = -1 is skipped", "weight 1.0", "distinct source ids",
                   "col_B[q] == e", "ascending order", "structural", "comes out 0.0 stays", "empty or unmapped", "only empty rows of B",
                   # the values
                   "contract by identity", "numpy mirror", "target_grid.compose_csr", "starts from 0.0", "in stored order",
                   "acc = acc + (a_p * b_q)", "rounded separately", "fp contract(off)", "Duplicate columns", "each occurrence is one term",
                   "same bytes from run to run", "no floating-point atomics", "compose_block_rows", "rows of any length",
                   "fixed byte budget", "2^31 - 2 pairs",
                   # the refusals
                   "MPG_ERR_INVALID_ARG", "NULL outer, inner or out", "both numbers are printed", "localized or rebased outer",
                   "MPG_ERR_UNSUPPORTED", "mpg_handle_pole_count > 0", "MPG_ERR_OVERFLOW", "more than 2^31 - 2 entries", "rowptr is int32",
                   "64-bit quantity", "leaks nothing",
                   # the planes
                   "caller-owned value planes", "mpg_reconstruct_weights_dev", "[nplanes][nnz_B]", "[nplanes][nnz_C]", "b_q = inner_m[k][q]",
                   "nplanes in 1..4", "neither allocates nor synchronises", "hipGraph", "Memory-safe", "contributes nothing",
                   "exactly composed's values", "mpg_compose_weights", "a fixed inner", "mpg_handle_get_weights", "mpg_handle_from_weights",
                   "a fixed composed", "nplanes outside 1..4", "composed.n_dst != outer.n_dst", "composed.n_src != inner.n_src",
                   "inner.n_dst != outer.n_src", "m_dev aliasing inner_m_dev"):
        assert phrase in doc, phrase
    assert "mpg_handle_compose" in _doc("mpg_tune", '"compose_block_rows"')      # the knob is listed with mpg_tune's keys


def test_lib_lists_binds_and_exports_them():
    from mpassit_amd import _lib, build
    for name in ARGS:
        assert name in _lib.SYMBOLS
    assert "k_compose.hip" in build.SOURCES and "compose_checks.h" in build.HEADERS
    assert os.path.exists(os.path.join(build.CSRC, "k_compose.hip")) and os.path.exists(os.path.join(build.CSRC, "compose_checks.h"))
    build.build()
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    for name in ARGS:
        assert hasattr(lib, name)
        assert re.search(r" T %s\b" % name, out)
    at = _lib._HANDLE_COMPOSE_PROTO._argtypes_
    assert list(at) == [C.c_void_p, C.c_void_p, C.c_void_p] and _lib._HANDLE_COMPOSE_PROTO._restype_ is C.c_int
    at = _lib._COMPOSE_WEIGHTS_PROTO._argtypes_
    assert list(at) == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert _lib._COMPOSE_WEIGHTS_PROTO._restype_ is C.c_int
    assert callable(_lib.handle_compose) and callable(_lib.compose_weights_dev)
    # the warm-up anchor, the knob, the kernel file's promises
    api = open(os.path.join(build.CSRC, "mpg_api.hip")).read()
    assert re.search(r"X\(k_compose\)", api)
    assert '"compose_block_rows"' in open(os.path.join(build.CSRC, "k_apply.hip")).read()
    kern = open(os.path.join(build.CSRC, "k_compose.hip")).read()
    assert "mpg_anchor_k_compose" in kern and "fp contract(off)" in kern
    assert "mpg_sort_pairs_u64_i32" in kern and "mpg_scan_excl_i32" in kern
    code = re.sub(r"//[^\n]*", "", kern)
    assert not re.search(r"atomic(Add|Exch|CAS)\s*\(", code) and "__shared__" not in code     # (one integer atomicMax: the longest row)
    checks = open(os.path.join(build.CSRC, "compose_checks.h")).read()
    assert re.search(r"#define\s+CO_LDS_ROW_ENTRIES\s+\d+", checks) and "hip/hip_runtime.h" not in checks


def test_python_signatures():
    from mpassit_amd import regrid as R, target_grid as tg
    assert list(inspect.signature(R.compose).parameters) == ["outer", "inner"]
    assert list(inspect.signature(R.compose_weights).parameters) == ["composed", "outer", "inner", "m_inner"]
    for name in ("compose", "compose_weights"):
        assert name in R.__all__
    assert list(inspect.signature(tg.compose_csr).parameters) == ["a_rowptr", "a_col", "a_val", "b_rowptr", "b_col", "b_vals"]
    sig = inspect.signature(tg.fixed_to_csr)
    assert list(sig.parameters) == ["idx", "w"] and sig.parameters["w"].default is None


def _fortran_interface(src, name):
    m = re.search(r"function\s+%s\s*\(([^)]*)\)\s*&?\s*bind\s*\(\s*C\s*,\s*name\s*=\s*['\"]%s['\"]\s*\)(.*?)end\s+function" % (name, name),
                  src, flags=re.S | re.I)
    assert m, name + " has no bind(C) interface in mpg_mod.F90"
    return [a.strip().lower() for a in m.group(1).replace("&", " ").split(",")], m.group(2).lower(), m.start()


def test_fortran_binds_them():
    src = open(os.path.join(ROOT, "mpassit_amd", "fortran", "mpg_mod.F90")).read()
    ints = {COMPOSE: [], WEIGHTS: ["nplanes"]}
    byref = {COMPOSE: ["out"], WEIGHTS: []}
    beside = re.search(r"end\s+function\s+mpg_wind_reconstruct_dev", src).end()
    for name, decl in ARGS.items():
        names = [a.split()[-1].lstrip("*").lower() for a in decl]
        args, body, at = _fortran_interface(src, name)
        assert args == names
        for a in ints[name]:
            assert re.search(r"integer\(c_int\),\s*value\s*::.*\b%s\b" % a, body), a
        for a in byref[name]:
            assert re.search(r"type\(c_ptr\),\s*intent\(out\)\s*::.*\b%s\b" % a, body), a
        for a in [x for x in names if x not in ints[name] + byref[name]]:
            assert re.search(r"type\(c_ptr\),\s*value\s*::.*\b%s\b" % a, body), a
        assert beside < at < src.index("function mpg_dev_alloc"), "after mpg_wind_reconstruct_dev, before mpg_dev_alloc"
    for f in ("interp_mod.F90", "mpassit_driver.F90"):
        txt = open(os.path.join(ROOT, "mpassit_amd", "fortran", f)).read()
        for name in ARGS:
            assert name not in txt
