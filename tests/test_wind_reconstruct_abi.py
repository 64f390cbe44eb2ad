"""CPU checks of the three calls of the wind reconstruction from edge-normal u: the header declares mpg_reconstruct_store,
mpg_reconstruct_weights_dev and mpg_wind_reconstruct_dev with the agreed argument lists, between mpg_wind_vector_dev and the output
epilogues, and states the pattern, the values and the value rule; _lib lists and binds the three, the built library exports them, the
kernel file and the checks header are part of the build, the Python wrappers have the agreed signatures, and the Fortran module has
matching bind(C) interfaces (which the driver does not use)."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORE, WEIGHTS, APPLY = "mpg_reconstruct_store", "mpg_reconstruct_weights_dev", "mpg_wind_reconstruct_dev"
ARGS = {
    STORE: ["int64_t nCells", "int64_t nEdges", "int maxEdges", "const int32_t *nEdgesOnCell_host", "const int32_t *edgesOnCell_host",
            "mpg_handle *out"],
    WEIGHTS: ["mpg_handle rh", "int maxEdges", "const double *coeffs_dev", "const double *dst_frames_dev", "double *m_dev", "void *hip_stream"],
    APPLY: ["mpg_handle rh", "const double *m_dev", "int nout", "const void *u_dev", "int src_type", "int src_layout", "int64_t u_level_stride",
            "int nlev", "void *r0_dev", "void *r1_dev", "void *r2_dev", "int dst_type", "int dst_layout", "void *hip_stream"],
}


def _header(strip_comments=True):
    txt = open(os.path.join(ROOT, "include", "mpassit_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S) if strip_comments else txt


def _doc(name, start):
    txt = _header(strip_comments=False)
    i = txt.index("int " + name + "(")
    doc = " ".join(txt[max(0, i - 9000):i].replace("\n *", "\n").split())
    return doc[doc.rindex(start):]


def test_header_declares_the_three_calls():
    txt = _header()
    for name, want in ARGS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, name + " is not declared"
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want
    assert len(ARGS[APPLY]) == 14
    full = _header(strip_comments=False)
    at = [full.index("int " + n + "(") for n in (STORE, WEIGHTS, APPLY)]
    assert full.index("int mpg_wind_vector_dev(") < at[0] < at[1] < at[2] < full.index("---- output epilogues")
    assert at[2] < full.index("int mpg_dev_alloc(")


def test_header_states_the_contract():
    doc = _doc(STORE, "Winds FROM the edge-normal u")
    for phrase in ("mpas_reconstruct", "V(k, c) = sum_i coeffs_reconstruct(:, i, c) * u(k, edgesOnCell(i, c))", "uReconstructZonal / uReconstructMeridional",
                   "hipGraph", "atomics",
                   # the Store
                   "n_src = nEdges, n_dst = nx_dst = nCells, ny_dst = 1", "1-based", "slot order", "summation order", "every value is 1.0",
                   "empty row", "duplicate edge ids", "mpg_handle_from_weights", "mpg_handle_get_csr", "mpg_regrid_transpose_dev", "Not cached",
                   "mpg_handle_release", "longest row", "the offending cell", "a count outside [0, maxEdges]", "an id outside [1, nEdges]",
                   # the values
                   "[nCells][maxEdges][3]", "padding included", "[6][nCells]", "mpg_sphere_frames_dev", "[nout][nnz]", "nout = 2 with frames, 3 without",
                   "The same bits as numpy", "fp contract(off)", "slot i = q - rowptr[c]",
                   "m0 = val[q] * ((cx*D0.x + cy*D0.y) + cz*D0.z)", "m_k = val[q] * c_k", "mpg_mesh_rotang_dev", "uReconstructX / Y / Z",
                   "writes nothing", "exceeds maxEdges", "no device read-back",
                   # the apply
                   "r2_dev is non-NULL exactly when nout == 3", "nout == 1 is refused", "mpg_regrid_csr_to_mesh_dev / mpg_regrid_csr_rows_dev",
                   "u[nEdges][nlev]", "u_level_stride must be 0", "0 = dense", "[lev][cell]", "[cell][lev]", "fully overwritten",
                   "acc_k = fma(m_k[q], (double)u[col[q]], acc_k)", "in stored order", "whatever LDS chunk", "store (TD) fma(acc_k, 1.0, 0.0)",
                   "one rounding to the destination type", "(TD)(+0.0)", "bit for bit mpg_regrid_csr_to_mesh_dev of a from-weights handle",
                   "scale 1 and offset 0", "all four layout pairs", "dense and pitched sources", "from call to call",
                   # refusals
                   "MPG_ERR_UNSUPPORTED", "mpg_handle_pole_count > 0", "MPG_TYPE_BE", "mpg_bswap_dev", "MPG_ERR_INVALID_ARG", "nlev < 1",
                   "a level stride below n_src", "aliasing", "MPG_ERR_OVERFLOW", "64-row blocks"):
        assert phrase in doc, phrase


def test_lib_lists_binds_and_exports_them():
    from mpassit_amd import _lib, build
    for name in ARGS:
        assert name in _lib.SYMBOLS
    assert "k_wind_reconstruct.hip" in build.SOURCES and "wind_reconstruct_checks.h" in build.HEADERS
    assert os.path.exists(os.path.join(build.CSRC, "k_wind_reconstruct.hip")) and os.path.exists(os.path.join(build.CSRC, "wind_reconstruct_checks.h"))
    build.build()
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    for name in ARGS:
        assert hasattr(lib, name)
        assert re.search(r" T %s\b" % name, out)
    at = _lib._RECONSTRUCT_STORE_PROTO._argtypes_
    assert list(at) == [C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] and _lib._RECONSTRUCT_STORE_PROTO._restype_ is C.c_int
    at = _lib._RECONSTRUCT_WEIGHTS_PROTO._argtypes_
    assert list(at) == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] and _lib._RECONSTRUCT_WEIGHTS_PROTO._restype_ is C.c_int
    at = _lib._WIND_RECONSTRUCT_PROTO._argtypes_
    assert len(at) == 14 and _lib._WIND_RECONSTRUCT_PROTO._restype_ is C.c_int
    assert at[6] is C.c_int64, "the level stride is 64-bit"
    assert [at[i] for i in (2, 4, 5, 7, 11, 12)] == [C.c_int] * 6
    assert all(at[i] is C.c_void_p for i in (0, 1, 3, 8, 9, 10, 13))
    assert callable(_lib.reconstruct_store) and callable(_lib.reconstruct_weights_dev) and callable(_lib.wind_reconstruct_dev)
    # the warm-up anchor
    api = open(os.path.join(build.CSRC, "mpg_api.hip")).read()
    assert re.search(r"X\(k_wind_reconstruct\)", api)
    kern = open(os.path.join(build.CSRC, "k_wind_reconstruct.hip")).read()
    assert "mpg_anchor_k_wind_reconstruct" in kern and "fp contract(off)" in kern and "mpg_dispatch_types" in kern


def test_python_signatures():
    from mpassit_amd import regrid as R, synth, target_grid as tg
    assert list(inspect.signature(R.reconstruct_store).parameters) == ["nEdgesOnCell", "edgesOnCell", "nEdges"]
    sig = inspect.signature(R.reconstruct_weights)
    assert list(sig.parameters) == ["rh", "coeffs", "dst_frames"] and sig.parameters["dst_frames"].default is None
    sig = inspect.signature(R.wind_reconstruct)
    assert list(sig.parameters) == ["rh", "m", "u", "nlev", "src_layout", "layout", "out_dtype", "outs"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["src_layout"], d["layout"], d["out_dtype"], d["outs"]) == (R.LAYOUT_LEV_FAST, R.LAYOUT_CELL_FAST, None, None)
    assert d["nlev"] is inspect.Parameter.empty
    sig = inspect.signature(R.wind_reconstruct_autograd)
    assert list(sig.parameters) == ["rh", "m", "u", "nlev", "src_layout", "layout"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["src_layout"], d["layout"]) == (R.LAYOUT_LEV_FAST, R.LAYOUT_CELL_FAST)
    for name in ("reconstruct_store", "reconstruct_weights", "wind_reconstruct", "wind_reconstruct_autograd"):
        assert name in R.__all__
    assert list(inspect.signature(tg.reconstruct_blocks).parameters) == ["rowptr", "coeffs", "val", "dst_frames"]
    assert list(inspect.signature(synth.edges_on_cell).parameters) == ["m"]
    assert list(inspect.signature(synth.reconstruct_coeffs).parameters) == ["m", "nEdgesOnCell", "edgesOnCell"]


def _fortran_interface(src, name):
    m = re.search(r"function\s+%s\s*\(([^)]*)\)\s*&?\s*bind\s*\(\s*C\s*,\s*name\s*=\s*['\"]%s['\"]\s*\)(.*?)end\s+function" % (name, name),
                  src, flags=re.S | re.I)
    assert m, name + " has no bind(C) interface in mpg_mod.F90"
    return [a.strip().lower() for a in m.group(1).replace("&", " ").split(",")], m.group(2).lower(), m.start()


def test_fortran_binds_them():
    src = open(os.path.join(ROOT, "mpassit_amd", "fortran", "mpg_mod.F90")).read()
    ints = {STORE: ["maxedges"], WEIGHTS: ["maxedges"], APPLY: ["nout", "src_type", "src_layout", "nlev", "dst_type", "dst_layout"]}
    int64s = {STORE: ["ncells", "nedges"], WEIGHTS: [], APPLY: ["u_level_stride"]}
    byref = {STORE: ["out"], WEIGHTS: [], APPLY: []}
    beside = re.search(r"end\s+function\s+mpg_wind_vector_dev", src).end()
    for name, decl in ARGS.items():
        names = [a.split()[-1].lstrip("*").lower() for a in decl]
        args, body, at = _fortran_interface(src, name)
        assert args == names
        for a in ints[name]:
            assert re.search(r"integer\(c_int\),\s*value\s*::.*\b%s\b" % a, body), a
        for a in int64s[name]:
            assert re.search(r"integer\(c_int64_t\),\s*value\s*::.*\b%s\b" % a, body), a
        for a in byref[name]:
            assert re.search(r"type\(c_ptr\),\s*intent\(out\)\s*::.*\b%s\b" % a, body), a
        for a in [x for x in names if x not in ints[name] + int64s[name] + byref[name]]:
            assert re.search(r"type\(c_ptr\),\s*value\s*::.*\b%s\b" % a, body), a
        assert beside < at < src.index("function mpg_dev_alloc"), "after mpg_wind_vector_dev, before mpg_dev_alloc"
    for f in ("interp_mod.F90", "mpassit_driver.F90"):
        txt = open(os.path.join(ROOT, "mpassit_amd", "fortran", f)).read()
        for name in ARGS:
            assert name not in txt
