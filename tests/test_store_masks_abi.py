"""CPU checks of the Store-time mask calls: the header declares mpg_handle_mask and mpg_handle_extrapolate_masked with the agreed argument
lists, the struct and the enum -- in a section of their own behind mpg_handle_extrapolate and before the output epilogues -- and states
both contracts; _lib lists, binds and exports the two; the kernel file and the two HIP-free headers are part of the build and keep their
promises; the Python wrappers and the numpy mirrors have the agreed signatures; the Fortran module has matching bind(C) types and
interfaces (which the driver does not use)."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK, EXM = "mpg_handle_mask", "mpg_handle_extrapolate_masked"
ARGS = {
    MASK: ["mpg_handle rh", "const mpg_store_mask_opts *opts", "mpg_handle *out"],
    EXM: ["mpg_handle rh", "const mpg_points *src", "const mpg_points *dst", "const mpg_extrap_opts *opts", "const uint8_t *src_mask_dev",
          "const uint8_t *dst_skip_dev", "mpg_handle *out"],
}


def _header(strip_comments=True):
    txt = open(os.path.join(ROOT, "include", "mpassit_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S) if strip_comments else txt


def test_header_declares_the_calls_the_struct_and_the_enum():
    txt = _header()
    for name, want in ARGS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, name + " is not declared"
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want
        assert len(want) <= 14
    assert re.search(r"enum\s*\{\s*MPG_MASKRULE_AUTO\s*=\s*0\s*,\s*MPG_MASKRULE_ROW\s*=\s*1\s*,\s*MPG_MASKRULE_ENTRY\s*=\s*2\s*\}", txt)
    opts = re.search(r"typedef\s+struct\s+mpg_store_mask_opts\s*\{(.*?)\}\s*mpg_store_mask_opts\s*;", txt, flags=re.S).group(1)
    assert [" ".join(f.split()) for f in opts.split(";") if f.strip()] == ["const uint8_t *src_mask_dev", "const uint8_t *dst_mask_dev", "int rule", "int norm_type"]
    full = _header(strip_comments=False)
    sec = full.index("---- Store-time masks")
    assert full.index("int mpg_handle_extrapolate(") < sec < full.index("int " + MASK + "(") < full.index("int " + EXM + "(") < full.index("---- output epilogues")
    assert "---- extrapolation" not in full[sec:full.index("---- output epilogues")]


def test_header_states_both_contracts():
    txt = _header(strip_comments=False)
    a, b = txt.index("---- Store-time masks"), txt.index("int " + MASK + "(")
    doc = " ".join(txt[a:b].replace("\n *", "\n").split())
    for phrase in ("srcMaskValues / dstMaskValues", "an ordinary handle", "non-zero = masked", "It needs no geometry", "both NULL is success",
                   # the destination mask and the ROW rule
                   "masked destination row becomes unmapped", "under either rule", "MPG_MASKRULE_ROW", "a masked corner", "index >= 0, whatever its weight",
                   "copied verbatim", "Fixed and CSR handles", "cap rows", "rows like any other", "stays fixed", "same slot count",
                   "stays without a weight array", "every slot's index -1, every weight +0.0", "unmapped rows are empty",
                   # the ENTRY rule
                   "MPG_MASKRULE_ENTRY", "do not take part", "CSR handles only", "stored order", "left to right", "rounded on its own", "fp contract(off)",
                   "MPG_NORM_DSTAREA: the values are unchanged and frac' = Wk", "w' = w / Wk and frac' = frac * Wk", "Wk <= 0", "frac' = +0.0",
                   "no masked entry is copied verbatim", "bit for bit", "An input without dst_frac gives an output without one",
                   # AUTO
                   "MPG_MASKRULE_AUTO", "MPG_REGRIDMETHOD_BILINEAR or MPG_REGRIDMETHOD_NEAREST_STOD", "MPG_REGRIDMETHOD_CONSERVE", "from weights, composed, reconstruct",
                   "explicit rule",
                   # the output, determinism, blocking, refusals
                   "n_src, n_dst, nx_dst, ny_dst, method and kind", "not cached", "owns its arrays", "mpg_handle_release", "longest row", "mpg_handle_store_ms",
                   "mpg_handle_store_stats", "the source rule unmapped", "destination mask unmapped", "entries removed", "target_grid.mask_rows",
                   "same bytes from run to run", "no floating-point atomics", "drains the Store worker", "mpg_handle_get_csr", "names mpg_handle_mask",
                   "MPG_ERR_INVALID_ARG", "unknown rule", "unknown norm_type", "MPG_ERR_UNSUPPORTED", "mpg_handle_pole_count > 0", "localized or rebased",
                   "source window", "mpg_handle_get_weights -> mpg_handle_from_weights", "leaks nothing",
                   # the masked extrapolation
                   "word for word, with two changes", "src_mask[c] == 0", "K = min(N, number of unmasked sources)", "dst_skip[p] != 0", "left unmapped",
                   "lower UNMASKED id at every rank", "knn_weights", "with both NULL the output bytes equal mpg_handle_extrapolate's",
                   "every source masked nothing is filled", "[1] = rows filled, [2] = K, [3] = unmasked sources", "target_grid.extrapolate_rows_masked",
                   "never enters a subtree that holds no unmasked source", "`alive` byte per tree node", "bottom-up", "valid lower bounds", "the result is exact",
                   "under the name mpg_handle_extrapolate_masked",
                   # what is out
                   "Not served", "node-located sources", "creep fills"):
        assert phrase in doc, phrase
    # the dynamic masked Regrid points at the new calls
    i = txt.index("NOT ESMF's Store-time srcMaskValues")
    assert MASK in txt[i:i + 200] and EXM in txt[i:i + 200]


def test_lib_lists_binds_and_exports_them():
    from mpassit_amd import _lib, build
    for name in ARGS:
        assert name in _lib.SYMBOLS
    assert "k_handle_mask.hip" in build.SOURCES and "knn_mask.h" in build.HEADERS and "handle_mask.h" in build.HEADERS
    for f in ("k_handle_mask.hip", "knn_mask.h", "handle_mask.h"):
        assert os.path.exists(os.path.join(build.CSRC, f))
    build.build()
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    for name in ARGS:
        assert hasattr(lib, name)
        assert re.search(r" T %s\b" % name, out)
    assert [f[0] for f in _lib.StoreMaskOpts._fields_] == ["src_mask_dev", "dst_mask_dev", "rule", "norm_type"]
    assert [f[1] for f in _lib.StoreMaskOpts._fields_] == [C.c_void_p, C.c_void_p, C.c_int, C.c_int] and C.sizeof(_lib.StoreMaskOpts) == 24
    assert list(_lib._HANDLE_MASK_PROTO._argtypes_) == [C.c_void_p, C.POINTER(_lib.StoreMaskOpts), C.c_void_p] and _lib._HANDLE_MASK_PROTO._restype_ is C.c_int
    assert list(_lib._HANDLE_EXTRAPOLATE_MASKED_PROTO._argtypes_) == [C.c_void_p, C.POINTER(_lib.Points), C.POINTER(_lib.Points), C.POINTER(_lib.ExtrapOpts),
                                                                     C.c_void_p, C.c_void_p, C.c_void_p]
    assert _lib._HANDLE_EXTRAPOLATE_MASKED_PROTO._restype_ is C.c_int
    assert callable(_lib.handle_mask) and callable(_lib.handle_extrapolate_masked)
    assert (_lib.MASKRULE_AUTO, _lib.MASKRULE_ROW, _lib.MASKRULE_ENTRY) == (0, 1, 2)
    assert (_lib.MPG_MASKRULE_AUTO, _lib.MPG_MASKRULE_ROW, _lib.MPG_MASKRULE_ENTRY) == (0, 1, 2)


def test_kernel_files_keep_their_promises():
    from mpassit_amd import build
    api = open(os.path.join(build.CSRC, "mpg_api.hip")).read()
    assert re.search(r"X\(k_handle_mask\)", api)
    # the Store worker is drained on the way of both entry points
    a = api.index("int " + MASK + "(")
    assert "store_worker_drain();" in api[a:api.index("mpg_k_handle_mask(rh", a)]
    b = api.index("int " + EXM + "(")
    body = api[b:api.index("\n}\n", b)]
    assert 'ex_extrapolate("' + EXM + '"' in body
    shared = api.index("static int ex_extrapolate(", b)
    assert "store_worker_drain();" in api[shared:api.index("mpg_k_extrapolate(rh", shared)]
    kern = open(os.path.join(build.CSRC, "k_handle_mask.hip")).read()
    for word in ("mpg_anchor_k_handle_mask", "mpg_scan_excl_i32", "mpg_sum_i32_i64", "hm_entry_row", "handle_mask.h", "k_hm_flag", "k_hm_fill_fixed", "k_hm_fill_csr"):
        assert word in kern, word
    code = re.sub(r"//[^\n]*", "", kern)
    assert not re.search(r"atomic(Add|Exch|CAS)\s*\(", code) and "__shared__" not in code          # (one integer atomicMax: the longest row)
    ex = open(os.path.join(build.CSRC, "k_extrapolate.hip")).read()
    for word in ("knn_mask.h", "knn_search_masked", "k_ex_knn_masked<Src, 1>", "k_ex_knn_masked<Src, 2>", "k_ex_knn_masked<Src, 4>", "k_ex_knn_masked<Src, 8>",
                 "k_ex_alive_leaf", "k_ex_alive_up", "k_ex_flag_skip", "leaf_masked", "if (mask[c]) continue;"):
        assert word in ex, word
    for leaf in re.findall(r"void leaf_masked\(.*?\n  \}", ex, flags=re.S):
        assert leaf.index("mask[") < leaf.index("dist2_nofma"), "the mask is tested before a distance is computed"
    for name in ("knn_mask.h", "handle_mask.h"):
        h = open(os.path.join(build.CSRC, name)).read()
        assert "hip/hip_runtime.h" not in h and "TW_FN" in h and "__shared__" not in h
    km = open(os.path.join(build.CSRC, "knn_mask.h")).read()
    for word in ("struct AliveTree", "alive_parent", "alive_build_host", "alive_root", "return (c >= 0 && alive["):
        assert word in km, word
    hm = open(os.path.join(build.CSRC, "handle_mask.h")).read()
    assert "fp contract(off)" in hm and hm.count("hm_entry_row(") == 1, "one function holds the row's value rule"


def test_python_signatures():
    from mpassit_amd import regrid as R, target_grid as tg

    def sig(f):
        s = inspect.signature(f)
        return list(s.parameters), {k: v.default for k, v in s.parameters.items() if v.default is not inspect.Parameter.empty}

    names, d = sig(R.mask_handle)
    assert names == ["rh", "src_mask", "dst_mask", "rule", "norm_type"]
    assert d == {"src_mask": None, "dst_mask": None, "rule": R.MASKRULE_AUTO, "norm_type": R.NORM_DSTAREA}
    names, d = sig(R.extrapolate_masked)
    assert names == ["rh", "src", "dst", "src_mask", "dst_skip", "method", "num_src_pnts", "dist_exponent", "src_loc", "dst_loc"]
    assert d == {"src_mask": None, "dst_skip": None, "method": R.EXTRAPMETHOD_NEAREST_STOD, "num_src_pnts": 8, "dist_exponent": 2.0, "src_loc": None, "dst_loc": None}
    names, d = sig(R.store_masks)
    assert names == ["rh", "src", "dst", "src_mask", "dst_mask", "norm_type", "extrap_method", "num_src_pnts", "dist_exponent", "src_loc", "dst_loc"]
    assert d == {"src_mask": None, "dst_mask": None, "norm_type": R.NORM_DSTAREA, "extrap_method": None, "num_src_pnts": 8, "dist_exponent": 2.0,
                 "src_loc": None, "dst_loc": None}
    for name in ("mask_handle", "extrapolate_masked", "store_masks", "MASKRULE_AUTO", "MASKRULE_ROW", "MASKRULE_ENTRY"):
        assert name in R.__all__
    assert sig(tg.mask_rows)[0] == ["rowptr", "col", "val", "frac", "src_mask", "dst_mask", "rule", "norm_type"]
    assert sig(tg.extrapolate_rows_masked)[0] == ["src_xyz", "dst_xyz", "unmapped", "src_mask", "method", "num_src_pnts", "dist_exponent"]
    assert sig(tg.extrapolate_rows)[0] == ["src_xyz", "dst_xyz", "unmapped", "method", "num_src_pnts", "dist_exponent"], "extrapolate_rows keeps its signature"
    assert (tg.MASKRULE_ROW, tg.MASKRULE_ENTRY, tg.NORM_DSTAREA, tg.NORM_FRACAREA) == (R.MASKRULE_ROW, R.MASKRULE_ENTRY, R.NORM_DSTAREA, R.NORM_FRACAREA)


def _fortran_interface(src, name):
    m = re.search(r"function\s+%s\s*\(([^)]*)\)\s*&?\s*bind\s*\(\s*C\s*,\s*name\s*=\s*['\"]%s['\"]\s*\)(.*?)end\s+function" % (name, name),
                  src, flags=re.S | re.I)
    assert m, name + " has no bind(C) interface in mpg_mod.F90"
    return [a.strip().lower() for a in m.group(1).replace("&", " ").split(",")], m.group(2).lower(), m.start()


def test_fortran_binds_them():
    src = open(os.path.join(ROOT, "mpassit_amd", "fortran", "mpg_mod.F90")).read()
    low = src.lower()
    body = re.search(r"type\s*,\s*bind\(c\)\s*::\s*mpg_store_mask_opts(.*?)end\s+type\s+mpg_store_mask_opts", low, flags=re.S).group(1)
    order = [body.index(k) for k in (":: src_mask_dev", ":: dst_mask_dev", ":: rule", ":: norm_type")]
    assert order == sorted(order) and body.count("type(c_ptr)") == 2 and body.count("integer(c_int)") == 2
    assert re.search(r"mpg_maskrule_auto\s*=\s*0\s*,\s*mpg_maskrule_row\s*=\s*1\s*,\s*mpg_maskrule_entry\s*=\s*2", low)
    args, body, at = _fortran_interface(src, MASK)
    assert args == ["rh", "opts", "out"]
    assert re.search(r"type\(c_ptr\),\s*value\s*::\s*rh\b", body) and re.search(r"type\(mpg_store_mask_opts\),\s*intent\(in\)\s*::\s*opts", body)
    assert re.search(r"type\(c_ptr\),\s*intent\(out\)\s*::\s*out", body) and "mpg_store_mask_opts" in body.split("\n")[1], "the type is imported"
    args, body, at2 = _fortran_interface(src, EXM)
    assert args == ["rh", "src", "dst", "opts", "src_mask_dev", "dst_skip_dev", "out"]
    assert re.search(r"type\(mpg_points\),\s*intent\(in\)\s*::\s*src,\s*dst", body) and re.search(r"type\(mpg_extrap_opts\),\s*intent\(in\)\s*::\s*opts", body)
    assert re.search(r"type\(c_ptr\),\s*value\s*::\s*src_mask_dev,\s*dst_skip_dev", body) and re.search(r"type\(c_ptr\),\s*intent\(out\)\s*::\s*out", body)
    assert re.search(r"end\s+function\s+mpg_grid_get_xyz", src).end() < at < at2 < src.index("function mpg_dev_alloc")
    for f in ("interp_mod.F90", "mpassit_driver.F90"):
        txt = open(os.path.join(ROOT, "mpassit_amd", "fortran", f)).read()
        for name in ARGS:
            assert name not in txt
