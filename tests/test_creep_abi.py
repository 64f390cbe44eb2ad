"""CPU checks of the creep call: the header declares mpg_handle_creep, mpg_creep_opts (16 bytes) and MPG_CREEP_ALL_LEVELS in a section of
its own behind mpg_handle_conserve2nd and before the output epilogues, states the rule, and leaves the extrapolation section and the
"creep fills" remark of the mask section as they were; _lib lists, binds and exports the call; k_creep.hip and creep.h are part of the
build and keep their promises; the Python wrappers and the numpy mirror have the agreed names and defaults; the Fortran module has a
matching interface (which the driver does not use)."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CREEP = "mpg_handle_creep"
ARGS = ["mpg_handle rh", "const mpg_points *dst", "const mpg_creep_opts *opts", "mpg_handle *out"]


def _header(strip_comments=True):
    txt = open(os.path.join(ROOT, "include", "mpassit_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S) if strip_comments else txt


def test_header_declares_the_call():
    txt = _header()
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % CREEP, txt)
    assert m, CREEP + " is not declared"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == ARGS
    assert re.search(r"enum\s*\{\s*MPG_CREEP_ALL_LEVELS\s*=\s*0x7fffffff\s*\}\s*;", txt)
    s = re.search(r"typedef\s+struct\s+mpg_creep_opts\s*\{(.*?)\}\s*mpg_creep_opts\s*;", txt, flags=re.S)
    assert s and [" ".join(f.split()) for f in s.group(1).split(";") if f.strip()] == ["int num_levels", "const uint8_t *dst_skip_dev"]
    # the extrapolation call, its enum line and its struct as they were
    assert re.search(r"enum\s*\{\s*MPG_EXTRAPMETHOD_NEAREST_STOD\s*=\s*1\s*,\s*MPG_EXTRAPMETHOD_NEAREST_IDAVG\s*=\s*2\s*\}\s*;", txt)
    full = _header(strip_comments=False)
    assert "Not served: handles with pole terms, localized or windowed handles, node-located sources, creep fills. */" in full
    at = full.index("int " + CREEP + "(")
    assert full.index("int mpg_handle_conserve2nd(") < full.index("---- creep-fill extrapolation") < at < full.index("---- output epilogues")


def test_struct_layout():
    from mpassit_amd import _lib
    assert C.sizeof(_lib.CreepOpts) == 16
    assert [(n, t) for n, t in _lib.CreepOpts._fields_] == [("num_levels", C.c_int), ("dst_skip_dev", C.c_void_p)]
    assert (_lib.CreepOpts.num_levels.offset, _lib.CreepOpts.dst_skip_dev.offset) == (0, 8)
    assert (_lib.MPG_CREEP_ALL_LEVELS, _lib.CREEP_ALL_LEVELS) == (0x7fffffff, 0x7fffffff)
    # the C compiler agrees
    src = '#include <stddef.h>\n#include "mpassit_amd.h"\n_Static_assert(sizeof(mpg_creep_opts) == 16, "size");\n' \
          '_Static_assert(offsetof(mpg_creep_opts, dst_skip_dev) == 8, "offset");\n_Static_assert(MPG_CREEP_ALL_LEVELS == 2147483647, "all");\n'
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_states_the_rule():
    txt = _header(strip_comments=False)
    i = txt.index("int " + CREEP + "(")
    doc = " ".join(txt[max(0, i - 12000):i].replace("\n *", "\n").split())
    doc = doc[doc.rindex("---- creep-fill extrapolation"):]
    for phrase in ("ESMF_EXTRAPMETHOD_CREEP", "extrapNumLevels", "ESMF_EXTRAPMETHOD_CREEP_NRST_D", "supersedes", "creep fills",
                   "mpg_handle_mask first, then mpg_handle_creep with dst_skip_dev = the destination mask",
                   "an ordinary CSR handle", "no source geometry and no search", "mpg_points rules",
                   # the rule
                   "target_grid.creep_rows", "creep.h", "rounded on its own", "fp contract(off)", "the only operations are + and /",
                   "slot 0's index < 0", "an empty row", "copied verbatim", "slots in slot order", "-1 slots dropped", "weight 1.0 for a nearest handle",
                   "ascending id, p itself excluded", "id = j * snx + i", "[i - 1, i + 1] x [j - 1, j + 1]", "up to 8", "NOT the shifted 3 x 3 window",
                   "no wrap", "N1(p) as mpg_handle_patch defines it, minus p", "node neighbours of ESMF's dual mesh", "bare centres",
                   "nothing is filled, and that is success",
                   "level[p] = 0 for a mapped row", "never gets a level", "level[q] == L - 1", "ends early at the first L that assigns nothing",
                   "dst_skip only stops filling",
                   "Q = { q in Nb(p) : level[q] == L - 1 }", "m = |Q| >= 1", "ascending distinct union of the contributors' columns",
                   "acc = acc + v from 0.0", "contributors in ascending id", "in stored order", "w = acc / (double)m", "Zero values stay in the row",
                   "Duplicate columns in a mapped input row are one term each", "With m = 1", "copied exactly",
                   "creep(creep(h, a), b) has the bytes of creep(h, a + b)",
                   # the output
                   "always a new CSR handle", "n_src, n_dst, nx_dst, ny_dst and method", "no dst_frac", "longest row is recorded", "not cached",
                   "owns its arrays", "mpg_handle_release", "released right after the call", "mpg_handle_store_ms", "mpg_handle_store_stats",
                   "[1] rows filled", "[2] the last level that filled a row", "[3] rows still unmapped", "[6] the longest row",
                   "a CSR copy of the pattern", "same bytes from run to run", "no floating-point atomics", "no blocking knob",
                   "drains the Store worker", "orders itself after whatever produced rh", "reads counts back", "per level",
                   # the refusals
                   "names mpg_handle_creep", "MPG_ERR_INVALID_ARG", "NULL rh, dst, opts or out", "num_levels < 1", "both are printed",
                   "MPG_ERR_UNSUPPORTED", "MPG_MESHLOC_NODE or MPG_MESHLOC_EDGE", "no ring is defined there", "mpg_mesh_create_window",
                   "maxEdges > 12", "MPG_GRID_PERIODIC_I", "the seam would be a wall", "mpg_handle_pole_count > 0", "localized, rebased or windowed",
                   "MPG_ERR_OVERFLOW", "2^31 - 2 entries", "leaks nothing",
                   "Not served: vertices and edges; periodic destinations; distance-weighted averages; a fixed-handle output",
                   "multi-GPU sharding", "interp.py or the Fortran driver"):
        assert phrase in doc, phrase


def test_lib_lists_binds_and_exports_it():
    from mpassit_amd import _lib, build
    assert CREEP in _lib.SYMBOLS
    assert "k_creep.hip" in build.SOURCES and "creep.h" in build.HEADERS
    assert os.path.exists(os.path.join(build.CSRC, "k_creep.hip")) and os.path.exists(os.path.join(build.CSRC, "creep.h"))
    build.build()
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    assert hasattr(lib, CREEP) and re.search(r" T %s\b" % CREEP, out)
    assert list(_lib._HANDLE_CREEP_PROTO._argtypes_) == [C.c_void_p, C.POINTER(_lib.Points), C.POINTER(_lib.CreepOpts), C.c_void_p]
    assert _lib._HANDLE_CREEP_PROTO._restype_ is C.c_int and callable(_lib.handle_creep)
    # the warm-up anchor, the entry point's order and the kernel file's promises
    api = open(os.path.join(build.CSRC, "mpg_api.hip")).read()
    body = api[api.index("int mpg_handle_creep("):api.index("mpg_k_creep(rh")]
    assert re.search(r"X\(k_creep\)", api) and "store_worker_drain();" in body and "h->method = rh->method;" in body
    assert "ex_points(who, \"destination\", dst" in body, "mpg_handle_extrapolate's point-set checks, shared"
    ext = api[api.index("static int ex_extrapolate(const char *who, mpg_handle rh, const mpg_points *src, const mpg_points *dst, const mpg_extrap_opts *opts,\n"
                        "                          const uint8_t *src_mask_dev, const uint8_t *dst_skip_dev, mpg_handle *out) {"):api.index("int mpg_handle_mask(")]
    assert "creep" not in ext.lower(), "the extrapolation entry is untouched"
    kern = open(os.path.join(build.CSRC, "k_creep.hip")).read()
    code = re.sub(r"//[^\n]*", "", kern)
    assert code.index("#pragma clang fp contract(off)") < code.index("#include"), "the whole file is compiled without contraction"
    for word in ("mpg_anchor_k_creep", "mpg_scan_excl_i32", "mpg_sum_i32_i64", "mpg_sort_pairs_u64_i32", "k_cr_init", "k_cr_front", "k_cr_compact",
                 "k_cr_expand", "k_cr_heads", "k_cr_values", "k_cr_rows", "k_cr_gather0", "k_cr_gather", "cr_neighbours", "cr_joins", "cr_sum_div"):
        assert word in kern, word
    assert not re.search(r"atomic(Add|Exch|CAS)\s*\(", code) and "__shared__" not in code, "no floating-point atomics, nothing per row in LDS"
    assert re.findall(r"atomicMax\(longest", code) and not re.search(r"atomic\w+\((?!longest)", code), "one integer maximum only"
    hdr = open(os.path.join(build.CSRC, "creep.h")).read()
    hcode = re.sub(r"//[^\n]*", "", hdr)
    assert "hip/hip_runtime.h" not in hdr and "fp contract(off)" in hdr and '#include "patch.h"' in hdr
    assert "d.ring1(p, ids)" in hcode and "voc[" not in hcode and "tri[" not in hcode, "PtSrc::ring1 is reused, not copied"
    assert not re.search(r"\b(fma|pow|exp|log|sin|cos|atan2?|hypot|sqrt)\s*\(", hcode), "+ and / only"
    assert "creep.h" in open(os.path.join(ROOT, "tests", "c", "creep_test.cpp")).read()


def test_python_names_and_defaults():
    from mpassit_amd import regrid as R, target_grid as tg
    sig = inspect.signature(R.creep)
    assert list(sig.parameters) == ["rh", "dst", "num_levels", "dst_skip", "dst_loc"]
    assert sig.parameters["num_levels"].default == R.CREEP_ALL_LEVELS == tg.CREEP_ALL_LEVELS == 0x7fffffff
    assert sig.parameters["dst_skip"].default is None and sig.parameters["dst_loc"].default is None
    sig = inspect.signature(R.creep_nearest)
    assert list(sig.parameters)[:6] == ["rh", "src", "dst", "num_levels", "src_mask", "dst_skip"]
    assert sig.parameters["num_levels"].default is inspect.Parameter.empty and sig.parameters["src_mask"].default is None
    assert {"src_loc", "dst_loc"} <= set(sig.parameters)
    for name in ("creep", "creep_nearest", "CREEP_ALL_LEVELS"):
        assert name in R.__all__
    assert list(inspect.signature(tg.creep_neighbours_grid).parameters) == ["snx", "sny"]
    assert list(inspect.signature(tg.creep_neighbours_mesh).parameters) == ["voc", "tri"]
    sig = inspect.signature(tg.creep_rows)
    assert list(sig.parameters) == ["rowptr", "col", "val", "neighbours", "num_levels", "dst_skip"] and sig.parameters["dst_skip"].default is None
    # the extrapolation wrapper is as it was
    assert list(inspect.signature(R.extrapolate).parameters) == ["rh", "src", "dst", "method", "num_src_pnts", "dist_exponent", "src_loc", "dst_loc"]


def test_fortran_binds_it():
    src = open(os.path.join(ROOT, "mpassit_amd", "fortran", "mpg_mod.F90")).read()
    low = src.lower()
    assert re.search(r"mpg_creep_all_levels\s*=\s*2147483647", low)
    t = re.search(r"type,\s*bind\(c\)\s*::\s*mpg_creep_opts(.*?)end\s+type\s+mpg_creep_opts", low, flags=re.S)
    assert t and re.search(r"integer\(c_int\)\s*::\s*num_levels", t.group(1)) and re.search(r"type\(c_ptr\)\s*::\s*dst_skip_dev", t.group(1))
    assert t.group(1).index("num_levels") < t.group(1).index("dst_skip_dev")
    m = re.search(r"function\s+%s\s*\(([^)]*)\)\s*&?\s*bind\s*\(\s*C\s*,\s*name\s*=\s*['\"]%s['\"]\s*\)(.*?)end\s+function" % (CREEP, CREEP), src, flags=re.S | re.I)
    assert m, CREEP + " has no bind(C) interface in mpg_mod.F90"
    assert [a.strip().lower() for a in m.group(1).split(",")] == ["rh", "dst", "opts", "out"]
    body = m.group(2).lower()
    assert re.search(r"type\(c_ptr\),\s*value\s*::\s*rh\b", body) and re.search(r"type\(mpg_points\),\s*intent\(in\)\s*::\s*dst\b", body)
    assert re.search(r"type\(mpg_creep_opts\),\s*intent\(in\)\s*::\s*opts", body) and re.search(r"type\(c_ptr\),\s*intent\(out\)\s*::\s*out", body)
    assert "mpg_points" in body.split("\n")[1] and "mpg_creep_opts" in body.split("\n")[1], "the types are imported"
    assert re.search(r"end\s+function\s+mpg_handle_conserve2nd", src).end() < m.start() < src.index("function mpg_dev_alloc")
    for f in ("interp_mod.F90", "mpassit_driver.F90"):
        assert CREEP not in open(os.path.join(ROOT, "mpassit_amd", "fortran", f)).read()
