"""CPU checks of the second-order conservative call: the header declares mpg_handle_conserve2nd with the agreed argument list, the options
struct and MPG_REGRIDMETHOD_CONSERVE_2ND on an enum line of its own (the existing lines as they were) -- the new section behind patch
regridding and before the output epilogues -- and states the rule; _lib lists, binds and exports the call; k_conserve2nd.hip and
conserve2nd.h are part of the build and keep their promises; the Python wrappers and the numpy mirror have the agreed signatures; the
Fortran module has a matching interface (which the driver does not use)."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALL = "mpg_handle_conserve2nd"
ARGS = ["mpg_handle rh", "const mpg_points *src", "const mpg_points *dst", "const mpg_conserve2nd_opts *opts", "mpg_handle *out"]


def _header(strip_comments=True):
    txt = open(os.path.join(ROOT, "include", "mpassit_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S) if strip_comments else txt


def test_header_declares_the_call():
    txt = _header()
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % CALL, txt)
    assert m, CALL + " is not declared"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == ARGS
    assert re.search(r"enum\s*\{\s*MPG_REGRIDMETHOD_CONSERVE_2ND\s*=\s*4\s*\}\s*;", txt), "an enum line of its own"
    assert re.search(r"enum\s*\{\s*MPG_REGRIDMETHOD_PATCH\s*=\s*3\s*\}\s*;", txt), "the patch line as it was"
    assert re.search(r"enum\s*\{\s*MPG_REGRIDMETHOD_BILINEAR\s*=\s*0\s*,\s*MPG_REGRIDMETHOD_CONSERVE\s*=\s*1\s*,\s*MPG_REGRIDMETHOD_NEAREST_STOD\s*=\s*2\s*\}\s*;", txt)
    s = re.search(r"typedef\s+struct\s+mpg_conserve2nd_opts\s*\{(.*?)\}\s*mpg_conserve2nd_opts\s*;", txt, flags=re.S)
    assert s and [" ".join(f.split()) for f in s.group(1).split(";") if f.strip()] == ["int norm_type", "const uint8_t *src_mask_dev"]
    full = _header(strip_comments=False)
    at = full.index("int " + CALL + "(")
    assert full.index("int mpg_handle_patch(") < full.index("---- second-order conservative regridding") < at < full.index("---- output epilogues")


def test_header_states_the_rule():
    txt = _header(strip_comments=False)
    i = txt.index("int " + CALL + "(")
    doc = " ".join(txt[max(0, i - 16000):i].replace("\n *", "\n").split())
    doc = doc[doc.rindex("---- second-order conservative regridding"):]
    for phrase in ("ESMF_REGRIDMETHOD_CONSERVE_2ND", "an ordinary CSR handle", "Mesh -> Grid, Grid -> Mesh and Mesh -> Mesh", "no new search",
                   "the stored pairs are the candidate list", "mpg_points rules", "MPG_MESHLOC_ELEMENT", "MPG_STAGGERLOC_CENTER",
                   "the one the Store was called with", "src_mask_dev", "Green's-theorem gradient is not reproduced",
                   # the rule
                   "rounded on its own", "fp contract(off)", "+ - * / sqrt", "(x*x' + y*y') + z*z'",
                   "num = a . ((b - a) x (c - a))", "x = x / (1 + sqrt(1 + x * x))", "|x| >= 2^-10", "den <= 0 gives 0",
                   "non-zero verticesOnCell entries in listed order", "four CORNER points", "id = j * nx + i",
                   "counter-clockwise by the sign of its own fan area", "subject polygon", "the closing side last", "a x (b - a)", "1e-15 * |n|",
                   "|b - a|^2 < 1e-24", "clamped at 0", "m_q = sum_t a_t * (((p_0 + p_t) + p_(t+1)) / 3)", "area(d) is |fan area|",
                   "ascending destination id", "transposed index", "G_i is the unit vector", "stored cell centre", "frame about n = G_i",
                   "S(i) = N1(i)", "minus i", "masked cells take no part in a gradient", "d_k = ((G_k - G_i) . e1, (G_k - G_i) . e2)",
                   "|S| >= 2", "|N1| <= MPG_PATCH_MAX_PNTS", "det = M00 * M11 - M01 * M01 > 2^-26 * (M00 * M11)",
                   "(M11 * dx - M01 * dy) / det", "b_i = -(sum_k b_k)", "single entry i with b = 0", "stays first order",
                   "delta_q = ((m_q / A_q - M_i / A_i) . e1", "0 when A_q <= 0 or A_i <= 0", "w_q = A_q / area(d)", "in stored order",
                   "ascending distinct union of the stencils", "mpg_handle_compose", "acc = acc + (w_q * t)", "g = (dx * bx) + (dy * by)",
                   "t = 1.0 + g", "Zero values stay in the row", "An empty input row stays empty", "carried over bit for bit",
                   "sum_j area(d_j) * c_(j,e) = A_e", "sum_q A_q delta_q = 0", "sum_k b_k = 0", "weights can be negative", "no limiter",
                   "the rim is only first-order accurate", "target_grid.conserve2nd_rows", "conserve2nd.h",
                   # the output
                   "n_src, n_dst, nx_dst and ny_dst", "MPG_REGRIDMETHOD_CONSERVE_2ND", "longest row is recorded", "not cached", "owns its arrays",
                   "mpg_handle_release", "released right after the call", "mpg_handle_store_ms", "[1] pairs clipped",
                   "[2] sources with a passing stencil", "[3] sources without one", "[4] stencil entries", "[6] the longest row",
                   "same bytes from run to run", "no floating-point atomics", "compose_block_rows", "drains the Store worker",
                   "MPG_MASKRULE_ENTRY", "then call this with the same source mask", "MPG_MASKRULE_AUTO refuses method 4",
                   # the refusals
                   "names mpg_handle_conserve2nd", "MPG_ERR_INVALID_ARG", "NULL argument", "both numbers are printed", "unknown norm_type",
                   "method is not MPG_REGRIDMETHOD_CONSERVE", "grid without CORNER coordinates", "MPG_ERR_UNSUPPORTED", "a fixed handle",
                   "pole terms", "localized, rebased or windowed", "mpg_mesh_create_window", "maxEdges > 12", "MPG_GRID_PERIODIC_I",
                   "MPG_ERR_OVERFLOW", "2^31 - 2 entries", "outgrew its slots", "leaks nothing",
                   # not served
                   "ESMF's own gradient", "a limiter", "node-located fields", "_begin variant", "multi-GPU sharding", "Fortran driver",
                   "-m conserve2nd"):
        assert phrase in doc, phrase


def test_lib_lists_binds_and_exports_it():
    from mpassit_amd import _lib, build
    assert CALL in _lib.SYMBOLS
    assert "k_conserve2nd.hip" in build.SOURCES and "conserve2nd.h" in build.HEADERS
    assert os.path.exists(os.path.join(build.CSRC, "k_conserve2nd.hip")) and os.path.exists(os.path.join(build.CSRC, "conserve2nd.h"))
    build.build()
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    assert hasattr(lib, CALL) and re.search(r" T %s\b" % CALL, out)
    assert list(_lib._HANDLE_CONSERVE2ND_PROTO._argtypes_) == [C.c_void_p, C.POINTER(_lib.Points), C.POINTER(_lib.Points),
                                                              C.POINTER(_lib.Conserve2ndOpts), C.c_void_p]
    assert _lib._HANDLE_CONSERVE2ND_PROTO._restype_ is C.c_int and callable(_lib.handle_conserve2nd)
    assert [(n, t) for n, t in _lib.Conserve2ndOpts._fields_] == [("norm_type", C.c_int), ("src_mask_dev", C.c_void_p)]
    assert (_lib.MPG_REGRIDMETHOD_CONSERVE_2ND, _lib.REGRIDMETHOD_CONSERVE_2ND) == (4, 4)
    # the warm-up anchor, the entry point's order, the kernel file's promises
    api = open(os.path.join(build.CSRC, "mpg_api.hip")).read()
    body = api[api.index("int mpg_handle_conserve2nd("):api.index("mpg_k_conserve2nd(rh")]
    assert re.search(r"X\(k_conserve2nd\)", api) and "store_worker_drain();" in body and "h->method = MPG_REGRIDMETHOD_CONSERVE_2ND;" in body
    mask = api[api.index("int mpg_handle_mask("):api.index("mpg_k_handle_mask(rh")]
    assert "CONSERVE_2ND" not in mask, "mpg_handle_mask is unchanged"
    kern = open(os.path.join(build.CSRC, "k_conserve2nd.hip")).read()
    code = re.sub(r"//[^\n]*", "", kern)
    assert code.index("#pragma clang fp contract(off)") < code.index("#include"), "the whole file is compiled without contraction"
    for word in ("mpg_anchor_k_conserve2nd", "mpg_scan_excl_i32", "mpg_sum_i32_i64", "mpg_k_transpose_build", "mpg_k_compose_pattern", "LdsPoly",
                 "clip_halfspace_lds", "CLIP_NT", "k_c2_cells", "k_c2_stencil", "k_c2_piece", "k_c2_centroid", "k_c2_entry", "k_c2_values",
                 "c2_tri_area", "c2_moment_add", "c2_sten_pass", "c2_offset", "c2_t", "TmpBuf"):
        assert word in kern, word
    assert not re.search(r"atomic(Add|Exch|CAS)\s*\(\s*&?\s*\(?\s*(double|float)", code), "no floating-point atomics"
    assert set(re.findall(r"atomic\w+\(([^,]+),", code)) == {"&stats[0]", "&stats[1]", "truncated"}, "integer statistics and the flag only"
    assert "DevBuf<" not in re.sub(r"out->\w+", "", code), "all temporaries are TmpBuf"
    hdr = open(os.path.join(build.CSRC, "conserve2nd.h")).read()
    assert "hip/hip_runtime.h" not in hdr and "fp contract(off)" in hdr and "__host__ __device__" in hdr and "0x1p-26" in hdr
    assert not re.search(r"\b(fma|pow|exp|log|sin|cos|atan2?|hypot)\s*\(", re.sub(r"//[^\n]*", "", hdr)), "+ - * / sqrt only"
    assert "conserve2nd.h" in open(os.path.join(ROOT, "tests", "c", "conserve2nd_test.cpp")).read()
    # the symbolic job is shared with mpg_handle_compose, whose own entry is a thin caller of it
    comp = open(os.path.join(build.CSRC, "k_compose.hip")).read()
    assert "int mpg_k_compose_pattern(" in comp and comp.count("co_compose(") == 3


def test_python_signatures():
    from mpassit_amd import regrid as R, target_grid as tg
    assert list(inspect.signature(R.conserve_2nd).parameters) == ["rh", "src", "dst", "norm", "src_mask", "src_loc", "dst_loc"]
    assert list(inspect.signature(R.regrid_store_conserve_2nd).parameters) == ["src", "dst", "norm"]
    assert inspect.signature(R.conserve_2nd).parameters["norm"].default == R.NORM_DSTAREA
    for name in ("conserve_2nd", "regrid_store_conserve_2nd", "REGRIDMETHOD_CONSERVE_2ND"):
        assert name in R.__all__
    assert (R.REGRIDMETHOD_CONSERVE_2ND, tg.REGRIDMETHOD_CONSERVE_2ND) == (4, 4)
    assert list(inspect.signature(tg.conserve2nd_rows).parameters) == ["rowptr", "col", "src_polys", "dst_polys", "neighbours", "norm", "src_mask"]
    assert list(inspect.signature(tg.conserve2nd_polygons_mesh).parameters) == ["voc", "vert_xyz", "cell_xyz"]
    assert list(inspect.signature(tg.conserve2nd_polygons_grid).parameters) == ["corner_xyz", "nx", "ny", "center_xyz"]
    # the mirror at its smallest: one source square over one identical destination square has no neighbours -> first order, weight 1
    import numpy as np
    h = 0.01
    sq = np.array([[h, h, 1.0], [-h, h, 1.0], [-h, -h, 1.0], [h, -h, 1.0]])
    sq /= np.linalg.norm(sq, axis=1, keepdims=True)
    polys = (sq[None], np.array([4]), np.array([[0.0, 0.0, 1.0]]))
    rp, col, val = tg.conserve2nd_rows([0, 1], [0], polys, polys[:2], tg.patch_neighbours_grid(1, 1), tg.NORM_DSTAREA)
    assert rp.tolist() == [0, 1] and col.tolist() == [0] and val.tolist() == [1.0]


def test_fortran_binds_it():
    src = open(os.path.join(ROOT, "mpassit_amd", "fortran", "mpg_mod.F90")).read()
    low = src.lower()
    assert re.search(r"mpg_regridmethod_conserve_2nd\s*=\s*4", low) and re.search(r"mpg_regridmethod_patch\s*=\s*3", low)
    assert re.search(r"mpg_regridmethod_bilinear = 0, mpg_regridmethod_conserve = 1, mpg_regridmethod_nearest_stod = 2\n", low), "the old line as it was"
    t = re.search(r"type,\s*bind\(c\)\s*::\s*mpg_conserve2nd_opts(.*?)end\s+type", low, flags=re.S)
    assert t and re.search(r"integer\(c_int\)\s*::\s*norm_type.*type\(c_ptr\)\s*::\s*src_mask_dev", t.group(1), flags=re.S), "the C struct's order"
    m = re.search(r"function\s+%s\s*\(([^)]*)\)\s*&?\s*bind\s*\(\s*C\s*,\s*name\s*=\s*['\"]%s['\"]\s*\)(.*?)end\s+function" % (CALL, CALL), src, flags=re.S | re.I)
    assert m, CALL + " has no bind(C) interface in mpg_mod.F90"
    assert [a.strip().lower() for a in m.group(1).split(",")] == ["rh", "src", "dst", "opts", "out"]
    body = m.group(2).lower()
    assert re.search(r"type\(c_ptr\),\s*value\s*::\s*rh\b", body) and re.search(r"type\(mpg_points\),\s*intent\(in\)\s*::\s*src,\s*dst", body)
    assert re.search(r"type\(mpg_conserve2nd_opts\),\s*intent\(in\)\s*::\s*opts", body) and re.search(r"type\(c_ptr\),\s*intent\(out\)\s*::\s*out", body)
    assert "mpg_points" in body.split("\n")[1] and "mpg_conserve2nd_opts" in body.split("\n")[1], "the types are imported"
    assert re.search(r"end\s+function\s+mpg_handle_patch", src).end() < m.start() < src.index("function mpg_dev_alloc")
    for f in ("interp_mod.F90", "mpassit_driver.F90"):
        assert CALL not in open(os.path.join(ROOT, "mpassit_amd", "fortran", f)).read()
