"""CPU checks of the patch call: the header declares mpg_handle_patch with the agreed argument list, MPG_REGRIDMETHOD_PATCH on an enum
line of its own (the existing line as it was) and MPG_PATCH_MAX_PNTS -- the new section behind the Store-time masks and before the output
epilogues -- and states the rule; _lib lists, binds and exports the call; k_patch.hip and patch.h are part of the build and keep their
promises; the Python wrappers and the numpy mirror have the agreed signatures; the Fortran module has a matching interface (which the
driver does not use)."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH = "mpg_handle_patch"
ARGS = ["mpg_handle rh", "const mpg_points *src", "const mpg_points *dst", "mpg_handle *out"]


def _header(strip_comments=True):
    txt = open(os.path.join(ROOT, "include", "mpassit_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S) if strip_comments else txt


def test_header_declares_the_call():
    txt = _header()
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % PATCH, txt)
    assert m, PATCH + " is not declared"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == ARGS
    assert re.search(r"enum\s*\{\s*MPG_REGRIDMETHOD_PATCH\s*=\s*3\s*\}\s*;", txt), "an enum line of its own"
    assert re.search(r"enum\s*\{\s*MPG_REGRIDMETHOD_BILINEAR\s*=\s*0\s*,\s*MPG_REGRIDMETHOD_CONSERVE\s*=\s*1\s*,\s*MPG_REGRIDMETHOD_NEAREST_STOD\s*=\s*2\s*\}\s*;", txt)
    assert re.search(r"#define\s+MPG_PATCH_MAX_PNTS\s+32\b", txt)
    full = _header(strip_comments=False)
    at = full.index("int " + PATCH + "(")
    assert full.index("int mpg_handle_extrapolate_masked(") < full.index("---- patch regridding") < at < full.index("---- output epilogues")


def test_header_states_the_rule():
    txt = _header(strip_comments=False)
    i = txt.index("int " + PATCH + "(")
    doc = " ".join(txt[max(0, i - 12000):i].replace("\n *", "\n").split())
    doc = doc[doc.rindex("---- patch regridding"):]
    for phrase in ("ESMF_REGRIDMETHOD_PATCH", "rh_patch", "an ordinary CSR handle", "Mesh -> Grid, Mesh -> Mesh, Grid -> Mesh and Grid -> Grid",
                   "S = 3 or 4 slots", "mpg_points rules", "mpg_handle_extrapolate",
                   # the rule
                   "rounded on its own", "fp contract(off)", "+ - * / sqrt", "mpg_mesh_get_xyz / mpg_grid_get_xyz",
                   "N1(c)", "ascending id", "valid dual triangle", "no -1 in its column", "non-zero entries of c's verticesOnCell row",
                   "id = j * snx + i", "[i0, i0 + 2] x [j0, j0 + 2]", "clamp(i - 1, 0, max(snx - 3, 0))", "full 3 x 3 block",
                   "N2(c) = the union of N1(d) over d in N1(c)", "at most MPG_PATCH_MAX_PNTS points",
                   "n = X_c", "smallest |component|", "lowest axis on ties", "t = a - (a . n) n", "e1 = t / sqrt(t . t)", "e2 = n x e1",
                   "d = X_q - X_c", "h = sqrt(max over the patch of d . d)", "u = (d . e1) / h", "v = (d . e2) / h", "(x*x' + y*y') + z*z'",
                   "phi = (1, u, v, u*u, u*v, v*v)", "(1, u, v) for degree 1", "in patch order from 0.0", "G = R^T R", "left-to-right inner products",
                   "h > 0 and every pivot s_k > 2^-26 * G_kk", "a definition, not a tuning constant",
                   "(A) degree 2 on N1 if |N1| >= 6", "(B) degree 2 on N2", "6 <= |N2| <= MPG_PATCH_MAX_PNTS", "(C) degree 1 on N1 if |N1| >= 3",
                   "(D) degree 0: the node itself with value 1", "R^T z = phi(p)", "R y = z", "L_k = sum_a phi_a(q_k) * y_a", "basis order",
                   "every slot with an index >= 0 takes part, whatever its weight", "distinct ids of the slots' patches, in ascending order",
                   "acc = acc + (b_s * L_(s,k))", "(slot, patch position) in ascending order", "Zero values stay in the row",
                   "slot 0's index < 0", "target_grid.patch_rows", "patch.h",
                   # the output
                   "n_src, n_dst, nx_dst and ny_dst", "MPG_REGRIDMETHOD_PATCH", "no dst_frac", "longest row is recorded", "not cached",
                   "owns its arrays", "mpg_handle_release", "released right after the call", "mpg_handle_store_ms", "mpg_handle_store_stats",
                   "[1] is the number of rows written", "attempts A, B, C and D", "[6] is the longest row",
                   "same bytes from run to run", "no floating-point atomics", "reads the entry count back", "drains the Store worker",
                   "patch first, then mpg_handle_mask / mpg_handle_extrapolate", "MPG_MASKRULE_AUTO picks MPG_MASKRULE_ROW", "go on refusing method 3",
                   # the refusals
                   "names mpg_handle_patch", "MPG_ERR_INVALID_ARG", "NULL argument", "both numbers are printed", "location other than ELEMENT",
                   "method is not MPG_REGRIDMETHOD_BILINEAR", "MPG_ERR_UNSUPPORTED", "CSR or 1-slot handle", "mpg_handle_pole_count > 0",
                   "localized or rebased", "source window", "mpg_mesh_create_window", "MPG_GRID_PERIODIC_I", "MPG_ERR_OVERFLOW", "2^31 - 2 entries",
                   "leaks nothing"):
        assert phrase in doc, phrase


def test_lib_lists_binds_and_exports_it():
    from mpassit_amd import _lib, build
    assert PATCH in _lib.SYMBOLS
    assert "k_patch.hip" in build.SOURCES and "patch.h" in build.HEADERS
    assert os.path.exists(os.path.join(build.CSRC, "k_patch.hip")) and os.path.exists(os.path.join(build.CSRC, "patch.h"))
    build.build()
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    assert hasattr(lib, PATCH) and re.search(r" T %s\b" % PATCH, out)
    assert list(_lib._HANDLE_PATCH_PROTO._argtypes_) == [C.c_void_p, C.POINTER(_lib.Points), C.POINTER(_lib.Points), C.c_void_p]
    assert _lib._HANDLE_PATCH_PROTO._restype_ is C.c_int and callable(_lib.handle_patch)
    assert (_lib.MPG_REGRIDMETHOD_PATCH, _lib.REGRIDMETHOD_PATCH, _lib.PATCH_MAX_PNTS) == (3, 3, 32)
    # the warm-up anchor, the entry point's order and the kernel file's promises
    api = open(os.path.join(build.CSRC, "mpg_api.hip")).read()
    body = api[api.index("int mpg_handle_patch("):api.index("mpg_k_patch(rh")]
    assert re.search(r"X\(k_patch\)", api) and "store_worker_drain();" in body and "h->method = MPG_REGRIDMETHOD_PATCH;" in body
    assert "rh->method == MPG_REGRIDMETHOD_PATCH" in api[api.index("int mpg_handle_mask("):api.index("mpg_k_handle_mask(rh")]
    kern = open(os.path.join(build.CSRC, "k_patch.hip")).read()
    code = re.sub(r"//[^\n]*", "", kern)
    assert code.index("#pragma clang fp contract(off)") < code.index("#include"), "the whole file is compiled without contraction"
    for word in ("mpg_anchor_k_patch", "mpg_scan_excl_i32", "mpg_sum_i32_i64", "k_pt_node", "k_pt_count", "k_pt_fill", "pt_attempt", "pt_slot", "pt_row_add"):
        assert word in kern, word
    assert not re.search(r"atomic(Add|Exch|CAS)\s*\(\s*&?\s*\(?\s*(double|float)", code) and "__shared__" not in code
    assert re.findall(r"atomic\w+\(&stats", code) and not re.search(r"atomic\w+\((?!&stats)", code), "integer statistics only"
    hdr = open(os.path.join(build.CSRC, "patch.h")).read()
    assert "hip/hip_runtime.h" not in hdr and "fp contract(off)" in hdr and "__host__ __device__" in hdr and "0x1p-26" in hdr
    assert not re.search(r"\b(fma|pow|exp|log|sin|cos|atan2?|hypot)\s*\(", re.sub(r"//[^\n]*", "", hdr)), "+ - * / sqrt only"
    assert "patch.h" in open(os.path.join(ROOT, "tests", "c", "patch_test.cpp")).read()


def test_python_signatures():
    from mpassit_amd import regrid as R, target_grid as tg
    assert list(inspect.signature(R.patch).parameters) == ["rh", "src", "dst", "src_loc", "dst_loc"]
    assert list(inspect.signature(R.regrid_store_patch).parameters) == ["src", "dst", "src_loc", "dst_loc"]
    for name in ("patch", "regrid_store_patch", "REGRIDMETHOD_PATCH", "PATCH_MAX_PNTS"):
        assert name in R.__all__
    assert (R.REGRIDMETHOD_PATCH, R.PATCH_MAX_PNTS, tg.REGRIDMETHOD_PATCH, tg.PATCH_MAX_PNTS) == (3, 32, 3, 32)
    assert list(inspect.signature(tg.patch_rows).parameters) == ["idx", "w", "src_xyz", "dst_xyz", "neighbours"]
    assert list(inspect.signature(tg.patch_neighbours_mesh).parameters) == ["voc", "tri"]
    assert list(inspect.signature(tg.patch_neighbours_grid).parameters) == ["snx", "sny"]
    # the two neighbourhood tables at their smallest: a shifted window keeps a full block, a narrow stagger is cut to the grid
    nbr, cnt, ring2 = tg.patch_neighbours_grid(4, 3)
    assert not ring2 and cnt.tolist() == [9] * 12 and nbr[0].tolist() == [0, 1, 2, 4, 5, 6, 8, 9, 10] and nbr[11].tolist() == [1, 2, 3, 5, 6, 7, 9, 10, 11]
    nbr, cnt, _ = tg.patch_neighbours_grid(2, 1)
    assert cnt.tolist() == [2, 2] and nbr.tolist() == [[0, 1], [0, 1]]
    voc = [[1, 2, 0], [1, 2, 3], [1, 0, 0], [2, 3, 0], [3, 0, 0]]         # vertex 1: cells 0 1 2, vertex 2: cells 0 1 3, vertex 3 has no triangle
    nbr, cnt, ring2 = tg.patch_neighbours_mesh(voc, [[0, 1, 2], [0, 1, 3], [-1, 3, 4]])
    assert ring2 and cnt.tolist() == [4, 4, 3, 3, 1]
    assert nbr.tolist() == [[0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, -1], [0, 1, 3, -1], [4, -1, -1, -1]]


def test_fortran_binds_it():
    src = open(os.path.join(ROOT, "mpassit_amd", "fortran", "mpg_mod.F90")).read()
    low = src.lower()
    assert re.search(r"mpg_regridmethod_patch\s*=\s*3", low) and re.search(r"mpg_patch_max_pnts\s*=\s*32", low)
    assert re.search(r"mpg_regridmethod_bilinear = 0, mpg_regridmethod_conserve = 1, mpg_regridmethod_nearest_stod = 2\n", low), "the old line as it was"
    m = re.search(r"function\s+%s\s*\(([^)]*)\)\s*&?\s*bind\s*\(\s*C\s*,\s*name\s*=\s*['\"]%s['\"]\s*\)(.*?)end\s+function" % (PATCH, PATCH), src, flags=re.S | re.I)
    assert m, PATCH + " has no bind(C) interface in mpg_mod.F90"
    assert [a.strip().lower() for a in m.group(1).split(",")] == ["rh", "src", "dst", "out"]
    body = m.group(2).lower()
    assert re.search(r"type\(c_ptr\),\s*value\s*::\s*rh\b", body) and re.search(r"type\(mpg_points\),\s*intent\(in\)\s*::\s*src,\s*dst", body)
    assert re.search(r"type\(c_ptr\),\s*intent\(out\)\s*::\s*out", body) and "mpg_points" in body.split("\n")[1], "the type is imported"
    assert re.search(r"end\s+function\s+mpg_handle_extrapolate_masked", src).end() < m.start() < src.index("function mpg_dev_alloc")
    for f in ("interp_mod.F90", "mpassit_driver.F90"):
        assert PATCH not in open(os.path.join(ROOT, "mpassit_amd", "fortran", f)).read()
