"""CPU checks of the Grid -> Grid boundary between two grids: the header declares mpg_regrid_store_grid_to_grid and
mpg_regrid_store_conserve_grid_to_grid with their exact argument lists and states the rules, _lib lists and binds both, the built library
exports them, the Python wrappers have the agreed signatures and refuse bad arguments before any device call, the Fortran module has
matching bind(C) interfaces, the new source is built, anchored and contraction-free, the cache keys are new kinds appended to the old
ones -- and the phrases the older boundary tests rely on are still where they look for them."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORE, CONSERVE = "mpg_regrid_store_grid_to_grid", "mpg_regrid_store_conserve_grid_to_grid"
STORE_ARGS = ["mpg_grid src", "int src_staggerloc", "mpg_grid dst", "int dst_staggerloc", "int regridmethod", "int pole_method", "mpg_handle *out"]
CONSERVE_ARGS = ["mpg_grid src", "mpg_grid dst", "int norm_type", "mpg_handle *out"]
CSRC = os.path.join(ROOT, "mpassit_amd", "csrc")


def _header(strip_comments=True):
    txt = open(os.path.join(ROOT, "include", "mpassit_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S) if strip_comments else txt


def _doc(name, start):
    txt = _header(strip_comments=False)
    i = txt.index("int " + name + "(")
    doc = " ".join(re.sub(r"\n \*(?!/)", " ", txt[max(0, i - 9000):i]).split())   # (the comment's line leaders dropped: a phrase may wrap)
    return doc[doc.rindex(start):]


def test_header_declares_both_calls_in_one_block():
    txt = _header()
    for name, want in ((STORE, STORE_ARGS), (CONSERVE, CONSERVE_ARGS)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, name + " is not declared"
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want
        assert m.start() > txt.index("int mpg_handle_creep("), "the block sits behind every older Store and handle call"
    assert re.search(r"int\s+%s\s*\([^)]*\)\s*;\s*int\s+%s\s*\(" % (STORE, CONSERVE), txt)


def test_header_states_the_rules():
    doc = _doc(STORE, "Grid -> Grid between two grids: ESMF_FieldRegridStore")
    for phrase in ("source index = j * snx + i", "n_src = snx * sny", "CORNER included", "n_dst = dnx * dny, nx_dst = dnx, ny_dst = dny",
                   "[lev][dny][dnx]", "src == dst is allowed", "periodic flag is irrelevant for bilinear and nearest", "row block of a larger grid",
                   "the rule of mpg_regrid_store_to_mesh", "lowest passing quad id", "grid_inside_tol_exp", "slots A, B, C, D",
                   "A fixed 4-slot handle", "idx -1", "identical bytes", "SOURCE grid's inverse projection", "pyramid walk",
                   'mpg_tune("store_boxes", 0)', "mpg_handle_store_path", "src_staggerloc must be MPG_STAGGERLOC_CENTER",
                   "The rule of mpg_regrid_store_periodic_to_mesh", "seam quads", "pole caps under pole_method", "end-row hemisphere rule",
                   "MPG_GRID_NO_*_POLE", "CSR handle without pole terms", "quad rows have 4 entries, cap rows nx",
                   "MPG_POLEMETHOD_NONE or MPG_POLEMETHOD_ALLAVG on every call", "it is 0 in the cache key",
                   "the rule of the Grid -> Mesh nearest Store", "A fixed 1-slot handle; every point is mapped",
                   "MPG_REGRIDMETHOD_CONSERVE -> MPG_ERR_UNSUPPORTED; the message names " + CONSERVE,
                   "(i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1), index j * nx + i", "without CORNER coordinates -> MPG_ERR_INVALID_ARG",
                   "word for word", "subject polygon", "sign of its own fan area", "sides in listed order", "a x (b - a)", "1e-15 * |n|",
                   "|b - a|^2 < 1e-24", "clamped at 0", "no floating-point contraction", "columns ascending", "MPG_NORM_DSTAREA: w = I / area(d)",
                   "MPG_NORM_FRACAREA: w = I / sum_s I", "I <= 1e-14 * area(d)", "empty row", "ascending source index", "mpg_handle_get_dst_frac",
                   "no atomic decides a stored byte", "collapsed pole sides bound nothing", "a cell without area is part of no pair",
                   "2 e2 + 1e-9", "no pair with I > 0 is removed", "the only candidate route", "mpg_handle_store_path reports 0",
                   "[1] pairs clipped", "[6] vertex slots", "fewer than 2 x 2 source points for bilinear", "MPG_ERR_OVERFLOW: counts beyond int32",
                   "nnz >= 2^31", "outgrew its vertex slots", "both grids, both staggers and the method", "inside_tol_exp for bilinear",
                   "pole_method for a periodic source", "norm_type for the conservative Store", "collide with no other Store's key",
                   "EITHER grid is destroyed", "There are no _begin variants", "whose source grid is not its destination grid is marked",
                   "MPG_ERR_UNSUPPORTED for it", "mpg_handle_patch (non-periodic bilinear)", "mpg_handle_compose"):
        assert phrase in doc, phrase


def test_older_phrases_are_still_in_place():
    """The destaggering Store keeps its words and now points at the new calls; the new block stays out of the older tests' comment
    searches; the dst fraction message names the new Store after the two it named."""
    txt = " ".join(_header(strip_comments=False).split())
    assert "Grid -> Grid on the same grid, CENTER -> EDGE1/EDGE2 bilinear (interp.F90:298,316)." in txt
    head = _doc("mpg_regrid_store_grid", "Grid -> Grid on the same grid")
    assert STORE in head and CONSERVE in head
    new = _doc(STORE, "Grid -> Grid between two grids: ESMF_FieldRegridStore")
    for start in ("Grid -> Mesh: ESMF_FieldRegridStore", "Periodic Grid -> Mesh: ESMF_FieldRegridStore", "Mesh -> Mesh: ESMF_FieldRegridStore",
                  "Conservative Mesh -> Mesh: ESMF_FieldRegridStore", "Regrid from rows to rows", "output epilogues"):
        assert start not in new, start
        assert start in txt, start
    assert txt.index("int mpg_handle_creep(") < txt.index("Grid -> Grid between two grids") < txt.index("---- output epilogues")
    api = open(os.path.join(CSRC, "mpg_api.hip")).read()
    flat = lambda s: " ".join(s.split()).replace('" "', "")
    assert "mpg_regrid_store_grid: only bilinear CENTER -> EDGE1/EDGE2 is used by the reference" in flat(api)
    frac = flat(api[api.index("int mpg_handle_get_dst_frac("):api.index("int mpg_handle_release(")])
    assert "the handle has no destination fraction (mpg_regrid_store_conserve_to_mesh stores one, and so does mpg_regrid_store_conserve_mesh" in frac
    assert frac.index("mpg_regrid_store_conserve_mesh") < frac.index(CONSERVE)
    entry = flat(api[api.index("int " + STORE + "("):api.index("int " + CONSERVE + "(")])
    assert "conservative regridding is not served by this call" in entry and CONSERVE + " is the conservative Store between two grids" in entry
    assert "takes its CENTER points only" in entry and "NPNTAVG and TEETH are not built" in entry


def test_cache_kinds_and_keys_are_appended():
    cache = open(os.path.join(CSRC, "store_cache.h")).read()
    enum = re.search(r"enum StoreKind \{(.*?)\}", cache, flags=re.S).group(1)
    kinds = [k.split("=")[0].strip() for k in enum.split(",") if k.strip()]
    assert kinds == ["STORE_MESH_TO_GRID", "STORE_GRID_TO_GRID", "STORE_GRID_TO_MESH", "STORE_PERIODIC_TO_MESH", "STORE_CONSERVE_TO_MESH",
                     "STORE_MESH_TO_MESH", "STORE_CONSERVE_MESH_TO_MESH", "STORE_GRID_TO_OTHER_GRID", "STORE_CONSERVE_GRID_TO_GRID", "STORE_KIND_COUNT"]
    ctors = re.findall(r"static StoreKey (\w+)\(", cache)
    assert ctors == ["mesh_to_grid", "grid_to_grid", "grid_to_mesh", "periodic_to_mesh", "conserve_to_mesh", "mesh_to_mesh", "conserve_mesh_to_mesh",
                     "grid_to_other_grid", "conserve_grid_to_grid"]
    api = open(os.path.join(CSRC, "mpg_api.hip")).read()
    table = re.search(r"table\[STORE_KIND_COUNT\] = \{(.*?)\}", api, flags=re.S).group(1)
    assert [f.strip() for f in table.split(",")] == ["store_mesh_build", "store_grid_build", "store_to_mesh_build", "store_periodic_to_mesh_build",
                                                     "store_conserve_to_mesh_build", "store_mesh_mesh_build", "store_conserve_mesh_build",
                                                     "store_grid_to_grid_build", "store_conserve_grid_build"]
    assert "_begin" not in api[api.index("int " + STORE + "("):api.index("static StoreBuildFn store_build_fn(StoreKind kind) {")]


def test_the_wind_chain_is_guarded_on_the_host():
    wind = open(os.path.join(CSRC, "k_wind.hip")).read()
    dims = wind[wind.index("int mpg_wind_pair_dims("):wind.index("int mpg_k_wind_destagger(")]
    assert "if (h->cross_grid) return MPG_ERR_UNSUPPORTED;" in dims
    api = open(os.path.join(CSRC, "mpg_api.hip")).read()
    assert api.count("h->cross_grid = x.src_grid != x.dst_grid;") == 2
    assert "bool cross_grid = false;" in open(os.path.join(CSRC, "mpg_internal.h")).read()


def test_lib_lists_binds_and_exports_them():
    from mpassit_amd import _lib, build
    assert STORE in _lib.SYMBOLS and CONSERVE in _lib.SYMBOLS
    build.build()
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    for name in (STORE, CONSERVE):
        assert hasattr(lib, name)
        assert re.search(r" T %s\b" % name, out)
    at = _lib._STORE_GRID_TO_GRID_PROTO._argtypes_
    assert len(at) == 7 and _lib._STORE_GRID_TO_GRID_PROTO._restype_ is C.c_int
    assert at[0] is C.c_void_p and at[2] is C.c_void_p and all(at[k] is C.c_int for k in (1, 3, 4, 5))
    at = _lib._STORE_CONSERVE_GRID_TO_GRID_PROTO._argtypes_
    assert len(at) == 4 and at[2] is C.c_int and _lib._STORE_CONSERVE_GRID_TO_GRID_PROTO._restype_ is C.c_int
    assert callable(_lib.regrid_store_grid_to_grid) and callable(_lib.regrid_store_conserve_grid_to_grid)


def test_python_signatures():
    from mpassit_amd import regrid as R
    sig = inspect.signature(R.regrid_store_grid_to_grid)
    assert list(sig.parameters) == ["src_grid", "dst_grid", "regridmethod", "src_staggerloc", "dst_staggerloc", "pole_method"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["regridmethod"], d["src_staggerloc"], d["dst_staggerloc"], d["pole_method"]) == (R.REGRIDMETHOD_BILINEAR, R.STAGGERLOC_CENTER,
                                                                                                R.STAGGERLOC_CENTER, R.POLEMETHOD_ALLAVG)
    sig = inspect.signature(R.regrid_store_conserve_grid_to_grid)
    assert list(sig.parameters) == ["src_grid", "dst_grid", "norm"] and sig.parameters["norm"].default == R.NORM_DSTAREA
    assert "regrid_store_grid_to_grid" in R.__all__ and "regrid_store_conserve_grid_to_grid" in R.__all__
    for fn, words in ((R.regrid_store_patch, ("regrid_store_grid_to_grid(src, dst, REGRIDMETHOD_BILINEAR",)),
                      (R.regrid_store_conserve_2nd, ("regrid_store_conserve_grid_to_grid(src, dst, norm)", "src is not dst"))):
        body = inspect.getsource(fn)
        for w in words:
            assert w in body, (fn.__name__, w)


def test_wrappers_reject_bad_arguments_before_any_device_call():
    """No GPU, no mpg_init: every one of these must fail in Python, with a message of its own (a call that reached the library would
    raise MpgError 'mpg_init has not been called')."""
    from mpassit_amd import regrid as R

    class NotAGrid:
        _h = None

    fake = R.Grid.__new__(R.Grid)             # a Grid object without a device grid behind it
    fake._h = C.c_void_p()
    mesh = R.Mesh.__new__(R.Mesh)
    mesh._h = C.c_void_p()
    for a, b in ((NotAGrid(), fake), (fake, None), (mesh, fake), (fake, mesh)):
        with pytest.raises(TypeError, match="Grid objects"):
            R.regrid_store_grid_to_grid(a, b)
        with pytest.raises(TypeError, match="Grid objects"):
            R.regrid_store_conserve_grid_to_grid(a, b)
    for bad in (2, -1, None):
        with pytest.raises(ValueError, match="norm"):
            R.regrid_store_conserve_grid_to_grid(fake, fake, norm=bad)
    with pytest.raises(ValueError, match="two different Grids"):
        R.regrid_store_conserve_2nd(fake, fake)


def test_fortran_binds_them():
    src = open(os.path.join(ROOT, "mpassit_amd", "fortran", "mpg_mod.F90")).read()

    def interface(name):
        m = re.search(r"function\s+%s\s*\(([^)]*)\)\s*&?\s*bind\s*\(\s*C\s*,\s*name\s*=\s*['\"]%s['\"]\s*\)(.*?)end\s+function" % (name, name),
                      src, flags=re.S | re.I)
        assert m, name + " has no bind(C) interface in mpg_mod.F90"
        return [a.strip().lower() for a in m.group(1).replace("&", " ").split(",")], m.group(2).lower()

    args, body = interface(STORE)
    assert args == ["src", "src_staggerloc", "dst", "dst_staggerloc", "regridmethod", "pole_method", "rh"]
    for a in ("src_staggerloc", "dst_staggerloc", "regridmethod", "pole_method"):
        assert re.search(r"integer\(c_int\),\s*value\s*::.*\b%s\b" % a, body), a
    for a in ("src", "dst"):
        assert re.search(r"type\(c_ptr\),\s*value\s*::.*\b%s\b" % a, body), a
    assert re.search(r"type\(c_ptr\),\s*intent\(out\)\s*::\s*rh\b", body)
    args, body = interface(CONSERVE)
    assert args == ["src", "dst", "norm_type", "rh"]
    assert re.search(r"integer\(c_int\),\s*value\s*::.*\bnorm_type\b", body)
    for a in ("src", "dst"):
        assert re.search(r"type\(c_ptr\),\s*value\s*::.*\b%s\b" % a, body), a
    assert re.search(r"type\(c_ptr\),\s*intent\(out\)\s*::\s*rh\b", body)


def test_kernel_source_is_built_anchored_and_contraction_free():
    from mpassit_amd import build
    assert "k_store_conserve_grid.hip" in build.SOURCES and "conserve_clip.h" in build.HEADERS
    api = open(os.path.join(CSRC, "mpg_api.hip")).read()
    assert "X(k_store_conserve_grid)" in api
    store = open(os.path.join(CSRC, "k_store_conserve_grid.hip")).read()
    code = store[store.index("#pragma clang fp contract(off)"):]
    assert store.index("#pragma clang fp contract(off)") < store.index("#include"), "the pragma comes ahead of every include"
    assert '#include "conserve_clip.h"' in code and "const void *mpg_anchor_k_store_conserve_grid()" in code
    # the clip step lives in ONE place; the polygon sits in LDS as [vertex][component][lane]; at least 4 + 4 vertex slots
    for name in ("struct LdsPoly", "int clip_halfspace_lds("):
        assert name not in store, name
    assert "clip_halfspace_lds(" in code and "LdsPoly" in code and "__shared__" in code
    assert int(re.search(r"#define CG_SLOTS (\d+)", code).group(1)) >= 8
    assert "2.0 * e2 + 1e-9" in code and "mpg_scan_excl_i32" in code and "walk_filter" in code
    # no atomic but the truncation flag of the error path; no fixed list length, no spill path
    assert re.findall(r"atomic\w+\(", code) == ["atomicOr("] and "atomicOr(truncated, 1)" in code
    assert "no pair with I > 0 is removed" in store and "store_path is 0" in store
    # the existing searches take a destination point set: their kernels are launched by the wrappers the new Store calls
    for f, fn in (("k_store_to_mesh.hip", "mpg_k_store_to_points"), ("k_store_periodic_to_mesh.hip", "mpg_k_store_periodic_to_points")):
        txt = open(os.path.join(CSRC, f)).read()
        assert "int %s(" % fn in txt and "const PointSet &dst, int64_t n" in txt and fn + "(" in api
