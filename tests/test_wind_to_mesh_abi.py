"""CPU checks of the wind chain turned round: the header declares mpg_wind_to_mesh_dev and mpg_mesh_rotang_dev with their exact argument
lists and states the value rule, _lib lists and binds both, the built library exports them, the Python wrappers have the agreed
signatures, the Fortran module has matching bind(C) interfaces (which the driver does not use), and the closed-form rotation angle
(target_grid.rotang_at) has the sign of the reference's get_rotang."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import LAMBERT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIND, ROTANG = "mpg_wind_to_mesh_dev", "mpg_mesh_rotang_dev"
WIND_ARGS = ["mpg_handle rh_u", "mpg_handle rh_v", "const double *cosa_dev", "const double *sina_dev", "const void *u_dev", "const void *v_dev",
             "int src_type", "int64_t u_level_stride", "int64_t v_level_stride", "int nlev", "void *ue_dev", "void *ve_dev", "int dst_type",
             "int dst_layout", "void *hip_stream"]
ROTANG_ARGS = ["mpg_grid grid", "mpg_mesh mesh", "int meshloc", "double *cosa_dev", "double *sina_dev", "void *hip_stream"]


def _header(strip_comments=True):
    txt = open(os.path.join(ROOT, "include", "mpassit_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S) if strip_comments else txt


def _doc(name, start):
    txt = _header(strip_comments=False)
    i = txt.index("int " + name + "(")
    doc = " ".join(txt[max(0, i - 9000):i].replace("\n *", "\n").split())
    return doc[doc.rindex(start):]


def test_header_declares_both_calls():
    txt = _header()
    for name, want in ((WIND, WIND_ARGS), (ROTANG, ROTANG_ARGS)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, name + " is not declared"
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want
    # next to the forward chain
    full = _header(strip_comments=False)
    assert full.index("int mpg_wind_destagger_dev(") < full.index("int " + WIND + "(") < full.index("int mpg_dev_alloc(")


def test_header_states_the_rule():
    doc = _doc(WIND, "The wind chain turned round")
    for phrase in ("a = wsum_fixed<NNZ>(w_u, U[idx_u])", "exactly mpg_regrid_to_mesh_dev(rh_u, dst F64, scale 1, offset 0)",
                   "b = wsum_fixed<NNZ>(w_v, V[idx_v])", "ue = a * ca - b * sa ; ve = a * sa + b * ca",
                   "four products and two sums, each rounded", "no rotation: ue = a, ve = b", "store (TD)ue, (TD)ve",
                   "one rounding to the destination type", "either handle", "(TD)(+0.0)", "hipGraph", "MPG_TYPE_BE", "CSR handles", "pole caps",
                   "interp.F90:737-748", "No atomics", "MPG_ERR_UNSUPPORTED", "MPG_ERR_INVALID_ARG", "MPG_ERR_OVERFLOW", "rh_u == rh_v",
                   "u_level_stride", "MPG_LAYOUT_LEV_FAST [cell][lev]", "mpg_wind_destagger_pitched_dev"):
        assert phrase in doc, phrase
    doc = _doc(ROTANG, "cos / sin of the rotation angle")
    for phrase in ("-hemi * cone * wrap180(lon - stand_lon)", "atan2(y, x)", "PROJ_LC only", "pass NULL angles", "mpg_mesh_create_window",
                   "get_rotang"):
        assert phrase in doc, phrase


def test_lib_lists_binds_and_exports_them():
    from mpassit_amd import _lib, build
    assert WIND in _lib.SYMBOLS and ROTANG in _lib.SYMBOLS
    assert "k_wind_pair.hip" in build.SOURCES
    build.build()
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    for name in (WIND, ROTANG):
        assert hasattr(lib, name)
        assert re.search(r" T %s\b" % name, out)
    at = _lib._WIND_TO_MESH_PROTO._argtypes_
    assert len(at) == 15 and _lib._WIND_TO_MESH_PROTO._restype_ is C.c_int
    assert at[7] is C.c_int64 and at[8] is C.c_int64, "the level strides are 64-bit"
    assert [at[i] for i in (6, 9, 12, 13)] == [C.c_int] * 4
    assert all(at[i] is C.c_void_p for i in (0, 1, 2, 3, 4, 5, 10, 11, 14))
    at = _lib._MESH_ROTANG_PROTO._argtypes_
    assert len(at) == 6 and at[2] is C.c_int and _lib._MESH_ROTANG_PROTO._restype_ is C.c_int
    assert callable(_lib.wind_to_mesh_dev) and callable(_lib.mesh_rotang_dev)


def test_python_signatures():
    from mpassit_amd import regrid as R
    sig = inspect.signature(R.wind_to_mesh)
    assert list(sig.parameters) == ["rh_u", "rh_v", "cosa", "sina", "u", "v", "nlev", "layout", "out_dtype", "outs"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["layout"], d["out_dtype"], d["outs"]) == (R.LAYOUT_CELL_FAST, None, None)
    assert d["nlev"] is inspect.Parameter.empty
    sig = inspect.signature(R.mesh_rotang)
    assert list(sig.parameters) == ["grid", "mesh", "meshloc"] and sig.parameters["meshloc"].default == R.MESHLOC_ELEMENT
    sig = inspect.signature(R.wind_to_mesh_autograd)
    assert list(sig.parameters) == ["rh_u", "rh_v", "cosa", "sina", "u", "v", "nlev", "layout"]
    assert sig.parameters["layout"].default == R.LAYOUT_CELL_FAST
    for name in ("wind_to_mesh", "mesh_rotang", "wind_to_mesh_autograd"):
        assert name in R.__all__


def _fortran_interface(src, name):
    m = re.search(r"function\s+%s\s*\(([^)]*)\)\s*&?\s*bind\s*\(\s*C\s*,\s*name\s*=\s*['\"]%s['\"]\s*\)(.*?)end\s+function" % (name, name),
                  src, flags=re.S | re.I)
    assert m, name + " has no bind(C) interface in mpg_mod.F90"
    return [a.strip().lower() for a in m.group(1).replace("&", " ").split(",")], m.group(2).lower()


def test_fortran_binds_them():
    src = open(os.path.join(ROOT, "mpassit_amd", "fortran", "mpg_mod.F90")).read()
    args, body = _fortran_interface(src, WIND)
    assert args == ["rh_u", "rh_v", "cosa_dev", "sina_dev", "u_dev", "v_dev", "src_type", "u_level_stride", "v_level_stride", "nlev", "ue_dev",
                    "ve_dev", "dst_type", "dst_layout", "hip_stream"]
    for a in ("src_type", "nlev", "dst_type", "dst_layout"):
        assert re.search(r"integer\(c_int\),\s*value\s*::.*\b%s\b" % a, body), a
    for a in ("u_level_stride", "v_level_stride"):
        assert re.search(r"integer\(c_int64_t\),\s*value\s*::.*\b%s\b" % a, body), a
    for a in ("rh_u", "rh_v", "cosa_dev", "sina_dev", "u_dev", "v_dev", "ue_dev", "ve_dev", "hip_stream"):
        assert re.search(r"type\(c_ptr\),\s*value\s*::.*\b%s\b" % a, body), a
    args, body = _fortran_interface(src, ROTANG)
    assert args == ["grid", "mesh", "meshloc", "cosa_dev", "sina_dev", "hip_stream"]
    assert re.search(r"integer\(c_int\),\s*value\s*::.*\bmeshloc\b", body)
    for a in ("grid", "mesh", "cosa_dev", "sina_dev", "hip_stream"):
        assert re.search(r"type\(c_ptr\),\s*value\s*::.*\b%s\b" % a, body), a
    # the driver and interp_mod do not use them: the reference's job takes no wind back to the mesh
    for f in ("interp_mod.F90", "mpassit_driver.F90"):
        txt = open(os.path.join(ROOT, "mpassit_amd", "fortran", f)).read()
        assert WIND not in txt and ROTANG not in txt


@pytest.mark.parametrize("nx,ny", [(61, 41), (181, 107)])
def test_rotang_at_has_the_sign_of_get_rotang(nx, ny):
    """The closed form against the reference's centred differences on the 30-km Lambert grids: 1e-4 on interior rows (measured 2.3e-6 in
    sina, 5.8e-5 in cosa -- the latter over all rows); the opposite sign misses by more than 0.1."""
    from mpassit_amd import target_grid as tg
    g = tg.define_target_grid_params("lambert", nx, ny, dx=30000.0, dy=30000.0, **LAMBERT)
    want_c, want_s = tg.get_rotang(g.lat, g.lon)
    assert np.array_equal(want_c, g.cosa) and np.array_equal(want_s, g.sina)
    cosa, sina = tg.rotang_at(g.proj, g.lon)
    assert cosa.shape == g.lon.shape and sina.shape == g.lon.shape
    ds, dc = np.abs(sina - want_s)[1:-1].max(), np.abs(cosa - want_c)[1:-1].max()
    flipped = np.abs(-sina - want_s)[1:-1].max()
    print("%d x %d: |sina - get_rotang| %.3g, |cosa - get_rotang| %.3g on interior rows; with -sina %.3g" % (nx, ny, ds, dc, flipped))
    assert ds <= 1e-4 and dc <= 1e-4
    assert flipped > 0.1, "the check cannot tell the two signs apart"
    # a scalar, and a longitude a whole circle off, give the same angle
    c1, s1 = tg.rotang_at(g.proj, float(g.lon[3, 5]))
    c2, s2 = tg.rotang_at(g.proj, float(g.lon[3, 5]) + 360.0)
    assert abs(c1 - cosa[3, 5]) == 0.0 and abs(s1 - sina[3, 5]) == 0.0 and abs(c2 - c1) < 1e-14 and abs(s2 - s1) < 1e-14
    lat_lon = tg.define_target_grid_params("lat-lon", 81, 61, dx=0.25, dy=0.25, ref_lat=30.0, ref_lon=-110.0, ref_x=1.0, ref_y=1.0, stand_lon=-110.0)
    with pytest.raises(ValueError):
        tg.rotang_at(lat_lon.proj, 0.0)
