"""CPU checks of the Mesh -> Mesh boundary: the header declares mpg_regrid_store_mesh and mpg_regrid_rows_dev with their exact argument
lists and states the rules, _lib lists and binds both, the built library exports them, the Python wrappers have the agreed signatures
and refuse bad arguments before any device call, the Fortran module has matching bind(C) interfaces -- and the inputs of the GPU test
(tests/_mesh_to_mesh_cases.py) are qualified against the oracle alone: no pair puts more than the tie cap of its mapped points on
a triangle edge."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _mesh_to_mesh_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORE, APPLY = "mpg_regrid_store_mesh", "mpg_regrid_rows_dev"
STORE_ARGS = ["mpg_mesh src", "int src_meshloc", "mpg_mesh dst", "int dst_meshloc", "int regridmethod", "mpg_handle *out"]
APPLY_ARGS = ["mpg_handle rh", "const void *src_dev", "int src_type", "int nlev", "int nfields", "void *dst_dev", "int dst_type", "double scale",
              "double offset", "void *hip_stream"]


def _header(strip_comments=True):
    txt = open(os.path.join(ROOT, "include", "mpassit_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S) if strip_comments else txt


def _doc(name, start):
    txt = _header(strip_comments=False)
    i = txt.index("int " + name + "(")
    doc = " ".join(txt[max(0, i - 9000):i].split())
    return doc[doc.rindex(start):]


def test_header_declares_both_calls():
    txt = _header()
    for name, want in ((STORE, STORE_ARGS), (APPLY, APPLY_ARGS)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, name + " is not declared"
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want


def test_header_states_the_rules():
    doc = _doc(STORE, "Mesh -> Mesh: ESMF_FieldRegridStore")
    for phrase in ("lowest triangle id", "stored order", "dA / S", "idx -1", "bilinear_linetype", "depends on the two meshes and the knob only",
                   "lowest cell id on ties", "MPG_ERR_UNSUPPORTED: MPG_REGRIDMETHOD_CONSERVE", "src_meshloc = MPG_MESHLOC_NODE",
                   "mpg_mesh_create_window", "MPG_ERR_OVERFLOW", "MPG_ERR_INVALID_ARG", "src == dst is allowed", "EITHER mesh is destroyed",
                   "mpg_mesh_set_source_window on the SOURCE mesh", "no _begin variant", "nnz_per_row 3 (bilinear) or 1 (nearest)",
                   "ny_dst = 1", "mpg_regrid_rows_dev"):
        assert phrase in doc, phrase
    doc = _doc(APPLY, "Regrid from rows to rows")
    for phrase in ("[cell][lev] in and [cell][lev] out", "1, 3 or 4 slots", "no pole caps", "(dst type) fma(0.0, scale, offset)",
                   "MPG_ERR_UNSUPPORTED: MPG_TYPE_BE; CSR handles", "pole caps", "nlev < 1", "Contract by identity, no tolerance",
                   "element [p][k] has the bits of element [k][p]", "MPG_LAYOUT_LEV_FAST", "mpg_regrid_typed_dev", "nfields batching", "No atomics",
                   "allocates nothing and synchronises nothing", "hipGraph"):
        assert phrase in doc, phrase


def test_lib_lists_binds_and_exports_them():
    from mpassit_amd import _lib, build
    assert STORE in _lib.SYMBOLS and APPLY in _lib.SYMBOLS
    build.build()
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    for name in (STORE, APPLY):
        assert hasattr(lib, name)
        assert re.search(r" T %s\b" % name, out)
    assert len(_lib._STORE_MESH_PROTO._argtypes_) == 6 and _lib._STORE_MESH_PROTO._restype_ is C.c_int
    at = _lib._ROWS_PROTO._argtypes_
    assert len(at) == 10 and _lib._ROWS_PROTO._restype_ is C.c_int
    assert at[3] is C.c_int and at[7] is C.c_double and at[8] is C.c_double and at[9] is C.c_void_p
    assert callable(_lib.regrid_store_mesh) and callable(_lib.regrid_rows_dev)


def test_python_signatures():
    from mpassit_amd import regrid as R
    sig = inspect.signature(R.regrid_store_mesh)
    assert list(sig.parameters) == ["src_mesh", "dst_mesh", "regridmethod", "src_meshloc", "dst_meshloc"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["regridmethod"], d["src_meshloc"], d["dst_meshloc"]) == (R.REGRIDMETHOD_BILINEAR, R.MESHLOC_ELEMENT, R.MESHLOC_ELEMENT)
    sig = inspect.signature(R.RouteHandle.regrid_rows)
    assert list(sig.parameters) == ["self", "src", "nlev", "nfields", "out_dtype", "scale", "offset", "out"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["nlev"], d["nfields"], d["out_dtype"], d["scale"], d["offset"], d["out"]) == (1, 1, None, 1.0, 0.0, None)
    sig = inspect.signature(R.regrid_rows_autograd)
    assert list(sig.parameters) == ["rh", "src", "nlev", "nfields"]
    assert "regrid_store_mesh" in R.__all__ and "regrid_rows_autograd" in R.__all__


def test_wrappers_reject_bad_arguments_before_any_device_call():
    """No GPU, no mpg_init: every one of these must fail in Python, with a message of its own (a call that reached the library would
    raise MpgError 'mpg_init has not been called')."""
    import torch
    from mpassit_amd import regrid as R

    class NotAMesh:
        _h = None

    fake = R.Mesh.__new__(R.Mesh)             # a Mesh object without a device mesh behind it
    fake._h = C.c_void_p()
    with pytest.raises(TypeError, match="Mesh objects"):
        R.regrid_store_mesh(NotAMesh(), fake)
    with pytest.raises(TypeError, match="Mesh objects"):
        R.regrid_store_mesh(fake, None)
    with pytest.raises(ValueError, match="regridmethod"):
        R.regrid_store_mesh(fake, fake, regridmethod=7)
    with pytest.raises(ValueError, match="mesh location"):
        R.regrid_store_mesh(fake, fake, src_meshloc=2)
    with pytest.raises(ValueError, match="mesh location"):
        R.regrid_store_mesh(fake, fake, dst_meshloc=-1)
    rh = R.RouteHandle.__new__(R.RouteHandle)  # a handle's bookkeeping without a device handle behind it
    rh._h, rh.n_src, rh.n_dst, rh.nx_dst, rh.ny_dst, rh.nnz_per_row = C.c_void_p(), 10, 7, 7, 1, 3
    with pytest.raises(ValueError, match="CUDA tensor"):
        rh.regrid_rows(np.zeros((10, 2)), nlev=2)
    with pytest.raises(ValueError, match="CUDA tensor"):
        rh.regrid_rows(torch.zeros((10, 2), dtype=torch.float64), nlev=2)


def test_fortran_binds_them():
    src = open(os.path.join(ROOT, "mpassit_amd", "fortran", "mpg_mod.F90")).read()

    def interface(name):
        m = re.search(r"function\s+%s\s*\(([^)]*)\)\s*&?\s*bind\s*\(\s*C\s*,\s*name\s*=\s*['\"]%s['\"]\s*\)(.*?)end\s+function" % (name, name),
                      src, flags=re.S | re.I)
        assert m, name + " has no bind(C) interface in mpg_mod.F90"
        return [a.strip().lower() for a in m.group(1).replace("&", " ").split(",")], m.group(2).lower()

    args, body = interface(STORE)
    assert args == ["src", "src_meshloc", "dst", "dst_meshloc", "regridmethod", "rh"]
    for a in ("src_meshloc", "dst_meshloc", "regridmethod"):
        assert re.search(r"integer\(c_int\),\s*value\s*::.*\b%s\b" % a, body), a
    for a in ("src", "dst"):
        assert re.search(r"type\(c_ptr\),\s*value\s*::.*\b%s\b" % a, body), a
    assert re.search(r"type\(c_ptr\),\s*intent\(out\)\s*::\s*rh\b", body)
    args, body = interface(APPLY)
    assert args == ["rh", "src_dev", "src_type", "nlev", "nfields", "dst_dev", "dst_type", "scale", "offset", "hip_stream"]
    for a in ("src_type", "nlev", "nfields", "dst_type"):
        assert re.search(r"integer\(c_int\),\s*value\s*::.*\b%s\b" % a, body), a
    assert re.search(r"real\(c_double\),\s*value\s*::.*\bscale\b.*\boffset\b", body)
    for a in ("rh", "src_dev", "dst_dev", "hip_stream"):
        assert re.search(r"type\(c_ptr\),\s*value\s*::.*\b%s\b" % a, body), a


def test_kernel_sources_are_built_and_anchored():
    from mpassit_amd import build
    assert "k_store_mesh.hip" in build.SOURCES and "k_apply_rows.hip" in build.SOURCES
    api = open(os.path.join(ROOT, "mpassit_amd", "csrc", "mpg_api.hip")).read()
    assert "X(k_store_mesh)" in api and "X(k_apply_rows)" in api
    store = open(os.path.join(ROOT, "mpassit_amd", "csrc", "k_store_mesh.hip")).read()
    assert "#pragma clang fp contract(off)" in store, "geometry translation units are compiled without floating-point contraction"
    rows = open(os.path.join(ROOT, "mpassit_amd", "csrc", "k_apply_rows.hip")).read()
    assert "atomic" not in rows.split("#include")[-1], "the rows Regrid uses no atomics"
    assert '#include "apply_mesh.h"' in rows and "apply_mesh.h" in build.HEADERS
    shared = open(os.path.join(ROOT, "mpassit_amd", "csrc", "apply_mesh.h")).read()
    assert "atomic" not in shared.split("#include")[-1], "nor do the helpers it shares with the other mesh-order kernels"
    assert "xcd_remap" in rows and "wsum_fixed" in rows and "stream_store_lane" in rows


# ---- the GPU test's inputs, qualified by the oracle alone ------------------------------------------------------------------------------
@pytest.mark.parametrize("linetype", [0, 1])
@pytest.mark.parametrize("name", MC.PAIR_NAMES)
def test_inputs_stay_inside_the_tie_cap(oracle, name, linetype):
    idx, w, pts, cx = MC.oracle_bilinear(oracle, name, linetype)
    mapped = idx[:, 0] >= 0
    share = MC.edge_share(idx, w)
    print("%s linetype %d: %d points, %d mapped, share within %.0e of an edge %.3g" % (name, linetype, pts.shape[0], int(mapped.sum()), MC.TIE_TOL, share))
    assert share <= MC.TIE_CAP, "the synthetic pair itself sits on triangle edges: change the seeds"
    assert mapped.any()
    assert np.abs(w[mapped].sum(axis=1) - 1.0).max() < 1e-12 and (w[~mapped] == 0.0).all()
    src, dst, loc = MC.pair(name)
    n = dst.nCells if loc == 0 else dst.nVertices
    assert pts.shape[0] == n and n % 64 != 0, "the last block of the rows Regrid is a partial one"
    # the ray from the centre tiles the sphere; dropped along each flat triangle's own normal, the triangles leave thin wedges
    # between them (their normals differ), so a few points of a global pair fall into none: that is the line type, not a rim
    covered = mapped.all() if linetype == 0 else mapped.mean() > 0.98
    if name in ("geo10_to_vor1500", "geo10_to_vor1500_nodes", "varres3000_to_geo8"):
        assert covered, "global -> global: nothing is unmapped"
    if name == "vor2500_to_hex":
        assert covered, "the limited-area mesh lies inside the global one"
        assert np.unique(idx[mapped]).size < 0.2 * src.nCells, "boundary conditions: a small part of the globe feeds the region"
    if name == "hex_to_geo10":
        assert 10 <= mapped.sum() < 0.5 * n, "most of the globe is outside the regional source"
        # the rim strip: points nearer to a rim cell centre than any rim cell is wide, and yet in no triangle
        near = oracle.nearest(cx, pts, brute=True)
        d = np.linalg.norm(pts - cx[near], axis=1)
        spacing = np.linalg.norm(cx[1] - cx[0])
        assert ((~mapped) & (d < 5.0 * spacing)).any(), "some unmapped points lie right next to the source mesh"


def test_identity_pair_is_the_all_ties_case(oracle):
    """src == dst: every point sits on a corner of its triangles; the oracle maps every point with one weight 1 on its own cell."""
    m = MC.mesh("geo8")
    cx = MC.cell_xyz(oracle, m)
    tri, _ = oracle.dual_triangles(m.verticesOnCell, m.nVertices, cx)
    idx, w = oracle.bilinear_weights(cx, tri, cx, 0)
    assert (idx[:, 0] >= 0).all()
    own = idx == np.arange(m.nCells)[:, None]
    assert (own.sum(axis=1) == 1).all() and (w[own] == 1.0).all() and (w[~own] == 0.0).all()
    assert MC.edge_share(idx, w) == 1.0
