"""Pitched destinations, the parts that need no GPU: the level-stride arithmetic (mpg_dst_level_stride works before mpg_init), the
header's new calls, and a C99 program that calls them (tests/c/pitch_smoke.c) compiling with gcc -pedantic -Werror."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "pitch_smoke.c")
NEW_CALLS = ["mpg_dst_level_stride", "mpg_regrid_pitched_dev", "mpg_regrid_typed_pitched_dev", "mpg_regrid_bundle_typed_pitched_dev",
             "mpg_wind_destagger_pitched_dev", "mpg_dev_to_file_planes"]


def _stride(points, dst_type):
    from mpassit_amd import _lib
    ld = C.c_int64(-1)
    rc = _lib.load().mpg_dst_level_stride(C.c_int64(points), C.c_int(dst_type), C.byref(ld))
    return rc, ld.value


@pytest.mark.parametrize("dst_type", [0, 1, 2, 3])
def test_level_stride_of_the_reference_grid(dst_type):
    # 1799 x 1059 mass points (the reference's namelist nx = 1800, ny = 1060): both element sizes round up to the same 128-byte line
    assert _stride(1799 * 1059, dst_type) == (0, 1905152)


@pytest.mark.parametrize("points,f32,want", [(1800 * 1060, 1, 1800 * 1060), (1800 * 1060, 0, 1800 * 1060), (32, 1, 32), (16, 0, 16),
                                             (1, 1, 32), (1, 0, 16), (17, 0, 32), (19080, 1, 19104), (19080, 0, 19088)])
def test_level_stride_rounds_to_whole_lines(points, f32, want):
    rc, ld = _stride(points, f32)
    assert rc == 0 and ld == want and ld >= points and (ld * (4 if f32 else 8)) % 128 == 0


def test_level_stride_refuses_bad_arguments():
    from mpassit_amd import _lib
    L = _lib.load()
    assert _stride(0, 0)[0] == _lib.MPG_ERR_INVALID_ARG
    assert _stride(-5, 1)[0] == _lib.MPG_ERR_INVALID_ARG
    assert _stride(100, 7)[0] == _lib.MPG_ERR_INVALID_ARG
    assert L.mpg_dst_level_stride(C.c_int64(100), C.c_int(0), None) == _lib.MPG_ERR_INVALID_ARG


def test_header_declares_the_pitched_calls():
    from mpassit_amd import _lib
    txt = open(os.path.join(ROOT, "include", "mpassit_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW_CALLS:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert m, name
        assert len(m.group(1).split(",")) <= 14, name
        assert name in _lib.SYMBOLS
    # each documented next to its dense twin
    for dense, pitched in (("mpg_regrid_dev", "mpg_regrid_pitched_dev"), ("mpg_regrid_typed_dev", "mpg_regrid_typed_pitched_dev"),
                           ("mpg_regrid_bundle_typed_dev", "mpg_regrid_bundle_typed_pitched_dev"),
                           ("mpg_wind_destagger_dev", "mpg_wind_destagger_pitched_dev"), ("mpg_dev_to_file", "mpg_dev_to_file_planes")):
        a, b = code.index("int %s(" % dense), code.index("int %s(" % pitched)
        assert 0 < b - a < 2000, (dense, pitched)


def test_c99_program_calling_the_pitched_calls_compiles_and_runs(tmp_path):
    from mpassit_amd import build
    build.build()
    exe = str(tmp_path / "pitch_smoke")
    lib = os.path.join(ROOT, "mpassit_amd")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L" + lib, "-lmpassit_amd", "-lm", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe, str(tmp_path / "planes.bin")], capture_output=True, text=True, timeout=120)
    assert "stride arithmetic ok" in r.stdout, r.stdout + r.stderr
    try:
        import torch
        gpu = torch.cuda.is_available()
    except Exception:
        gpu = False
    if gpu:
        assert r.returncode == 0 and "pitch_smoke ok" in r.stdout, r.stdout + r.stderr
    else:   # no GPU: the arithmetic ran, then mpg_init refused (no CPU fallback)
        assert r.returncode != 0 and "no CPU fallback" in r.stderr


def test_wind_destagger_refuses_outs_for_host_arrays():
    """outs= names device tensors to write into; the host-array chain allocates its results, so it must not ignore them silently"""
    import numpy as np
    from mpassit_amd import regrid as R
    um = np.zeros((2, 3, 4))
    with pytest.raises(ValueError):
        R.wind_destagger(None, None, None, None, um, um, 2, outs=(np.zeros((2, 3, 5)), np.zeros((2, 4, 4))))
