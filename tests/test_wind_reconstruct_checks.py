"""The argument checks of mpg_reconstruct_store, mpg_reconstruct_weights_dev and mpg_wind_reconstruct_dev on the host
(mpassit_amd/csrc/wind_reconstruct_checks.h): tests/c/wind_reconstruct_checks_test.cpp includes the header mpg_api.hip compiles and calls
every check with every refusal, the accepted forms and the edges of the 64-bit range.  A stand-alone program built with the host compiler
under AddressSanitizer and UndefinedBehaviorSanitizer: nothing is loaded into Python.  WIND_RECONSTRUCT_CHECKS_CXXFLAGS replaces the flags."""
import os
import shlex
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "wind_reconstruct_checks_test.cpp")


def test_wind_reconstruct_checks_on_host(tmp_path):
    exe = str(tmp_path / "wind_reconstruct_checks_test")
    extra = shlex.split(os.environ.get("WIND_RECONSTRUCT_CHECKS_CXXFLAGS", "-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all"))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + extra + [SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and not r.stderr.strip(), r.stderr
    for part in ("store: ok", "values: ok", "apply: ok", "lds: ok"):
        assert part in r.stdout


def test_the_api_compiles_the_same_text():
    api = open(os.path.join(ROOT, "mpassit_amd", "csrc", "mpg_api.hip")).read()
    assert '#include "wind_reconstruct_checks.h"' in api
    for fn in ("wr_check_store(", "wr_check_weights(", "wr_check_apply("):
        assert fn in api
    kern = open(os.path.join(ROOT, "mpassit_amd", "csrc", "k_wind_reconstruct.hip")).read()
    assert '#include "wind_reconstruct_checks.h"' in kern and "wr_lds_head(nout)" in kern
    from mpassit_amd import build
    assert "wind_reconstruct_checks.h" in build.HEADERS
