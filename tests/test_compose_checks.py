"""The argument checks of mpg_handle_compose and mpg_compose_weights_dev and the block plan of the composition's symbolic job on the host
(mpassit_amd/csrc/compose_checks.h): tests/c/compose_checks_test.cpp includes the header mpg_api.hip and k_compose.hip compile and calls
every check with every refusal, the accepted forms and the edges of the 64-bit and int32 ranges.  A stand-alone program built with the
host compiler under AddressSanitizer and UndefinedBehaviorSanitizer: nothing is loaded into Python.  COMPOSE_CHECKS_CXXFLAGS replaces the
flags."""
import os
import shlex
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "compose_checks_test.cpp")


def test_compose_checks_on_host(tmp_path):
    exe = str(tmp_path / "compose_checks_test")
    extra = shlex.split(os.environ.get("COMPOSE_CHECKS_CXXFLAGS", "-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all"))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + extra + [SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and not r.stderr.strip(), r.stderr
    for part in ("compose: ok", "blocks: ok", "planes: ok"):
        assert part in r.stdout


def test_the_library_compiles_the_same_text():
    api = open(os.path.join(ROOT, "mpassit_amd", "csrc", "mpg_api.hip")).read()
    assert '#include "compose_checks.h"' in api
    for fn in ("co_check_compose(", "co_check_weights("):
        assert fn in api
    kern = open(os.path.join(ROOT, "mpassit_amd", "csrc", "k_compose.hip")).read()
    assert '#include "compose_checks.h"' in kern
    for fn in ("co_next_block(", "co_check_nnz(", "CO_BLOCK_CAND"):
        assert fn in kern
    from mpassit_amd import build
    assert "compose_checks.h" in build.HEADERS
