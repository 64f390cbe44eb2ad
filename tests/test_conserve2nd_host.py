"""The second-order conservative arithmetic (mpassit_amd/csrc/conserve2nd.h) on the host: tests/c/conserve2nd_test.cpp includes the header
the kernels of k_conserve2nd.hip compile and checks, on exact inputs, the triangle area (the octant, a sweep of sizes against 2 atan2 in
long double, an excess beyond pi), the moment of a triangle and of a square split along either diagonal (and its clockwise twin), the
stencil solve on a symmetric cross (b known in closed form), collinear neighbours, one neighbour and zero neighbours (fail: first order),
sum b = 0 and sum b d^T = I on an irregular stencil, a near-collinear stencil on either side of the 2^-26 rule, the offsets and t.  A
stand-alone program with its own main, built with the host compiler twice: plain, and with -fsanitize=address,undefined.  Nothing is
loaded into Python and nothing is preloaded."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "conserve2nd_test.cpp")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("mode", sorted(FLAGS))
def test_conserve2nd_on_host(tmp_path, mode):
    exe = str(tmp_path / ("conserve2nd_test_" + mode))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off"] + FLAGS[mode] + [SRC, "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and "FAIL" not in r.stdout
    for line in ("moment: checked", "cross: pass", "collinear: fail", "one neighbour: fail", "zero neighbours: fail", "irregular: pass, sum b = 0",
                 "near-collinear 2^-12: pass", "near-collinear 2^-13: fail", "offsets: checked"):
        assert line in r.stdout, line
