"""The patch arithmetic (mpassit_amd/csrc/patch.h) on the host: tests/c/patch_test.cpp includes the header the kernels of k_patch.hip
compile and checks, on exact lattice inputs against rational arithmetic (__int128 fractions on the integer lattice), the shape values of
every rung of the attempt ladder -- a 3 x 3 block from its centre and from its border (A), a 2 x 3, a 5 x 2 and a 2 x 2 block and five
points of an open fan (C: six points of rank 5 must fall through), three collinear points, two points, a triangle with a missing cell and
a coincident patch with h = 0 (D), a valence-4 cell whose ring 2 is the 3 x 3 block (B), a hexagon with its centre, an exactly determined
pentagon with its centre (L at a node is that node's unit vector within 1e-12), a patch of 33 points (D) -- each with the shape values
summing to 1 within 64 eps, and the ordered merge with duplicate ids across slots, with all 3 * 32 candidates and at its cap.  A
stand-alone program with its own main, built with the host compiler twice: plain, and with -fsanitize=address,undefined.  Nothing is
loaded into Python and nothing is preloaded."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "patch_test.cpp")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("mode", sorted(FLAGS))
def test_patch_on_host(tmp_path, mode):
    exe = str(tmp_path / ("patch_test_" + mode))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off"] + FLAGS[mode] + [SRC, "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and "FAIL" not in r.stdout
    assert "frame: checked" in r.stdout and "merge: checked" in r.stdout
    got = dict(re.findall(r"^([^:\n]+): attempt ([ABCD])", r.stdout, flags=re.M))
    assert got == {"3x3 centre": "A", "3x3 corner": "A", "5x4 border": "A", "5x4 inner": "A", "2x3 block": "C", "5x2 block": "C",
                   "2x2 block": "C", "five points": "C", "three collinear": "D", "two points": "D", "invalid triangle": "D",
                   "coincident": "D", "valence 4": "B", "hexagon": "A", "hexagon at a node": "A", "pentagon": "A", "33 points": "D"}
    worst = [float(x) for x in re.findall(r"worst \|L - [a-z ]+\| ([0-9.e+-]+)", r.stdout)]
    assert len(worst) == 12 and max(worst) <= 1e-12
