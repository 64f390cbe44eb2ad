"""The creep arithmetic (mpassit_amd/csrc/creep.h) on the host: tests/c/creep_test.cpp includes the header the kernels of k_creep.hip
compile and checks the grid neighbourhoods on 1 x 1, 1 x 5, 2 x 2 and 3 x 3 (corner, edge, centre; no shifted window at a border), the
mesh neighbourhoods through PtSrc::ring1 of a hexagon centre, of a rim cell with an invalid triangle and of a bare cell, the level
predicate, and the ordered merge-and-divide with duplicate columns and m = 1, 2, 8 on dyadic values, where the expected row is exact --
through cr_merge_row and through the device's own route (a stable sort, cr_sum_div per run), bit for bit the same.  A stand-alone program
with its own main, built with the host compiler twice: plain, and with -fsanitize=address,undefined.  Nothing is loaded into Python and
nothing is preloaded."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "creep_test.cpp")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("mode", sorted(FLAGS))
def test_creep_on_host(tmp_path, mode):
    exe = str(tmp_path / ("creep_test_" + mode))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off"] + FLAGS[mode] + [SRC, "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and "FAIL" not in r.stdout
    for part in ("grid", "mesh", "levels", "merge"):
        assert part + ": checked" in r.stdout
