"""The nearest-destination-to-source search and its value rule (mpassit_amd/csrc/dtos.h) on the host: tests/c/dtos_test.cpp includes the
header the kernels of k_store_dtos.hip compile, builds BVHs of n in {1, 8, 9, 65, 600} items and point pyramids of 4 x 4, 5 x 3 and
33 x 17 points on a lattice of eighths (equal distances are equal bit for bit, exact duplicates among the items), asks with random
points, copies of an item and points equidistant from two items, under no mask and under masks that leave all, one, a random part or
none of the items alive, and checks that the answer is the brute-force minimum of (d2, id) -- -1 when nothing is alive --, that the
walk's stack stays within WalkCap<>::NEAREST, that a constructed tie goes to the lower id, and that the mean rule gives the rounded
1.0 / n for n = 1 .. 600.  A stand-alone program with its own main, built with the host compiler twice: plain, and with
-fsanitize=address,undefined.  Nothing is loaded into Python and nothing is preloaded."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "dtos_test.cpp")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("mode", sorted(FLAGS))
def test_dtos_on_host(tmp_path, mode):
    exe = str(tmp_path / ("dtos_test_" + mode))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off"] + FLAGS[mode] + [SRC, "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
    assert "tie: checked" in r.stdout and "values: checked" in r.stdout
    # 5 BVHs and 3 pyramids; the printed depths lie within the printed bounds, and both tree kinds ran
    depths = re.findall(r"dtos stack (\d+) of (\d+)", r.stdout)
    assert len(depths) == 8
    assert all(int(d) <= int(cap) for d, cap in depths)
    assert {int(cap) for _, cap in depths} == {46, 78}
