"""The K-nearest search and the extrapolation weights (mpassit_amd/csrc/knn.h) on the host: tests/c/knn_test.cpp includes the header the
kernels of k_extrapolate.hip compile, builds BVHs of n in {1, 5, 8, 9, 64, 65, 600} items and point pyramids of 5 x 3, 4 x 4, 9 x 7 and
33 x 17 points on a lattice of eighths (equal distances are equal bit for bit, exact duplicates among the items, queries that copy an
item), and checks for K in {1, 2, 3, 4, 8}, K above the number of items included, that the list equals a brute-force sort by (d2, id) and
that the stack stays within WalkCap<>::NEAREST; the weight function is checked for the coincidence rule, the order, e == 2 against
rational arithmetic on exact inputs and a sum within K eps of 1.  A stand-alone program with its own main, built with the host compiler
twice: plain, and with -fsanitize=address,undefined.  Nothing is loaded into Python and nothing is preloaded."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "knn_test.cpp")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("mode", sorted(FLAGS))
def test_knn_on_host(tmp_path, mode):
    exe = str(tmp_path / ("knn_test_" + mode))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off"] + FLAGS[mode] + [SRC, "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
    assert "weights: checked" in r.stdout
    # 7 BVHs and 4 pyramids; the printed depths lie within the printed bounds, and both tree kinds ran
    depths = re.findall(r"knn stack (\d+) of (\d+)", r.stdout)
    assert len(depths) == 11
    assert all(int(d) <= int(cap) for d, cap in depths)
    assert {int(cap) for _, cap in depths} == {46, 78}
