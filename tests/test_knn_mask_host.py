"""The masked K-nearest search (mpassit_amd/csrc/knn_mask.h) and mpg_handle_mask's row rule (mpassit_amd/csrc/handle_mask.h) on the host:
tests/c/knn_mask_test.cpp includes the headers the kernels of k_extrapolate.hip and k_handle_mask.hip compile, builds BVHs of n in
{1, 5, 8, 9, 64, 65, 600} items and point pyramids of 5 x 3, 4 x 4, 9 x 7 and 33 x 17 points on a lattice of eighths, and checks under
seven masks (none, all, all but one, all but three, one whole leaf, a half-space, a random third) and K in {1, 2, 3, 4, 8} that the list
equals a brute-force sort by (d2, id) over the unmasked items, n == min(K, unmasked), no leaf body runs on a leaf without an unmasked
item, an all-masked tree makes no leaf call, the stack stays within WalkCap<>::NEAREST, and a constructed tie picks the higher id exactly
when the lower one is masked; the row rule is checked against rational arithmetic on exact inputs under both norms, for Wk <= 0 and for a
row with nothing masked.  A stand-alone program with its own main, built with the host compiler twice: plain, and with
-fsanitize=address,undefined.  Nothing is loaded into Python and nothing is preloaded."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "knn_mask_test.cpp")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("mode", sorted(FLAGS))
def test_masked_knn_and_row_rule_on_host(tmp_path, mode):
    exe = str(tmp_path / ("knn_mask_test_" + mode))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off"] + FLAGS[mode] + [SRC, "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
    assert "tie: checked" in r.stdout and "row rule: checked" in r.stdout
    # 7 BVHs and 4 pyramids; the printed depths lie within the printed bounds, and both tree kinds ran
    depths = re.findall(r"knn stack (\d+) of (\d+)", r.stdout)
    assert len(depths) == 11
    assert all(int(d) <= int(cap) for d, cap in depths)
    assert {int(cap) for _, cap in depths} == {46, 78}
    calls = re.search(r"leaf calls (\d+), of them on leaves without an unmasked item (\d+)", r.stdout)
    assert calls and int(calls.group(1)) > 1000 and int(calls.group(2)) == 0
