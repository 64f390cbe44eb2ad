"""The Stores' two tree walks (mpassit_amd/csrc/tree_walk.h) on the host: tests/c/tree_walk_test.cpp includes the header the kernels
compile, builds pyramids and BVHs of the sizes at which the levels, the ragged last row / column and the last partial group change, and
checks that an accept-everything filter walk reaches every leaf exactly once, that the best-first walk returns the brute-force nearest
item (ties to the lowest id, exact duplicates among the items) and that neither stack ever holds more than the bound the header derives.
A stand-alone program built with the host compiler: nothing is loaded into Python.  TREE_WALK_TEST_CXXFLAGS adds flags, e.g.
"-O1 -g -fsanitize=address,undefined" for a host sanitizer run."""
import os
import re
import shlex
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "tree_walk_test.cpp")


def test_walks_on_host(tmp_path):
    exe = str(tmp_path / "tree_walk_test")
    extra = shlex.split(os.environ.get("TREE_WALK_TEST_CXXFLAGS", "-O2"))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off"] + extra + [SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
    # 6 pyramids and 5 BVHs, each with its filter and its nearest line; the printed depths lie within the printed bounds
    depths = re.findall(r"(filter|nearest) stack (\d+) of (\d+)", r.stdout)
    assert len(depths) == 22
    assert all(int(d) <= int(cap) for _, d, cap in depths)
    assert {int(cap) for _, _, cap in depths} == {45, 46, 77, 78}
