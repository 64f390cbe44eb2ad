"""The handle cache and the Store worker's queue (mpassit_amd/csrc/store_cache.h) on the host: tests/c/store_cache_test.cpp includes the
header mpg_api.hip compiles and runs it with a stub handle and a build it holds at a latch.  Keys: every key the eight Store entry points
can make, under every setting of the knobs that enter one, is equal to another exactly when the packed tuples the library used before were
equal.  Cache: insert-if-absent never replaces, the parked handle released longest ago is the one evicted, held ones never, purge by object
in either place, detach.  Queue: one build per key whoever asks, nothing cached after a failed build, stop drains first; every handle made
is freed.  A stand-alone program built with the host compiler: nothing is loaded into Python.  STORE_CACHE_TEST_CXXFLAGS adds flags, e.g.
"-O1 -g -fsanitize=thread" for a ThreadSanitizer run on the host."""
import os
import re
import shlex
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "store_cache_test.cpp")


def test_store_cache_on_host(tmp_path):
    exe = str(tmp_path / "store_cache_test")
    extra = shlex.split(os.environ.get("STORE_CACHE_TEST_CXXFLAGS", "-O2"))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-pthread"] + extra + [SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
    for part in ("keys:", "cache: ok", "queue: ok"):
        assert part in r.stdout
    made, freed = map(int, re.search(r"handles made (\d+) freed (\d+)", r.stdout).groups())
    assert made == freed > 0
