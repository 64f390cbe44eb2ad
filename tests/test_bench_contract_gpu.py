"""bench.py prints ONE JSON line with the fields the driver reads (metric / value / unit / n_gpus / steps / warmup /
ms_per_step / higher_is_better / scaling / vs_baseline / dtype / data / config.workload) plus the roofline object and,
with --full, the cpu_baseline one; checked here on the tiny workload so that a change to bench.py cannot silently break the contract."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_the_contract_line(gpu_lib):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "tiny", "--fields", "2", "--steps", "3", "--warmup", "1",
                        "--cpu-seconds", "1", "--full"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    rec = json.loads(lines[0])
    assert rec["metric"].startswith("interpolated 3-D fields/sec") and rec["unit"] == "fields/s" and rec["value"] > 0
    assert rec["n_gpus"] == 1 and rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
    assert rec["higher_is_better"] is True and rec["scaling"] in ("weak", "strong") and rec["vs_baseline"] is None
    assert rec["dtype"] == "f64" and rec["data"] == "synthetic" and "tiny" in rec["config"]["workload"] and "model" not in rec["config"]
    assert abs(rec["value"] - 2 * 3 / (rec["ms_per_step"] * 3e-3)) < 1e-6 * rec["value"]          # fields * steps / time
    ro = rec["roofline"]
    assert ro["bound"] == "hbm" and ro["unit"] == "GB/s" and ro["peak"] == 8000.0 and ro["achieved"] > 0
    assert abs(ro["frac"] - ro["achieved"] / ro["peak"]) < 1e-12 and (ro["traffic"] is None or ro["traffic"] > 0)
    cb = rec["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "fields/s" and cb["value"] > 0 and cb["cores"] >= 1 and isinstance(cb["sample"], str)


def test_plain_run_is_lean_and_dumps_the_last_step(gpu_lib, tmp_path):
    """A plain run (no --full) times the headline and nothing else: the same contract fields, no CPU baseline, no extra legs, no
    device-copy rates; --dump-outputs writes the last timed step's results, and the same arguments give the same bits twice."""
    F, steps = 2, 4
    got = []
    for run in ("a", "b"):
        d = tmp_path / run
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "tiny", "--fields", str(F), "--steps", str(steps),
                            "--warmup", "1", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, lines
        rec = json.loads(lines[0])
        assert rec["steps"] == steps and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["dtype"] == "f64" and rec["higher_is_better"] is True
        assert abs(rec["value"] - F * steps / (rec["ms_per_step"] * steps * 1e-3)) < 1e-6 * rec["value"]
        assert rec["cpu_baseline"] is None and rec["store"] is None and rec["job"] is None and rec["production_path"] is None
        assert rec["roofline"]["device_copy_GBs"] is None and rec["roofline"]["kernel_ms"] > 0
        assert sorted(os.listdir(d)) == ["out.npy"]
        out = np.load(d / "out.npy")
        assert out.dtype == np.float64 and out.shape[:2] == (F, rec["config"]["nlev"]) and out.shape[2] * out.shape[3] == rec["config"]["target_points"]
        assert np.isfinite(out).all() and np.abs(out).max() > 0
        got.append(out)
    assert np.array_equal(got[0], got[1])


def test_bench_gpus2_launches_itself(gpu_lib):
    """`python bench.py --gpus 2` with no torch.distributed.run around it starts its own two ranks (a child job, the
    parent never touches the GPU) and rank 0 prints the line; on the one-GPU box the ranks share the card and the halo
    travels over gloo (MPASSIT_DIST_BACKEND=gloo), on the 8-GPU node the same flow runs over RCCL.  The headline
    workload itself (C4, strong scaling: the same global problem split by target rows)."""
    env = dict(os.environ, MPASSIT_DIST_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["steps"] == 3 and rec["scaling"] == "strong" and rec["value"] > 0
    assert "c4_3m_regional" in rec["config"]["workload"] and rec["config"]["parallelism"].startswith("rows2+halo")
    h = rec["halo"]
    assert h["ranks_in_group"] == 2 and h["mode"] == "range" and len(h["per_rank"]) == 2
    assert sum(p["rows"] for p in h["per_rank"]) == 1060
    # aligned ownership: only the strips straddling the row-block boundary travel -- a few lattice rows of 13 x 55 values
    assert 0 < h["halo_bytes_per_step"] < 200e6 and h["exchange_ms_max"] > 0
    # round 6: the line names every transport of the run; on a multi-GPU node the C-ABI leg supplies `value` and the torch leg is the
    # comparison; in this rehearsal (gloo, ranks sharing the card) the C-ABI leg is skipped and says why
    tr = h["transports"]
    assert h["value_transport"] == "torch" and tr["torch"]["ms_per_step"] > 0 and tr["torch"]["ranks_in_group"] == 2
    assert abs(tr["torch"]["ms_per_step"] - rec["ms_per_step"]) < 1e-9 and "skipped" in tr["cabi"]


def test_bench_failing_cabi_leg_is_reported_and_ends_nonzero(gpu_lib):
    """MPASSIT_BENCH_TRANSPORT=both forced on the one-card rehearsal: RCCL refuses the second rank on the device, so the C-ABI leg
    (mpg_comm_init) FAILS for real.  The line must still come -- the torch leg's numbers, the error under halo.transports.cabi --
    and the run must end non-zero; nothing is re-executed."""
    env = dict(os.environ, MPASSIT_DIST_BACKEND="gloo", MPASSIT_BENCH_FORCE_CABI_LEG="1", MPG_COMM_TIMEOUT_S="30")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "tiny", "--steps", "2", "--warmup", "1", "--full"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:] + r.stderr[-2000:]
    rec = json.loads(lines[0])
    tr = rec["halo"]["transports"]
    assert r.returncode != 0, "a failed transport leg must fail the run"
    assert "error" in tr["cabi"] and tr["torch"]["ms_per_step"] > 0 and rec["halo"]["value_transport"] == "torch" and rec["value"] > 0


@pytest.mark.parametrize("workload,ranks,mode", [("tiny", 3, "range"), ("c5_small", 2, "owned")])
def test_bench_sharded_on_float32_file_order_sources(gpu_lib, workload, ranks, mode):
    """Round 5: `--gpus N --io f32 --layout lev_fast` -- the sources as the shipped driver holds them (float32, MPAS file order,
    input_data.F90:630-655) sharded over N ranks; the halo exchange moves whole [nlev] rows of that type.  BASELINE configs[4] is
    runnable at N > 1 as written (here its small sibling, a Morton-numbered global mesh: the owned halo form -- every cell to the lowest rank that references it --, and a banded regional
    mesh: the range form); the ranks share the one card and the halo travels over gloo."""
    env = dict(os.environ, MPASSIT_DIST_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(ranks), "--workload", workload, "--io", "f32", "--layout", "lev_fast",
                        "--fields", "3", "--steps", "3", "--warmup", "1"], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == ranks and rec["value"] > 0 and rec["config"]["src_layout"] == "lev_fast" and rec["config"]["io_dtype"].startswith("f32")
    h = rec["halo"]
    assert h["mode"] == mode and len(h["per_rank"]) == ranks and h["halo_bytes_per_step"] > 0
    nlev = rec["config"]["nlev"]
    assert all(p["received"] % (nlev * 4) == 0 for p in h["per_rank"])          # whole float32 rows travel


def test_default_line_carries_the_production_numbers_inside_roofline(gpu_lib):
    """The driver's record keeps the SCALARS of `roofline` (a nested object inside it was dropped in round 4), cuts keys at 40
    characters and strings at 120: what the shipped driver's paths measure rides there as flat scalars with short keys -- the
    float32 file-order Regrid, the whole job (cold = FIRST-IN-PROCESS, from a fresh child process; warm fraction of the HBM
    peak), the Stores' first-in-process sum, mpg_init of the fresh children, the counted : algorithmic traffic ratio.  The full
    objects stay at the top level.  The --full command on the headline workload, a short CPU leg."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--cpu-seconds", "1", "--full"],
                       capture_output=True, text=True, timeout=1100, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines                                 # ONE line, whatever the child legs printed
    rec = json.loads(lines[0])
    ro = rec["roofline"]
    for k, v in ro.items():                                       # nothing the driver's flattening would drop or cut
        assert len(k) <= 40 and not isinstance(v, (dict, list)), k
        assert not isinstance(v, str) or len(v) <= 120, (k, v)
    assert set(ro) >= {"f32_lev_fast_frac", "f32_lev_fast_ms", "job_cold_first_ms", "job_warm_frac", "store_first_ms_sum", "traffic_ratio",
                       "job_mpg_init_ms", "store_mpg_init_ms", "device_copy_GBs", "device_add_2r1w_GBs", "device_fill_GBs"}
    assert all(3000 < ro[k] < 8000 for k in ("device_copy_GBs", "device_add_2r1w_GBs", "device_fill_GBs")) and ro["device_fill_GBs"] > ro["device_copy_GBs"]
    assert 0.3 < ro["f32_lev_fast_frac"] < 1.0 and ro["f32_lev_fast_ms"] > 0 and 1.0 <= ro["traffic_ratio"] < 2.0
    assert all(len(k) <= 40 for k in rec["config"]) and rec["config"]["bundle_ends_equal_single"] is True
    assert len(rec["cpu_baseline"]["sample"]) <= 120
    job = rec["job"]
    assert set(job) >= {"cold_first_ms", "cold_ms", "warm_ms", "alg_bytes_warm", "frac_warm", "geometry_first_ms", "mpg_init_ms"}
    assert job["cold_first_ms"] >= job["cold_ms"] > job["warm_ms"] > 0 and 0.1 < job["frac_warm"] < 1.0
    assert abs(job["frac_warm"] - job["alg_bytes_warm"] / (job["warm_ms"] * 1e-3) / 1e9 / 8000.0) < 2e-4
    assert ro["job_cold_first_ms"] == job["cold_first_ms"] and ro["job_warm_frac"] == job["frac_warm"]
    st = {k: v for k, v in rec["store"].items() if isinstance(v, dict)}
    assert set(st) == {"bilinear", "nearest", "conserve"}
    for v in st.values():
        assert v["ms_first"] >= v["ms"] > 0
    assert abs(ro["store_first_ms_sum"] - sum(v["ms_first"] for v in st.values())) < 2e-3
    # the single-shot costs (code objects loaded by mpg_init's helper thread): first-in-process Stores within reach of the warm ones
    assert st["nearest"]["ms_first"] < 5.0 and st["conserve"]["ms_first"] < 7.0, st
    assert len(lines[0]) < 8000                                   # short enough that no evidence hangs on a cut-off tail
