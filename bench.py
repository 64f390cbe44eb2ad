#!/usr/bin/env python3
"""Headline benchmark: interpolated 3-D fields/s (nCells x nLev -> nx x ny) on MI355X.

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
  (N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...)

A "step" = one Regrid (ESMF_FieldBundleRegrid, interp.F90:251) of a bundle of F 3-D fields through a
cached bilinear route handle, inputs and outputs resident in HBM.  Workload at every N: BASELINE.json's
headline configuration, the 3.0 M-cell x 55-level regional mesh -> 1801x1061 Lambert grid (it fits one
GPU); for N > 1 the same global problem is split by target rows with a source halo exchange over
RCCL (strong scaling).  RegridStore (weight generation) is timed once and reported separately
(`store_ms`): weights are data, built once per (mesh, grid) and reused for every field and time.

Prints ONE JSON line on rank 0 (see the task contract).  A plain run sets up, warms up, times the K steps,
writes the last step's results if --dump-outputs is given, and prints the line.  --full adds everything
else: the in-bench self-checks, the live device-copy rates, the CPU baseline, the other paths, sizes and
numberings (`production_path`, `cell_numbering`, `end_to_end_pcie`), the fresh-process `store` / `job` /
`c3` legs and, for N > 1, the torch.distributed transport leg beside the C-ABI one.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E peak 8 TB/s (spec); ~6.3 TB/s achievable


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="c4_3m_regional")
    ap.add_argument("--fields", type=int, default=13, help="3-D fields per Regrid bundle (histlist_3d has 13 nz fields)")
    ap.add_argument("--layout", default="cell_fast", choices=["cell_fast", "lev_fast"])
    ap.add_argument("--io", default="f64", choices=["f64", "f32"], help="field element type in HBM; f64 = reference-faithful headline")
    ap.add_argument("--full", action="store_true",
                    help="also run the self-checks, device-copy rates, CPU baseline, extra legs and (N > 1) the comparison transport; "
                         "a plain run times the headline only")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write the last step's results to DIR/*.npy (a fixed seeded sample when larger than 32 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline and the extra legs (profiling runs)")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip production_path / store / job / cell_numbering / end_to_end_pcie")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--calib", action="store_true", help="also launch a known-byte-count streaming kernel (PMC calibration)")
    ap.add_argument("--leg", default=None, choices=["job", "store", "c3"],
                    help="internal: run only this leg in THIS (fresh) process and print its JSON object -- a --full run starts one "
                         "child process per leg so that its first-call numbers are first-in-process ones")
    ap.add_argument("--ownership", default="auto", choices=["auto", "aligned", "para_range", "need"],
                    help="N > 1: who owns which source cells -- aligned / para_range: the library's id blocks; need: every cell to the lowest rank whose "
                         "rows reference it (meshes without banded numbering); auto: aligned when the numbering is banded, else need")
    ap.add_argument("--block-decomp-file", default=None, help="N > 1: an MPAS graph partition file (the namelist's block_decomp_file, one owner per "
                                                              "cell): the source cells are partitioned as the model partitions them")
    ap.add_argument("--tune", action="append", default=[], metavar="KEY=VALUE",
                    help="kernel knob for experiments (mpg_tune), e.g. a3_staged=0; the default run sets none")
    return ap.parse_args()


def synth_fields_device(torch, lat, lon, nlev, nfields, out_rows, seed=20240807):
    """f(lat,lon,k) = a_k + b_k x + c_k y + d_k z + 0.1 sin(5 lon) cos(3 lat), written in
    place into out_rows [nfields*nlev][n] on the device."""
    dev = out_rows.device
    lat_t = torch.as_tensor(lat, device=dev)
    lon_t = torch.as_tensor(lon, device=dev)
    cl = torch.cos(lat_t)
    x, y, z = cl * torch.cos(lon_t), cl * torch.sin(lon_t), torch.sin(lat_t)
    wig = 0.1 * torch.sin(5.0 * lon_t) * torch.cos(3.0 * lat_t)
    rng = np.random.default_rng(seed)
    co = torch.as_tensor(rng.uniform(-1.0, 1.0, (nfields * nlev, 4)), device=dev)
    for r in range(nfields * nlev):
        out_rows[r].copy_(co[r, 0] + co[r, 1] * x + co[r, 2] * y + co[r, 3] * z + wig)


DUMP_BYTES = 32 << 20     # --dump-outputs: at most this many bytes of results over all ranks


def dump_outputs(dirname, out, rank, world, budget=DUMP_BYTES, seed=20240807):
    """--dump-outputs DIR: what the timed path computed in its last step, the result bundle `out` [F][nlev][ny][nx] (N > 1: this rank's
    rows), in its own element type (float64, or float32 with --io f32).  Whole as DIR/out.npy when it fits the budget (budget / N per
    rank), else DIR/out_sample.npy: the values at a fixed seeded sample of flat indices (np.random.default_rng(seed).integers(0, out.numel(),
    budget // N // element size), then np.unique: sorted, distinct) -- the same indices for the same arguments.  N > 1: out_rank<r>*.npy."""
    os.makedirs(dirname, exist_ok=True)
    suffix = "_rank%d" % rank if world > 1 else ""
    flat = out.reshape(-1)
    n = budget // world // out.element_size()
    if flat.numel() <= n:
        np.save(os.path.join(dirname, "out%s.npy" % suffix), out.cpu().numpy())
        return
    idx = np.unique(np.random.default_rng(seed).integers(0, flat.numel(), n))
    import torch
    vals = flat[torch.as_tensor(idx, device=flat.device)]
    np.save(os.path.join(dirname, "out_sample%s.npy" % suffix), vals.cpu().numpy())


def self_launch(args):
    """`python bench.py --gpus N` (N > 1) started WITHOUT a torch.distributed.run environment: start the N ranks as a
    fresh child job (one process per GPU, rendezvous on 127.0.0.1) and relay its output and exit code.  This parent has
    not touched the GPU (nothing but argparse has run) and never replaces itself with another program; rank 0 of the
    child job prints the JSON line on the inherited stdout."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC (RCCL P2P over xGMI on this driver)
    env.setdefault("OMP_NUM_THREADS", "4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    # Wall-clock watchdog: a rank that never arrives (a dead GPU, a stale rendezvous) must end the job, not hang it.  The
    # children live in their own process group; on the deadline exactly that group is killed and the exit code is non-zero.
    limit = float(os.environ.get("MPASSIT_BENCH_TIMEOUT_S", "900"))
    child = subprocess.Popen(cmd, env=env, start_new_session=True)
    try:
        return child.wait(timeout=limit)
    except subprocess.TimeoutExpired:
        import signal
        sys.stderr.write("bench.py: the %d-rank child job did not finish within %.0f s (MPASSIT_BENCH_TIMEOUT_S); killing its process group\n" % (args.gpus, limit))
        try:
            os.killpg(child.pid, signal.SIGKILL)
        except ProcessLookupError:
            pass
        child.wait()
        return 124


def fresh_process_leg(name, args):
    """Run one leg (`job`, `store`) in a FRESH child process and return its JSON object: MPASSIT is a single-shot tool
    (mpassit.F90:105-137), so what a run pays for its Stores and its first time level are the first-in-process values, and
    by the time this process gets to those legs it has loaded every code object and warmed every allocation.  A child is
    started (never an exec: this process has initialised the GPU), bounded by a timeout, and only its last stdout line is
    read; a leg that fails is reported as an error string, it does not take the bench line with it."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--workload", args.workload] + sum((["--tune", kv] for kv in args.tune), [])
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=float(os.environ.get("MPASSIT_BENCH_LEG_TIMEOUT_S", "420")))
    except subprocess.TimeoutExpired:
        return {"error": "leg %s timed out" % name}
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        return {"error": "leg %s failed rc %d: %s" % (name, r.returncode, r.stderr[-300:])}
    return json.loads(lines[-1])


def run_leg(args):
    """`--leg job|store`: this process IS the fresh process; nothing but mpg_init has touched the device before the leg."""
    import torch
    from mpassit_amd import _lib, regrid as R, workloads
    t0 = time.perf_counter()
    _lib.init(0)
    init_ms = (time.perf_counter() - t0) * 1e3
    for kv in args.tune:
        k, v = kv.split("=")
        _lib.tune(k, int(v))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.leg == "store":
        m, g, _, _ = workloads.workload(args.workload)
        res = store_leg(R, m, g)
    elif args.leg == "c3":
        res = c3_leg(torch, R, workloads, dev)
    else:
        res = job_leg(torch, R, workloads, args, dev)
    if res is not None:
        res["mpg_init_ms"] = round(init_ms, 1)
    print(json.dumps(res), flush=True)
    _lib.finalize()


def main():
    args = parse()
    if args.leg:
        return run_leg(args)
    if args.gpus > 1 and "RANK" not in os.environ:
        raise SystemExit(self_launch(args))
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: start bench.py with --nproc-per-node equal to --gpus" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the HIP path has no CPU fallback)")
    ndev = torch.cuda.device_count()
    backend = os.environ.get("MPASSIT_DIST_BACKEND", "nccl")  # "gloo" = rehearsal on fewer GPUs than ranks
    dev_index = local_rank if backend == "nccl" else local_rank % ndev
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    def all_gather_object(obj):
        if world == 1:
            return [obj]
        out = [None] * world
        dist.all_gather_object(out, obj)
        return out

    from mpassit_amd import _lib, dist as mdist, regrid as R, workloads
    _lib.init(dev_index)
    for kv in args.tune:
        k, v = kv.split("=")
        _lib.tune(k, int(v))
    arch, n_cu, hbm = _lib.device_info()

    t0 = time.time()
    m, g, nlev, desc = workloads.workload(args.workload)
    t_gen = time.time() - t0
    F = args.fields
    layout = R.LAYOUT_CELL_FAST if args.layout == "cell_fast" else R.LAYOUT_LEV_FAST

    # N > 1: the product's own transport is the C-ABI's (mpg_comm_init -> mpg_halo_build -> mpg_halo_exchange_dev: librccl directly, what the
    # Fortran / C hosts call); `value` is timed on it.  The same schedule on torch.distributed (all_to_all_single over the nccl backend =
    # RCCL) is timed FIRST in the same run as the comparison leg (--full only).  MPASSIT_BENCH_TRANSPORT=torch | cabi runs one leg only.
    # Under the gloo rehearsal backend (ranks sharing a card, where RCCL refuses a second rank per device) the default is the torch leg alone.
    want = os.environ.get("MPASSIT_BENCH_TRANSPORT", "both")
    if want not in ("both", "torch", "cabi"):
        raise SystemExit("MPASSIT_BENCH_TRANSPORT must be both, torch or cabi")
    if world == 1:
        legs = ["torch"]
    elif want == "both":
        legs = ["torch", "cabi"] if backend == "nccl" or os.environ.get("MPASSIT_BENCH_FORCE_CABI_LEG") == "1" else ["torch"]
        if not args.full:
            legs = legs[-1:]           # the leg that supplies `value`
    else:
        legs = [want]
    import uuid
    io32 = args.io == "f32"

    class Leg:
        pass

    def run_transport_leg(transport):
        """One whole measurement on one transport: Store, schedule, sources, W warm-up and K timed steps (barrier + synchronise on
        both sides, max over ranks), the halo object of that transport."""
        L_ = Leg()
        run_id = all_gather_object(uuid.uuid4().hex if rank == 0 else None)[0]
        id_file = "/dev/shm/mpassit_bench_%s.rcclid" % run_id   # fresh per leg
        os.environ["MPASSIT_RUN_ID"] = run_id                   # tags the id file of the C-ABI transport: several ranks without one are refused
        sr = mdist.ShardedRegrid(m, g, R.REGRIDMETHOD_BILINEAR, rank, world, all_gather_object, transport=transport, id_file=id_file,
                                 ownership=args.ownership if world > 1 else "aligned", decomp_file=args.block_decomp_file if world > 1 else None)
        L_.sr = sr
        c0, c1 = sr.sched.own
        own_sel = sr.sched.owned_ids if sr.sched.mode == "owned" else slice(c0, c1)     # the cells this rank provides (an id list in the owned form)
        big_bundle = io32 and world == 1 and F * nlev * 8.0 * sr.sched.n_local > 40e9
        if big_bundle:
            # BASELINE configs[4] as written ("100+ 3-D fields" in ONE bundle, interp.F90:240-254): the float64 staging copies of the
            # generic path below would not fit beside 58 GB of sources + 143 GB of results; the source goes straight into its final
            # form, field by field: float32, file order or cell-fast
            own = local = None
            src_for_kernel = torch.empty((F, sr.sched.n_local, nlev) if layout == R.LAYOUT_LEV_FAST else (F, nlev, sr.sched.n_local),
                                         dtype=torch.float32, device=dev)
            one = torch.empty((nlev, sr.sched.n_local), dtype=torch.float64, device=dev)
            for f in range(F):
                synth_fields_device(torch, m.latCell, m.lonCell, nlev, 1, one, seed=20240807 + f)
                src_for_kernel[f].copy_(one.t() if layout == R.LAYOUT_LEV_FAST else one)
            del one
        elif world > 1 and (io32 or layout == R.LAYOUT_LEV_FAST):
            # sharded run on the sources as the driver holds them (float32 and / or MPAS file order, input_data.F90:630-655): the local
            # slab exists in its final form only -- [F][n_local][L] in file order, where a neighbour's strip is one byte range per field --
            # and the halo exchange moves that element type
            local = sr.local_buffer(F, nlev, dev, dtype=torch.float32 if io32 else torch.float64, layout=layout)
            lev_fast = layout == R.LAYOUT_LEV_FAST
            if sr.sched.mode == "range":
                own = sr.own_view(local)
            else:
                own = torch.empty((F, c1 - c0, nlev) if lev_fast else (F * nlev, c1 - c0), dtype=local.dtype, device=dev)
            gen = torch.empty((F * nlev, c1 - c0), dtype=torch.float64, device=dev)
            synth_fields_device(torch, m.latCell[own_sel], m.lonCell[own_sel], nlev, F, gen)
            own.copy_(gen.view(F, nlev, -1).permute(0, 2, 1) if lev_fast else gen)
            del gen
            src_for_kernel = local
        else:
            local = sr.local_buffer(F, nlev, dev)
            if sr.sched.mode == "range":
                own = sr.own_view(local)
            else:
                own = torch.empty((F * nlev, c1 - c0), dtype=torch.float64, device=dev)
            synth_fields_device(torch, m.latCell[own_sel], m.lonCell[own_sel], nlev, F, own)
            src_for_kernel = local
            if layout == R.LAYOUT_LEV_FAST:  # [F][n][L]
                src_for_kernel = local.view(F, nlev, -1).permute(0, 2, 1).contiguous()
            if io32:  # fused ingest/egress variant: float32 in HBM on both sides, float64 arithmetic (not the headline)
                src_for_kernel = src_for_kernel.float()
                del local
                local = None
        out = torch.empty((F, nlev, sr.rh.ny_dst, sr.rh.nx_dst), dtype=torch.float32 if io32 else torch.float64, device=dev)
        torch.cuda.synchronize()
        L_.local, L_.own, L_.src_for_kernel, L_.out = local, own, src_for_kernel, out

        ev = []
        # N > 1: the halo exchange of batch s+1 runs on its own stream while batch s is regridded (two source buffers);
        # every step still performs exactly one exchange and one Regrid.
        pipe = None
        if world > 1:
            local2 = local.clone()
            bufs = [local, local2]
            owns = [own, sr.own_view(local2)] if sr.sched.mode == "range" else [own, own]
            halo_stream = torch.cuda.Stream(device=dev)
            pipe = {"n": 0, "halo_done": [torch.cuda.Event(), torch.cuda.Event()], "comp_done": [None, None], "ev": []}

            def exchange_into(b, record=False):
                with torch.cuda.stream(halo_stream):
                    if pipe["comp_done"][b] is not None:
                        halo_stream.wait_event(pipe["comp_done"][b])   # the Regrid that last read this buffer
                    if record:
                        x0, x1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        x0.record(halo_stream)
                    sr.sched.exchange(owns[b], bufs[b], pack_fn=sr._pack)
                    if record:
                        x1.record(halo_stream)
                        pipe["ev"].append((x0, x1))
                    pipe["halo_done"][b].record(halo_stream)
            halo_stream.wait_stream(torch.cuda.current_stream())
            exchange_into(0)

        def one_step(record):
            if world > 1:
                b = pipe["n"] % 2
                exchange_into(1 - b, record)                           # next batch's halo, overlapped
                torch.cuda.current_stream().wait_event(pipe["halo_done"][b])
                src_t = bufs[b]
            else:
                src_t = src_for_kernel
            if record:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            if io32:
                sr.rh.regrid_typed(src_t.view(-1), nlev=nlev, nfields=F, layout=layout, out=out)
            else:
                sr.rh.regrid(src_t.view(-1), nlev=nlev, nfields=F, layout=layout, out=out)
            if record:
                e1.record()
                ev.append((e0, e1))
            if world > 1:
                if pipe["comp_done"][b] is None:
                    pipe["comp_done"][b] = torch.cuda.Event()
                pipe["comp_done"][b].record()
                pipe["n"] += 1

        if args.calib:  # 1 GiB read / 1 GiB write, 8 B per lane fully coalesced: calibrates FETCH_SIZE / WRITE_SIZE
            n_cal = 1 << 27
            cal_src = torch.zeros(n_cal, dtype=torch.float64, device=dev)
            cal_dst = torch.empty(n_cal, dtype=torch.float64, device=dev)
            cal_ids = torch.arange(n_cal, dtype=torch.int32, device=dev)
            for _ in range(3):
                _lib.check(_lib.load().mpg_pack_dev(ctypes.c_void_p(cal_src.data_ptr()), ctypes.c_int64(n_cal), ctypes.c_int(1),
                                                    ctypes.c_void_p(cal_ids.data_ptr()), ctypes.c_int64(n_cal),
                                                    ctypes.c_void_p(cal_dst.data_ptr()),
                                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.synchronize()
            del cal_src, cal_dst, cal_ids

        for _ in range(args.warmup):
            one_step(False)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            one_step(True)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        dt = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([dt], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        L_.dt = dt
        L_.kern_ms = float(np.mean([a.elapsed_time(b) for a, b in ev])) if ev else float("nan")
        L_.halo = None
        if world > 1:   # the exchange as the halo stream saw it (it overlaps the Regrid of the previous batch), and what it moved
            plan = sr.sched.plan(local.shape[0], local)
            per_rank = all_gather_object({"exchange_ms": float(np.mean([a.elapsed_time(b) for a, b in pipe["ev"]])) if pipe["ev"] else None,
                                          "kernel_ms": L_.kern_ms, "sent": int(plan.bytes_sent), "received": int(plan.bytes_received),
                                          "n_local": int(sr.sched.n_local), "needed": int(sr.n_needed), "rows": int(sr.j1 - sr.j0)})
            if transport == "cabi":
                ranks_in_group = sr.sched.comm.info()[1]      # mpg_comm_info: what the C-ABI communicator itself says
            else:
                ranks_in_group = dist.get_world_size()
            L_.halo = {"mode": sr.sched.mode,
                       "transport": "%s all_to_all_single (grouped send/recv, zero-size peers skipped)" % backend if transport == "torch" else
                                    "C-ABI mpg_halo_exchange_dev (librccl: grouped ncclSend / ncclRecv)",
                       "ranks_in_group": int(ranks_in_group),
                       "ms_per_step": dt / args.steps * 1e3, "fields_per_s": F * args.steps / dt,
                       "exchange_ms_max": max(r["exchange_ms"] or 0.0 for r in per_rank),
                       "kernel_ms_max": max(r["kernel_ms"] for r in per_rank),
                       "halo_bytes_per_step": sum(r["received"] for r in per_rank),
                       "halo_bytes_per_step_max_rank": max(r["received"] for r in per_rank),
                       "per_rank": per_rank}
        L_.n_unmapped = L_.bundle_check = None
        if args.full:
            # correctness guard inside the bench, on every transport's own handle: constant field -> constant on mapped points (sum of weights = 1)
            chk = torch.full((nlev, sr.sched.n_local), 2.5, dtype=torch.float64, device=dev)
            if layout == R.LAYOUT_LEV_FAST:
                chk = chk.t().contiguous()
            o1 = sr.rh.regrid(chk.view(-1), nlev=nlev, nfields=1, layout=layout)
            torch.cuda.synchronize()
            bad = int(((o1 != 0.0) & ((o1 - 2.5).abs() > 1e-12)).sum().item())
            L_.n_unmapped = int((o1[0, 0] == 0.0).sum().item())
            del chk, o1
            if bad:
                raise SystemExit("bench self-check failed: %d points off" % bad)
        if args.full and world == 1:
            # a bundle's first and last field against the same fields regridded alone (any 32-bit overflow in field * level * point
            # offsets would show in the last one): bit for bit
            L_.bundle_check = True
            for f in sorted({0, F - 1}):
                sf = src_for_kernel.view(F, -1)[f]
                alone = sr.rh.regrid_typed(sf, nlev=nlev, nfields=1, layout=layout) if io32 else sr.rh.regrid(sf, nlev=nlev, nfields=1, layout=layout)
                if not torch.equal(alone[0], out[f]):
                    raise SystemExit("bench self-check failed: field %d of the %d-field bundle differs from the same field regridded alone" % (f, F))
                del alone
        torch.cuda.synchronize()
        L_.P_local, L_.U, L_.mode, L_.store_ms, L_.kernel = sr.rh.n_dst, sr.n_needed, sr.sched.mode, sr.store_ms, kernel_label(sr.rh, layout, R)
        return L_

    def teardown(L_):
        """A finished leg keeps its numbers; its handle, communicator and buffers go."""
        if L_.sr is not None:
            L_.sr.destroy()
        L_.sr = L_.local = L_.own = L_.src_for_kernel = L_.out = None
        torch.cuda.empty_cache()

    done, leg_error = {}, {}
    primary = None
    for transport in legs:
        if primary is not None:        # the comparison leg's buffers go before the product's leg allocates its own; its numbers stay
            teardown(primary)
        err = res_leg = None
        try:
            res_leg = run_transport_leg(transport)
        except Exception as e:         # noqa: BLE001 -- a failing C-ABI leg is reported IN the line (halo.transports.cabi.error); the torch leg,
            if world == 1 or transport != "cabi":   # already measured, supplies the line's numbers, and the run ends non-zero below.  Nothing is
                raise                                # re-executed and no communicator is built again in a process whose RCCL call failed.
            err = "%s: %s" % (type(e).__name__, str(e)[:300])
            res_leg = None
        errs = all_gather_object(err)
        if any(errs):                  # one rank's failure is every rank's: nobody goes on with a communicator a peer has left
            leg_error[transport] = next(e for e in errs if e)
            continue
        done[transport] = res_leg.halo
        primary = res_leg
    if primary is None:                # MPASSIT_BENCH_TRANSPORT=cabi alone, and it failed: a line without a measurement
        if rank == 0:
            print(json.dumps({"metric": "interpolated 3-D fields/sec (nCells x nLev -> nx x ny)", "value": None, "unit": "fields/s", "n_gpus": world,
                              "steps": args.steps, "warmup": args.warmup, "halo": {"transports": {k: {"error": e} for k, e in leg_error.items()}}}), flush=True)
        sys.stderr.write("bench.py: transport leg failed: %s\n" % leg_error)
        sys.exit(3)
    transport = "cabi" if "cabi" in done else "torch"
    sr, local, own, src_for_kernel, out, dt, kern_ms, halo = (primary.sr, primary.local, primary.own, primary.src_for_kernel, primary.out, primary.dt,
                                                               primary.kern_ms, primary.halo)
    P_local, n_unmapped, bundle_check = primary.P_local, primary.n_unmapped, primary.bundle_check
    if halo is not None:
        # both transports of the run, flat: ms per step, exchange time as the halo stream saw it, bytes
        halo = dict(halo)
        halo["value_transport"] = transport
        halo["transports"] = {k: {kk: v[kk] for kk in ("transport", "ranks_in_group", "ms_per_step", "fields_per_s", "exchange_ms_max", "kernel_ms_max",
                                                       "halo_bytes_per_step", "halo_bytes_per_step_max_rank")} for k, v in done.items() if v}
        for k, e in leg_error.items():
            halo["transports"][k] = {"error": e}
        if world > 1 and "cabi" not in legs:
            halo["transports"]["cabi"] = {"skipped": "MPASSIT_BENCH_TRANSPORT=torch" if want == "torch" else
                                                     "backend %s: ranks may share a card, RCCL refuses a second rank per device" % backend}
        if world > 1 and "torch" not in legs and want == "both":
            halo["transports"]["torch"] = {"skipped": "comparison leg: --full"}

    if args.dump_outputs:
        dump_outputs(args.dump_outputs, out, rank, world)

    copy_gbs, mix = None, {}
    if args.full:
        # live streaming reference of THIS device (boxes differ by >10 %): plain 2 GiB -> 2 GiB device copy
        cp_a = torch.empty(1 << 28, dtype=torch.float64, device=dev)
        cp_b = torch.empty_like(cp_a)
        cp_b.copy_(cp_a)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            cp_b.copy_(cp_a)
        e1.record()
        torch.cuda.synchronize()
        copy_gbs = 5 * 2 * cp_a.numel() * 8 / (e0.elapsed_time(e1) * 1e-3) / 1e9
        # ... and what the same memory system gives a 2 reads : 1 write mix (the headline kernel's traffic is 61 : 39) and pure writes
        # (profiles/r05_hbm_mix.md: no mix reaches the data sheet's 8 TB/s; a copy's 1 : 1 is the slowest)
        for key, fn, nbytes in (("device_add_2r1w_GBs", lambda: torch.add(cp_a, cp_b, out=cp_b), 3), ("device_fill_GBs", lambda: cp_b.fill_(1.5), 1)):
            fn()
            e0.record()
            for _ in range(5):
                fn()
            e1.record()
            torch.cuda.synchronize()
            mix[key] = 5 * nbytes * cp_a.numel() * 8 / (e0.elapsed_time(e1) * 1e-3) / 1e9
        del cp_a, cp_b

    U = primary.U
    esz = 4.0 if io32 else 8.0  # element size of the field values in HBM (float64 = reference-faithful headline)
    alg_bytes = F * nlev * esz * (U + P_local) + P_local * 36.0  # U*L*e + P*L*e per field + P*36 once per launch
    achieved = alg_bytes / (kern_ms * 1e-3) / 1e9
    traffic, traffic_source = (None, None)
    if world == 1:
        traffic, traffic_source = recorded_traffic(args.workload, F, args.layout, io32)

    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and not io32:
        cpu = cpu_baseline(sr, src_for_kernel if layout == R.LAYOUT_CELL_FAST else local, nlev, args.cpu_seconds, m, g)

    # "report two timings" -- kernel-only above, and end to end through the PCIe link (one 3-D field from
    # pageable host memory to pageable host memory: upload, Regrid, download; never `value`)
    e2e = None
    extras = args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and not args.no_extras
    if extras and layout == R.LAYOUT_CELL_FAST and not io32:
        e2e = {}
        for name, dt_np in (("f64", np.float64), ("f32", np.float32)):
            hs = np.random.default_rng(1).standard_normal((nlev, sr.sched.n_local)).astype(dt_np)
            ho = np.empty((1, nlev, sr.rh.ny_dst, sr.rh.nx_dst), dt_np)
            sr.rh.regrid_typed_host(hs, nlev=nlev, out=ho)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                sr.rh.regrid_typed_host(hs, nlev=nlev, out=ho)
                ts.append(time.perf_counter() - t0)
            e2e[name + "_fields_per_s"] = 1.0 / min(ts)
        # one 3-D field, pageable host -> device -> pageable host through mpg_regrid_typed (chunked, both PCIe directions at once)

    # The headline mesh numbers its cells row by row -- the best case for a cell-fast gather.  Beside it: the SAME 3.0 M cells
    # renumbered along a Morton curve (workload c4_3m_morton), what a production mesh reordered by a space-filling curve
    # or a graph partitioner looks like.  Extra object, never `value`.
    numbering = None
    if extras and args.workload == "c4_3m_regional" and not io32:
        numbering = realistic_numbering_leg(torch, R, workloads, args, F, layout, dev, out, sr.rh)
    # what the shipped Fortran driver runs: float32 as the MPAS / WRF files hold it, MPAS file order, either byte order
    production = store = job = c3 = None
    if extras and not io32 and layout == R.LAYOUT_CELL_FAST:
        production = production_path_leg(torch, R, args, F, nlev, dev, sr, local, U_hint=sr.n_needed)
        del out, local, src_for_kernel, own
        primary.local = primary.own = primary.src_for_kernel = primary.out = None
        torch.cuda.empty_cache()
        store = fresh_process_leg("store", args)      # one fresh child process per leg: first-in-process numbers
        job = fresh_process_leg("job", args) if args.workload == "c4_3m_regional" else None
        c3 = fresh_process_leg("c3", args) if args.workload == "c4_3m_regional" else None

    if rank == 0:
        fields_per_s = F * args.steps / dt
        # What the driver's record keeps whole is `roofline` and `config`: the numbers of the paths a run of the shipped
        # driver actually takes (float32 file order; the whole job; the Stores) ride inside `roofline` as flat scalars.  Cold values
        # are FIRST-IN-PROCESS ones: MPASSIT is a single-shot tool (mpassit.F90:105-137).
        # ... as FLAT scalars with short keys: the driver's record flattens `roofline` (a nested object inside it was dropped in
        # round 4) and cuts keys at 40 and strings at 120 characters.  The full objects stay at the top level of the line.
        flat = {}
        if production:
            flat.update(f32_lev_fast_ms=round(production["kernel_ms"], 4), f32_lev_fast_frac=round(production["roofline_frac"], 4),
                        f32_lev_fast_frac_be=round(production["roofline_frac_big_endian"], 4),
                        f32_lev_fast_traffic_ratio=round(production["traffic"] / production["alg_bytes_per_launch"], 3) if production.get("traffic") else None)
        if job and "error" not in job:
            flat.update(job_cold_first_ms=job["cold_first_ms"], job_cold_ms=job["cold_ms"], job_warm_ms=job["warm_ms"], job_warm_frac=job["frac_warm"],
                        job_geometry_first_ms=job["geometry_first_ms"], job_mpg_init_ms=job.get("mpg_init_ms"))
        if store and "error" not in store:
            st = {k: v for k, v in store.items() if isinstance(v, dict)}
            flat.update(store_first_ms_sum=round(sum(v["ms_first"] for v in st.values()), 3), store_ms_sum=round(sum(v["ms"] for v in st.values()), 3),
                        store_mpg_init_ms=store.get("mpg_init_ms"))
            for k, v in st.items():
                flat["store_%s_first_ms" % k] = round(v["ms_first"], 3)
        if c3 and "error" not in c3:   # BASELINE configs[2]: conservative snow fields + nearest soil on the 655 k mesh
            flat.update({k: c3[k] for k in ("c3_conserve_ms", "c3_conserve_frac", "c3_nearest_soil_ms", "c3_nearest_soil_frac", "c3_store_conserve_first_ms",
                                            "c3_store_nearest_first_ms", "c3_job_cold_first_ms", "c3_job_warm_ms", "c3_job_warm_frac")})
        if numbering:                  # the headline's kernel on the same cells numbered as production meshes are
            flat.update(morton_numbering_frac=round(numbering["roofline_frac"], 4), cutout_numbering_frac=round(numbering["cutout"]["roofline_frac"], 4),
                        odd_grid_1799x1059_frac=round(numbering["odd_grid"]["roofline_frac"], 4),
                        odd_grid_1799x1059_f32_lev_fast_frac=round(numbering["odd_grid_f32_lev_fast"]["roofline_frac"], 4))
        if traffic:
            flat["traffic_ratio"] = round(traffic / alg_bytes, 3)
        rec = {
            "metric": "interpolated 3-D fields/sec (nCells x nLev -> nx x ny)",
            "value": fields_per_s, "unit": "fields/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": "%s: %s" % (args.workload, desc), "fields_per_step": F, "nlev": nlev, "nCells": int(m.nCells),
                       "target_points": int(g.nx * g.ny), "method": "bilinear", "src_layout": args.layout,
                       "io_dtype": "f32 (fused ingest/egress, f64 arithmetic)" if io32 else "f64",
                       "parallelism": "rows%d+halo(%s,%s)" % (world, primary.mode, "c-abi rccl" if transport == "cabi" else "torch " + backend) if world > 1 else "single-gpu",
                       "row_split": ("para_range" if mdist.row_quantum(g.nx, g.ny, world) == 1 else "block boundaries on multiples of %d rows (planes of whole 128-byte lines)"
                                     % mdist.row_quantum(g.nx, g.ny, world)) if world > 1 else None,
                       "unmapped_points_rank0": n_unmapped, "bundle_ends_equal_single": bundle_check},
            "roofline": dict({"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                              "traffic": traffic, "traffic_source": traffic_source, "kernel": primary.kernel,
                              "kernel_ms": kern_ms, "alg_bytes_per_launch": alg_bytes, "unique_src_cells": int(U),
                              "device_copy_GBs": copy_gbs, **mix}, **flat),
            "cpu_baseline": cpu,
            "end_to_end_pcie": e2e,
            "production_path": production,
            "store": store,
            "job": job,
            "c3": c3,
            "cell_numbering": numbering,
            "halo": halo,
            "store_ms": primary.store_ms,
            "device": {"arch": arch, "cus": n_cu, "hbm_gib": round(hbm / 2 ** 30, 1), "name": torch.cuda.get_device_name(dev),
                       "uuid": str(getattr(torch.cuda.get_device_properties(dev), "uuid", ""))},
            "setup_s": {"synthetic_mesh_and_grid": round(t_gen, 2)},
        }
        print(json.dumps(rec), flush=True)
    if primary.sr is not None:
        teardown(primary)
    if world > 1:
        dist.destroy_process_group()
    if leg_error:      # the line above carries the error (halo.transports) and the comparison leg's numbers; the run itself has failed
        sys.stderr.write("bench.py: transport leg failed: %s\n" % leg_error)
        sys.exit(3)


def realistic_numbering_leg(torch, R, workloads, args, F, layout, dev, out, rh_rows):
    """The same step on the same 3.0 M cells numbered as production meshes are -- c4_3m_morton: along a Morton curve over the region itself;
    c4_3m_cutout (round 6): as a limited-area CUT-OUT of a global mesh numbered along a space-filling curve over the whole sphere (how
    MPAS-Limited-Area leaves a regional mesh) -- fields/s, roofline fraction, the kernel the library picked and its tile-list locality
    statistics next to those of the row-numbered headline mesh.  The Morton leg's keys stay at the top level; `cutout` holds the other.
    `odd_grid` (round 6): the headline's mesh under HRRR's own grid size, 1799 x 1059 mass points -- an odd number of points per level, so
    every level plane of the result starts somewhere else inside a 128-byte line (profiles/r06_plane_alignment.md); `odd_grid_f32_lev_fast`:
    the same in float32 file order, what the driver issues."""
    def one(name, f32_file_order=False):
        m, g, nlev, desc = workloads.workload(name)
        mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
        rh = R.regrid_store(mesh, grid, R.REGRIDMETHOD_BILINEAR)
        U = rh.unique_sources().size
        src = torch.empty((F * nlev, m.nCells), dtype=torch.float64, device=dev)
        synth_fields_device(torch, m.latCell, m.lonCell, nlev, F, src)
        lay, es = layout, 8.0
        if f32_file_order:
            lay, es = R.LAYOUT_LEV_FAST, 4.0
            src = src.view(F, nlev, -1).permute(0, 2, 1).to(torch.float32).contiguous()
            o = out.view(-1).view(torch.float32)[:F * nlev * rh.n_dst].view(F, nlev, g.ny, g.nx)
            launch = lambda: rh.regrid_typed(src.view(-1), nlev=nlev, nfields=F, layout=lay, out=o)   # noqa: E731
        else:
            if layout == R.LAYOUT_LEV_FAST:
                src = src.view(F, nlev, -1).permute(0, 2, 1).contiguous()
            o = out.view(-1)[:F * nlev * rh.n_dst].view(F, nlev, g.ny, g.nx)   # the headline's result buffer: starts on a line
            launch = lambda: rh.regrid(src.view(-1), nlev=nlev, nfields=F, layout=lay, out=o)   # noqa: E731
        steps = max(3, min(args.steps, 10))
        for _ in range(2):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            launch()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / steps
        alg = F * nlev * es * (U + rh.n_dst) + rh.n_dst * 36.0
        res = {"workload": name, "fields_per_s": F / ms * 1e3, "kernel_ms": ms, "steps": steps, "target_points": int(rh.n_dst),
               "roofline_frac": alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "kernel": kernel_label(rh, lay, R),
               "tile_stats": dict(zip(("tile_nx", "tile_ny", "reuse", "line_fill"), rh.tile_stats() or ()))}
        rh.release()
        mesh.destroy()
        grid.destroy()
        del src
        return res
    res = one("c4_3m_morton")
    res["tile_stats_row_numbered"] = dict(zip(("tile_nx", "tile_ny", "reuse", "line_fill"), rh_rows.tile_stats() or ()))
    res["cutout"] = one("c4_3m_cutout")
    res["odd_grid"] = one("x_c4_1799x1059")
    res["odd_grid_f32_lev_fast"] = one("x_c4_1799x1059", f32_file_order=True)
    return res


def kernel_label(rh, layout, R):
    """Name of the Regrid kernel the library picked for this handle (mpg_handle_kernel_choice)."""
    cf, lf, mu = rh.kernel_choice()
    if layout == R.LAYOUT_CELL_FAST:
        return "k_apply3_cfu (staged, a3_staged %d, <= %d cells per tile)" % (cf - 1, mu) if cf > 0 else "k_apply3_cf (lane gather)"
    return "k_apply3_lfu (staged, <= %d cells per tile)" % mu if lf > 0 else "k_apply3_lf_rows (row gather, linear tiles)"


def recorded_traffic(workload, F, layout, io32):
    """HBM bytes per launch from the PMC passes of the same command (tools/profile_bench.sh -> tools/summarize_profile.py ->
    profiles/traffic_*.json).  NOT measured in this run: the file is regenerated whenever the default kernel changes, and
    `traffic_source` names the summary it came from."""
    tpath = os.path.join(ROOT, "profiles", "traffic_%s_f%d_%s%s.json" % (workload, F, layout, "_io32" if io32 else ""))
    if not os.path.exists(tpath):
        return None, None
    d = json.load(open(tpath))
    return d.get("hbm_bytes_per_launch"), "recorded, not live: %s" % d.get("source", os.path.relpath(tpath, ROOT))


def _time_launches(torch, fn, steps):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def production_path_leg(torch, R, args, F, nlev, dev, sr, local, U_hint):
    """`--io f32 --layout lev_fast` on the same workload: float32 sources in MPAS file order [field][cell][level]
    (input_data.F90:630,645), float32 results (NF90_FLOAT, write_data.F90:779), float64 arithmetic -- the Regrid the Fortran
    driver issues -- in host byte order and with both sides big-endian (what the driver's NetCDF-classic file flow passes)."""
    rh = sr.rh
    P = rh.n_dst
    src = local.view(F, nlev, -1).permute(0, 2, 1).float().contiguous()
    out = torch.empty((F, nlev, rh.ny_dst, rh.nx_dst), dtype=torch.float32, device=dev)
    steps = max(3, min(args.steps, 10))
    alg = F * nlev * 4.0 * (U_hint + P) + P * 36.0
    res = {"flags": "--io f32 --layout lev_fast", "fields_per_step": F, "steps": steps, "alg_bytes_per_launch": alg}
    ms = _time_launches(torch, lambda: rh.regrid_typed(src.view(-1), nlev=nlev, nfields=F, layout=R.LAYOUT_LEV_FAST, out=out), steps)
    res.update(kernel_ms=ms, fields_per_s=F / ms * 1e3, roofline_frac=alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, kernel=kernel_label(rh, R.LAYOUT_LEV_FAST, R))
    ms_be = _time_launches(torch, lambda: rh.regrid_typed(src.view(-1), nlev=nlev, nfields=F, layout=R.LAYOUT_LEV_FAST, out=out, src_be=True,
                                                          dst_be=True), steps)
    res.update(kernel_ms_big_endian=ms_be, fields_per_s_big_endian=F / ms_be * 1e3, roofline_frac_big_endian=alg / (ms_be * 1e-3) / 1e9 / HBM_PEAK_GBS)
    res["traffic"], res["traffic_source"] = recorded_traffic(args.workload, F, "lev_fast", True)
    return res


def store_leg(R, m, g):
    """RegridStore of the three methods on the headline mesh and grid (weights are data: built once per run, cached), as
    points/s with the algorithmic bytes of SURVEY s8(d): P*16 (target coordinates) + T*(3*4 + 48) (elements: ids + box) +
    the weights written.  ms_first = the process's very FIRST Store of that method -- what a single-shot run pays
    (mpassit.F90:105-137) -- and the headline; ms = the fastest of the later repetitions on fresh mesh / grid objects (nothing
    from the handle cache).  None is memory-bound: what binds each kernel is in profiles/r03_store_pmc.md."""
    P = int(g.nx * g.ny)
    nT, nC, nE = int(m.nVertices), int(m.nCells), int(m.verticesOnCell.shape[1])
    codes = (("bilinear", R.REGRIDMETHOD_BILINEAR), ("nearest", R.REGRIDMETHOD_NEAREST_STOD), ("conserve", R.REGRIDMETHOD_CONSERVE))
    ms = {name: [] for name, _ in codes}
    nnz = {}
    for rep in range(3):
        mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_target(g)
        for name, code in codes:
            rh = R.regrid_store(mesh, grid, code)
            ms[name].append(rh.store_ms)
            nnz[name] = int(rh.nnz)
            rh.release()
        mesh.destroy()
        grid.destroy()
    res = {}
    for name, _ in codes:
        if name == "bilinear":
            alg = P * 16.0 + nT * (12.0 + 48.0) + P * 36.0
        elif name == "nearest":
            alg = P * 16.0 + nC * (24.0 + 4.0) + P * 4.0
        else:
            alg = (P + g.nx + g.ny + 1) * 16.0 + nC * (nE * 4.0 + 48.0) + nT * 16.0 + nnz[name] * 12.0 + (P + 1) * 4.0
        best, first = min(ms[name][1:]), ms[name][0]
        res[name] = {"ms_first": first, "ms": best, "points_per_s_first": P / (first * 1e-3), "alg_bytes": alg,
                     "frac_of_hbm_peak_first": alg / (first * 1e-3) / 1e9 / HBM_PEAK_GBS, "nnz": nnz[name]}
    return res


def job_leg(torch, R, workloads, args, dev):
    """The whole hot path of one run, through the C-ABI: interp_data (interp.F90:92-465) over the reference's default
    diag + hist lists with wrf_mod_vars=.true. -- every RegridStore, every Regrid, the wind rotation and the destaggering --
    on device-resident float32 fields in MPAS file order, target grid generated on the device.  cold = fresh mesh / grid
    objects (every Store and every tile-list build inside the timed region), cold_first = the first such pass of the
    PROCESS -- what a single-shot run pays; warm = the weights of the same objects kept (a second time level); host wall ms
    between two device synchronisations.  alg_bytes_warm = the algorithmic bytes of the warm level's Regrids and rotations
    (U*L*e_src + P*L*e_dst per field + indices and weights per call), frac_warm = those over warm_ms over the HBM peak.
    geometry_* = mpg_mesh_create (upload + dual triangles) + mpg_grid_create_proj, not part of cold_ms."""
    from mpassit_amd import interp as I
    if args.workload != "c4_3m_regional":
        return None
    m, g, nz, desc = workloads.workload(args.workload, arrays=False)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20240807)

    def f2():
        return torch.rand(m.nCells, dtype=torch.float32, device=dev, generator=gen)

    def f3(L):
        return torch.rand((m.nCells, L), dtype=torch.float32, device=dev, generator=gen)
    nsoil = 4
    inp = I.InputData(nz=nz, nzp1=nz + 1, nsoil=nsoil, hgt=torch.rand(m.nCells, dtype=torch.float64, device=dev, generator=gen), layout=R.LAYOUT_LEV_FAST)
    for n, _ in workloads.JOB_HIST_2D:
        inp.hist[n] = torch.floor(f2() * 3) if n == "xland" else f2()
    for n, _ in workloads.JOB_HIST_3D:
        inp.hist[n] = f3(nz + 1 if n in ("zgrid", "w") else nz)
    for n, _ in workloads.JOB_SOIL:
        inp.hist[n] = f3(nsoil)
    for n, _ in workloads.JOB_DIAG:
        inp.diag[n] = f3(nz) if n == "refl10cm" else f2()
    cfg = I.InterpConfig(interp_diag=True, wrf_mod_vars=True, diag_list=workloads.JOB_DIAG, hist_2d=workloads.JOB_HIST_2D,
                         hist_3d=workloads.JOB_HIST_3D, hist_soil=workloads.JOB_SOIL)
    cold, warm, geom = [], [], []
    n3d = nout = 0
    for rep in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mesh = R.Mesh.from_mpas(m)
        grid = R.Grid.from_proj(g)
        torch.cuda.synchronize()
        geom.append((time.perf_counter() - t0) * 1e3)
        for k in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            out = I.interp_data(mesh, grid, g, inp, cfg)
            e1.record()
            torch.cuda.synchronize()
            (cold if k == 0 else warm).append(((time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)))
            n3d, nout = sum(1 for v in out.values() if v.ndim == 3 and v.shape[0] >= nz), len(out)
            del out
        if rep == 0:   # algorithmic bytes of one warm time level (SURVEY s8(d) per call, regrid.ACCOUNT), in an untimed pass
            R.ACCOUNT = []
            del_out = I.interp_data(mesh, grid, g, inp, cfg)
            torch.cuda.synchronize()
            alg_warm = float(sum(b for _, b in R.ACCOUNT))
            R.ACCOUNT = None
            del del_out
        graph_ms = None
        if rep == 1:   # the same time level as ONE hipGraph (interp.GraphedInterp): what is left without the per-launch host cost
            gi = I.GraphedInterp(mesh, grid, g, inp, cfg)
            gt = []
            for _ in range(4):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                gi.replay()
                torch.cuda.synchronize()
                gt.append((time.perf_counter() - t0) * 1e3)
            graph_ms = min(gt)
            gi.close()
            del gi
        mesh.destroy()
        grid.destroy()
    warm_ms = min(w[0] for w in warm)
    return {"outputs": nout, "fields_3d": n3d, "warm_graph_replay_ms": graph_ms,
            "cold_first_ms": round(cold[0][0], 3), "cold_ms": round(min(c[0] for c in cold), 3), "warm_ms": round(warm_ms, 3),
            "geometry_first_ms": round(geom[0], 3), "geometry_ms": round(min(geom), 3),
            "alg_bytes_warm": alg_warm, "frac_warm": round(alg_warm / (warm_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "fields_3d_per_s_cold_first": n3d / (cold[0][0] * 1e-3), "fields_3d_per_s_warm": n3d / (warm_ms * 1e-3)}


def c3_leg(torch, R, workloads, dev):
    """BASELINE configs[2]: the 655 362-cell global mesh under the README's Lambert grid with the snow fields regridded conservatively
    (interp.F90:368-416), the soil bundle through the nearest-neighbour weights (the method set last, :436-447) and the
    rest of histlist_2d / 3d bilinearly -- device-resident float32 fields in MPAS file order, as the driver holds them.
    c3_conserve_* : one Regrid of the {snow, snowh} bundle through the CSR handle; c3_nearest_soil_*: one Regrid of the 3 x nsoil soil bundle;
    algorithmic bytes per SURVEY s8(d): U * L * e_src + P * L * e_dst per field + the handle's indices and weights once per call
    (CSR: nnz * 12 + (P + 1) * 4; nearest: P * 4).  c3_job_*: the whole interp_hist_data of the configuration, first-in-process cold
    and warm, fraction from the accounted bytes of its Regrids as in the `job` leg.  Store times are first-in-process."""
    from mpassit_amd import interp as I
    m, g, nz, desc = workloads.workload("c2_655k_global", arrays=False)
    nsoil = 4
    gen = torch.Generator(device=dev)
    gen.manual_seed(20240807)

    def f2():
        return torch.rand(m.nCells, dtype=torch.float32, device=dev, generator=gen)

    def f3(L):
        return torch.rand((m.nCells, L), dtype=torch.float32, device=dev, generator=gen)
    inp = I.InputData(nz=nz, nzp1=nz + 1, nsoil=nsoil, hgt=torch.rand(m.nCells, dtype=torch.float64, device=dev, generator=gen), layout=R.LAYOUT_LEV_FAST)
    for n, _ in workloads.JOB_HIST_2D:
        inp.hist[n] = torch.floor(f2() * 3) if n == "xland" else f2()
    for n, _ in workloads.JOB_HIST_3D:
        inp.hist[n] = f3(nz + 1 if n in ("zgrid", "w") else nz)
    for n, _ in workloads.JOB_SOIL:
        inp.hist[n] = f3(nsoil)
    cfg = I.InterpConfig(interp_diag=False, wrf_mod_vars=True, hist_2d=workloads.JOB_HIST_2D, hist_3d=workloads.JOB_HIST_3D, hist_soil=workloads.JOB_SOIL)
    mesh, grid = R.Mesh.from_mpas(m), R.Grid.from_proj(g)
    torch.cuda.synchronize()
    # the whole configuration first: its Stores and first calls are the process's first
    times = []
    for k in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = I.interp_data(mesh, grid, g, inp, cfg)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        n3d = sum(1 for v in out.values() if v.ndim == 3 and v.shape[0] >= nz)
        del out
    R.ACCOUNT = []
    out = I.interp_data(mesh, grid, g, inp, cfg)
    torch.cuda.synchronize()
    alg_warm = float(sum(b for _, b in R.ACCOUNT))
    R.ACCOUNT = None
    del out
    res = {"workload": "c3: " + desc + "; conservative snow / snowh, nearest soil (nsoil %d)" % nsoil, "fields_3d": n3d,
           "c3_job_cold_first_ms": round(times[0], 3), "c3_job_warm_ms": round(min(times[1:]), 3),
           "c3_job_warm_frac": round(alg_warm / (min(times[1:]) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "alg_bytes_warm": alg_warm}
    rh_c = R.regrid_store(mesh, grid, R.REGRIDMETHOD_CONSERVE)
    rh_n = R.regrid_store(mesh, grid, R.REGRIDMETHOD_NEAREST_STOD)
    res["c3_store_conserve_first_ms"], res["c3_store_nearest_first_ms"] = round(rh_c.store_ms, 3), round(rh_n.store_ms, 3)
    P = rh_c.n_dst

    def timed(fn, reps=30):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps
    snow = [inp.hist["snow"], inp.hist["snowh"]]
    outs_c = [torch.empty((1, g.ny, g.nx), dtype=torch.float64, device=dev) for _ in snow]
    ms_c = timed(lambda: rh_c.regrid_bundle(snow, nlev=1, layout=R.LAYOUT_CELL_FAST, out_dtype=torch.float64, outs=outs_c))
    U_c = int(rh_c.unique_sources().size)
    alg_c = len(snow) * (U_c * 4.0 + P * 8.0) + rh_c.nnz * 12.0 + (P + 1) * 4.0
    soil = [inp.hist[n].reshape(-1) for n, _ in workloads.JOB_SOIL]
    outs_n = [torch.empty((nsoil, g.ny, g.nx), dtype=torch.float64, device=dev) for _ in soil]
    ms_n = timed(lambda: rh_n.regrid_bundle(soil, nlev=nsoil, layout=R.LAYOUT_LEV_FAST, out_dtype=torch.float64, outs=outs_n))
    U_n = int(rh_n.unique_sources().size)
    alg_n = len(soil) * nsoil * (U_n * 4.0 + P * 8.0) + P * 4.0
    res.update(c3_conserve_ms=round(ms_c, 4), c3_conserve_frac=round(alg_c / (ms_c * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), c3_conserve_alg_bytes=alg_c,
               c3_conserve_nnz=int(rh_c.nnz), c3_conserve_unique_src=U_c,
               c3_nearest_soil_ms=round(ms_n, 4), c3_nearest_soil_frac=round(alg_n / (ms_n * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), c3_nearest_soil_alg_bytes=alg_n,
               c3_nearest_unique_src=U_n)
    rh_c.release()
    rh_n.release()
    mesh.destroy()
    grid.destroy()
    return res


def cpu_baseline(sr, local_rows, nlev, seconds, m, g):
    """Oracle ('port') apply loop on the host cores, one whole 3-D field of the same workload, same weights.
    Test infrastructure used only as the reported CPU comparator; never on the product path."""
    cores = len(os.sched_getaffinity(0))
    try:  # honour the cgroup CPU quota of the box (e.g. 16 of 256 hardware threads)
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            cores = max(1, min(cores, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    os.environ["OMP_NUM_THREADS"] = str(cores)
    from oracle import oracle as o
    o.build()
    idx, w = sr.rh.weights()
    src = local_rows.view(-1, local_rows.shape[-1])[:nlev].cpu().numpy()  # field 0: [nlev][n_local]
    dst = np.empty((nlev, idx.shape[0]))
    o.apply3_mt(idx, w, src, nlev, dst)  # warm-up / page-in
    reps, t0 = 0, time.perf_counter()
    while True:
        o.apply3_mt(idx, w, src, nlev, dst)
        reps += 1
        el = time.perf_counter() - t0
        if el > seconds or reps >= 200:
            break
    # the other half of a cold job: the oracle's RegridStore (bilinear: coordinates -> unit vectors, dual triangles, hashed
    # point-in-triangle search + weights) on the same host cores, once -- beside the GPU's `store_ms`
    t0 = time.perf_counter()
    lon_d, lat_d = o.mesh_coords_deg(m.lonCell, m.latCell)
    cxyz = o.lonlat_deg_to_xyz(lon_d, lat_d)
    tri, _ = o.dual_triangles(m.verticesOnCell, m.nVertices, cxyz)
    o.bilinear_weights(cxyz, tri, o.lonlat_deg_to_xyz(g.lon, g.lat))
    store_s = time.perf_counter() - t0
    alg_field = nlev * 8.0 * (int(np.unique(idx[idx >= 0]).size) + idx.shape[0]) + idx.shape[0] * 36.0   # SURVEY s8(d), one float64 field
    return {"value": reps / el, "unit": "fields/s", "cores": cores, "kind": "port", "GBs": round(alg_field * reps / el / 1e9, 1),
            "store_ms": store_s * 1e3,
            "sample": "%d whole 3-D fields (%d lev x %d pts), oracle OpenMP apply loop; a CPU restatement, NOT ESMF" % (reps, nlev, idx.shape[0]),
            "note": "weights from the GPU handle; GBs = algorithmic bytes per second; store_ms = the oracle's bilinear RegridStore once; "
                    "ESMF is unavailable here: do not read the ratio as a speed-up"}


if __name__ == "__main__":
    main()
