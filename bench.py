#!/usr/bin/env python3
"""Benchmark: Adam steps/s of the DAGMA linear inner loop on MI355X (BASELINE.json metric).

Default workload (every N): BASELINE config 4 -- d=1000, n=1e6 linear Gaussian
SEM, l2 loss, "data mode": X row-sharded over the N ranks, each step computes
Z_k = X_k^T (X_k (I - W)) on MFMA, all-reduces Z over RCCL/xGMI, then runs the
replicated log-det/inverse and fused Adam update.  Strong scaling (n fixed).

A plain run does what the headline needs and no more: it generates X, warms up, times --steps
steps and prints the JSON line (metric, value, unit, ms_per_step, ..., and sem_generator: the
GPU SEM generator's time for this rank's X shard, measured while setting up).  --dump-outputs DIR
also writes what the timed steps computed (W and the loop's counters) as DIR/<name>.npy, from
inputs that depend only on the arguments, so two builds can be compared output for output.

With --full, on rank 0 at N=1, it also reports (same run, same box)
  * value_check : every leg's W against the CPU oracle's run of the same steps;
  * cpu_baseline : the workload's own math (data-mode step) on the host cores, CPU oracle;
  * cpu_reference_algorithm / cov_mode : BASELINE config 2 (d=1000, n=1e4) with the
    reference's own algorithm (cov = X^T X / n once, O(d^3) per step) on the CPU and the GPU;
  * full_fit : DagmaLinear('l2').fit defaults at config 2, wall-clock (the metric's 2nd half);
  * config3 : d=5000, n=5e4 cov mode, with its CPU reference-algorithm baseline;
  * config5 : DagmaNonlinear Adam steps at dims [200, 10, 1], n=1000, with its CPU oracle;
  * roofline : the dominant data-mode GEMM vs the FP64 MFMA peak, PMC HBM traffic;
and at N > 1 the one-process device-group leg and the CPU baselines.  The --no-* options take
single legs out of a --full run.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

FP64_MFMA_PEAK_TF = 78.6    # MI355X dense FP64 matrix peak (spec)
HBM_PEAK_GBS = 8000.0       # MI355X HBM3E peak (spec; MI355X_MICROARCH.md)
# what only a --full run does (each also has its --no-* option)
FULL_ONLY_LEGS = ("cpu", "cov", "fit", "fit4", "large", "mlp", "small", "tcc", "logistic", "check", "group")


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--workload", choices=["data", "cov"], default="data")
    # (--dim / --rows: the same options under names torch.distributed.run does not take for
    # abbreviations of its own, e.g. --d for --duplicate-stdout-filters)
    p.add_argument("--d", "--dim", dest="d", type=int, default=1000)
    p.add_argument("--n", "--rows", dest="n", type=int, default=1_000_000)
    p.add_argument("--cov-n", type=int, default=10_000)
    p.add_argument("--cov-steps", type=int, default=2000)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--no-cpu", action="store_true")
    p.add_argument("--no-cov", action="store_true")
    p.add_argument("--profile-reps", type=int, default=3)
    p.add_argument("--no-fit", action="store_true", help="skip the full-fit wall-clock leg (config 2)")
    p.add_argument("--no-fit4", action="store_true", help="skip the config-4 full-fit leg (d=1000, n=1e6, cov mode "
                                                          "from the device / sharded X)")
    p.add_argument("--no-data", action="store_true", help="skip the data-mode leg (profiling the other legs)")
    p.add_argument("--no-large", action="store_true", help="skip the config 3 leg (d=5000, n=5e4, cov mode)")
    p.add_argument("--no-mlp", action="store_true", help="skip the config 5 leg (DagmaNonlinear, dims [200,10,1])")
    p.add_argument("--no-small", action="store_true", help="skip the config 1 leg (d=20, one persistent workgroup)")
    p.add_argument("--no-tcc", action="store_true", help="skip the TCC trek-regularizer leg (SURVEY 8f-3, d=20)")
    p.add_argument("--mlp-steps", type=int, default=2000)
    p.add_argument("--large-d", type=int, default=5000)
    p.add_argument("--large-n", type=int, default=50_000)
    p.add_argument("--large-steps", type=int, default=100)
    p.add_argument("--no-logistic", action="store_true", help="skip the logistic data-mode leg (SURVEY 8f-1)")
    p.add_argument("--logistic-steps", type=int, default=10)
    p.add_argument("--no-check", action="store_true", help="skip the value checks against the CPU oracle "
                   "(profiling runs)")
    p.add_argument("--no-group", action="store_true", help="skip the single-process device-group leg (ABI 11: "
                   "one process drives all N GPUs, DagmaLinear(devices=[...]))")
    p.add_argument("--group-leg", action="store_true", help=argparse.SUPPRESS)  # the leg's child process
    p.add_argument("--full", action="store_true", help="beside the headline: the value checks against the CPU "
                   "oracle, the CPU baselines, the per-kernel profile and roofline, and every other leg (configs 1, "
                   "2, 3, 5, TCC, logistic, the full fits, the device-group leg); off by default")
    p.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what they computed (W after "
                   "the last timed step, the loop's counters) as DIR/<name>.npy")
    args = p.parse_args()
    if not args.full:  # a plain run: the headline workload alone
        for leg in FULL_ONLY_LEGS:
            setattr(args, "no_" + leg, True)
    return args


def _free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def relaunch_ranks(args):
    """`python bench.py --gpus N` (N > 1) outside a launcher: start one rank per GPU under
    torch.distributed.run as a child process (no exec; nothing here has touched the GPU),
    relay its output (rank 0 prints the JSON line) and exit with its return code.  The ranks
    supervise their GPU workers themselves (supervise_ranks: the fallback to the host-driven
    all-reduce lives there, so it also covers an external launcher); this wait is only bounded
    (MIDAGMA_BENCH_TOTAL_S, default 2 h)."""
    import signal
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    log("launching:", " ".join(cmd))
    # its own session, so a timeout ends torchrun and its rank supervisors together (the workers
    # die with their supervisor: _run_worker's parent-death signal)
    p = subprocess.Popen(cmd, start_new_session=True)
    try:
        rc = p.wait(timeout=float(os.environ.get("MIDAGMA_BENCH_TOTAL_S", "7200")))
    except subprocess.TimeoutExpired:
        log("bench ranks exceeded MIDAGMA_BENCH_TOTAL_S")
        try:
            os.killpg(p.pid, signal.SIGKILL)
        except OSError:
            pass
        p.wait()
        rc = 124
    sys.exit(rc)


def _die_with_parent():
    """preexec_fn of a worker: SIGKILL when its supervisor dies (Linux PR_SET_PDEATHSIG), so a
    killed supervisor leaves no worker holding a GPU."""
    try:
        import ctypes
        import signal
        ctypes.CDLL("libc.so.6", use_errno=True).prctl(1, int(signal.SIGKILL), 0, 0, 0)
    except Exception:  # noqa: BLE001
        pass


def beat(what):
    """Worker progress mark for the rank supervisor (MIDAGMA_BENCH_HEARTBEAT): a stalled worker
    (a hung collective) is one whose file has not changed for MIDAGMA_BENCH_STALL_S."""
    p = os.environ.get("MIDAGMA_BENCH_HEARTBEAT")
    if p:
        with open(p, "a") as f:
            f.write(f"{time.time():.1f} {what}\n")


def _run_worker(cmd, env, hb, stall, cap, store, key):
    """One rank's GPU worker as a child process: its stdout and stderr relayed to this process's
    stderr (stdout lines kept: rank 0's JSON line), ended when it exits, stalls, overruns, or
    another rank's worker of the same attempt has failed (the store counter `key`).  Returns
    (outcome, stdout lines, last stderr lines); outcome "ok" or why it failed."""
    import signal
    import subprocess
    import threading
    p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         start_new_session=True, preexec_fn=_die_with_parent)
    out, err = [], []

    def pump(src, keep):
        for ln in src:
            keep.append(ln)
            sys.stderr.write(ln)
        sys.stderr.flush()
    th = [threading.Thread(target=pump, args=(p.stdout, out), daemon=True),
          threading.Thread(target=pump, args=(p.stderr, err), daemon=True)]
    for t in th:
        t.start()
    t0 = last = time.time()
    outcome = None
    while outcome is None:
        rc = p.poll()
        if rc is not None:
            # (a worker that failed only in teardown, after its last mark "done", finished its work)
            outcome = "ok" if rc == 0 or _last_mark(hb) == "done" else f"worker exited {rc}"
            break
        now = time.time()
        try:
            last = max(last, os.path.getmtime(hb))
        except OSError:
            pass
        if _last_mark(hb) == "done" and now - last > min(stall, 60.0):
            outcome = "ok"  # the worker finished its work (rank 0: the line is out) and hangs in teardown
            sys.stderr.write(f"bench worker still in teardown {now - last:.0f} s after its last mark: ended\n")
        elif now - last > stall:
            outcome = f"no progress for {stall:.0f} s (last mark: {_last_mark(hb)})"
        elif now - t0 > cap:
            outcome = f"still running after {cap:.0f} s"
        elif int(store.add(key, 0)) > 0:
            outcome = "stopped: another rank's worker failed"
        else:
            time.sleep(0.5)
    if p.poll() is None:
        try:
            os.killpg(p.pid, signal.SIGKILL)
        except OSError:
            pass
        p.wait()
    for t in th:
        t.join(timeout=10)
    if outcome != "ok" and not outcome.startswith("stopped"):
        store.add(key, 1)
    return outcome, [ln.rstrip("\n") for ln in out], [ln.rstrip("\n") for ln in err[-12:]]


def _last_mark(hb):
    try:
        with open(hb) as f:
            lines = f.read().strip().splitlines()
        return lines[-1].split(" ", 1)[1] if lines else "none"
    except OSError:
        return "none"


def supervise_ranks(args):
    """Under torch.distributed.run (WORLD_SIZE > 1) every rank process supervises one GPU worker
    (this script again, MIDAGMA_BENCH_WORKER=1) and never touches the GPU itself, so a failed or
    hung multi-GPU path cannot cost the line:
      * attempt 1: the in-library RCCL communicator (the all-reduce captured in the slot graphs);
      * if any rank's worker exits non-zero, makes no progress for MIDAGMA_BENCH_STALL_S (300 s)
        or runs past MIDAGMA_BENCH_ATTEMPT_S (1800 s), every worker of the attempt is killed and
        attempt 2 runs fresh workers on the host-driven path (MIDAGMA_BENCH_COMM=host:
        step_partial -> dist.all_reduce -> step_finish), on a fresh rendezvous port;
      * rank 0 then times the CPU baseline on the host cores (no GPU; the workers are gone) and
        prints the JSON line with the path taken and every failed attempt (`launch`).
    The supervisors talk over gloo (CPU) on torchrun's own rendezvous; the workers build their own
    process group on the port rank 0 picks."""
    import datetime
    import torch
    import torch.distributed as dist
    world, rank = int(os.environ["WORLD_SIZE"]), int(os.environ["RANK"])
    dist.init_process_group("gloo", timeout=datetime.timedelta(hours=3))
    store = dist.distributed_c10d._get_default_store()
    stall = float(os.environ.get("MIDAGMA_BENCH_STALL_S", "300"))
    cap = float(os.environ.get("MIDAGMA_BENCH_ATTEMPT_S", "1800"))
    first = os.environ.get("MIDAGMA_BENCH_COMM", "library")
    if os.environ.get("MIDAGMA_BENCH_BACKEND", "nccl") != "nccl":
        paths = ["host"]  # (gloo: the workers take the host-driven all-reduce, bench_data)
    else:
        paths = ["host"] if first == "host" else ["library", "host"]
    fake = os.environ.get("MIDAGMA_BENCH_WORKER_CMD")  # tests: a stand-in worker (JSON argv)
    cmd = json.loads(fake) if fake else [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]
    import tempfile
    td = tempfile.mkdtemp(prefix=f"midagma_bench_r{rank}_")
    attempts, line, cov_out = [], None, None
    for a, path in enumerate(paths):
        port = [_free_port() if rank == 0 else None]
        dist.broadcast_object_list(port, src=0)
        hb = os.path.join(td, f"heartbeat{a}")
        cov_out = os.path.join(td, f"cov{a}.npy")
        env = dict(os.environ, MIDAGMA_BENCH_WORKER="1", MASTER_PORT=str(port[0]),
                   TORCHELASTIC_USE_AGENT_STORE="False", MIDAGMA_BENCH_COMM=path, MIDAGMA_BENCH_HEARTBEAT=hb,
                   MIDAGMA_BENCH_COV_OUT=cov_out)
        t0 = time.time()
        outcome, out, err = _run_worker(cmd, env, hb, stall, cap, store, f"attempt{a}_failed")
        fails = torch.tensor([0 if outcome == "ok" else 1])
        dist.all_reduce(fails)
        per_rank = [None] * world if rank == 0 else None
        dist.gather_object({"rank": rank, "outcome": outcome, "stderr_tail": err[-6:] if outcome != "ok" else []},
                           per_rank, dst=0)
        rec = {"comm_path": path, "failed_ranks": int(fails.item()), "seconds": round(time.time() - t0, 1)}
        if rank == 0 and int(fails.item()):
            rec["ranks"] = [r for r in per_rank if r["outcome"] != "ok"]
        attempts.append(rec)
        if int(fails.item()) == 0:
            if rank == 0:
                js = [x for x in out if x.startswith("{")]
                line = json.loads(js[-1]) if js else None
            break
        log(f"bench attempt {a} ({path}) failed on {int(fails.item())} rank(s): {outcome}")
    rc = 0
    if rank == 0:
        if line is None:
            line = {"metric": "Adam steps/s, d=1000 linear DAGMA (l2, data mode)", "value": None, "unit": "steps/s",
                    "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "higher_is_better": True,
                    "verified": False, "error": "every multi-GPU attempt failed (see launch.attempts)"}
            rc = 1
        # the path the successful workers report they ran (bench_data's comm["path_kind"]); the
        # attempts list keeps what each attempt asked for
        ran = None
        if line.get("value"):
            ran = (line.get("comm") or {}).get("path_kind") or attempts[-1]["comm_path"]
            attempts[-1]["ran"] = ran
        line["launch"] = {"supervised": True, "comm_path": ran, "attempts": attempts,
                          "note": "each rank process ran its GPU work in a worker child; a failed or stalled "
                                  "attempt was killed on every rank and the next path started fresh; comm_path is "
                                  "the path the successful workers ran, attempts[].comm_path the one each asked for"}
        if isinstance(line.get("comm"), dict):
            line["comm"]["path_taken"] = ran
        if line.get("value") and not args.no_group and os.environ.get("MIDAGMA_BENCH_SAME_DEVICE") != "1":
            # the same workload from ONE process driving all the GPUs (ABI 11), now that the
            # workers are gone; the other ranks wait at the barrier below
            line["single_process"] = run_group_leg(args, world)
        if line.get("value") and not args.no_cpu and os.path.exists(cov_out):
            cpu = cpu_baseline(args, np.load(cov_out))
            attach_cpu(line, cpu, line["value"])
        print(json.dumps(line), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    return rc


def setup_dist(args):
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # rehearsal knobs (default off): every rank on cuda:0 and a gloo all-reduce, so the N > 1
    # path runs end to end on a one-GPU box; the driver's runs use one GPU per rank over RCCL
    if os.environ.get("MIDAGMA_BENCH_SAME_DEVICE") == "1":
        local = 0
    backend = os.environ.get("MIDAGMA_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(local)
    if world > 1:
        if backend == "nccl":
            # ring all-reduce hands every rank the same bits, so the replicated controllers
            # decide identically; RCCL's other algorithms need not
            os.environ.setdefault("NCCL_ALGO", "Ring")
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    if world != args.gpus:
        log(f"warning: --gpus {args.gpus} but WORLD_SIZE={world}; using WORLD_SIZE")
    return world, rank, local


def make_shard(d, n, world, rank, seed, device, sem="gauss"):
    """This rank's rows of an ER(s0=d) linear-Gaussian SEM, generated on the GPU by the
    library's SEM generator (csrc/sem.hip, counter-based noise: the shard is exactly the
    rank's rows of the unsharded X).  Returns (X, n_k, generation seconds)."""
    import torch
    from midagma_amd.simulate import simulate_er_dag, simulate_weights
    from midagma_amd.utils import simulate_linear_sem_gpu
    rng = np.random.default_rng(seed)
    W_true = simulate_weights(simulate_er_dag(d, d, rng), rng)
    base, extra = divmod(n, world)
    n_k = base + (1 if rank < extra else 0)
    row0 = rank * base + min(rank, extra)
    dev_index = device.index if hasattr(device, "index") else device
    # one tiny call first: the process's first launch of the library's kernels loads its code
    # object, a one-time cost that is not the generator's
    simulate_linear_sem_gpu(W_true, n, sem, seed=seed * 1000003 + 17, device=dev_index, row0=row0,
                            n_rows=min(n_k, 256))
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    X = simulate_linear_sem_gpu(W_true, n, sem, seed=seed * 1000003 + 17, device=device.index
                                if hasattr(device, "index") else device, row0=row0, n_rows=n_k)
    torch.cuda.synchronize(device)
    return X, n_k, time.perf_counter() - t0


def comm_summary(ar_ms, ar_ms_min, ms_per_step, nbytes, world, backend):
    """The N > 1 line's communication breakdown: the all-reduce's device time per step (hipEvents
    on the solver stream, mean over the timed steps, max and min over ranks), the rest of the
    step, and the achieved bandwidth of the score-partial all-reduce."""
    algbw = nbytes / (ar_ms * 1e-3) / 1e9 if ar_ms > 0 else None
    out = {"allreduce_ms": ar_ms, "allreduce_ms_min_rank": ar_ms_min, "compute_ms": ms_per_step - ar_ms,
           "allreduce_frac": ar_ms / ms_per_step if ms_per_step > 0 else None, "bytes": int(nbytes),
           "algbw_GBps": algbw, "busbw_GBps": None if algbw is None else algbw * 2.0 * (world - 1) / world,
           "timing": "hipEvents around dist.all_reduce on the solver stream, mean over the timed steps, max over "
                     "ranks; compute_ms = ms_per_step - allreduce_ms; busbw = algbw * 2(N-1)/N (ring)",
           "backend": backend, "world_size": world,
           "NCCL_ALGO": os.environ.get("NCCL_ALGO"), "NCCL_PROTO": os.environ.get("NCCL_PROTO")}
    try:
        import torch
        out["rccl_version"] = ".".join(str(x) for x in torch.cuda.nccl.version())
    except Exception:  # noqa: BLE001
        out["rccl_version"] = None
    return out


def allreduce_(t, op=None):
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(t, op=op or dist.ReduceOp.SUM)
    return t


def bench_data(args, world, rank, local):
    import torch
    import torch.distributed as dist
    from midagma_amd.solver import HipSolver
    dev = torch.device("cuda", local)
    d, n = args.d, args.n
    X, n_k, t_gen = make_shard(d, n, world, rank, args.seed, dev)
    colsum = allreduce_(X.sum(0))
    X -= colsum / n                      # l2 centers X with the global mean (linear.py:411)
    torch.cuda.synchronize()
    s = HipSolver(d, "l2", "data", device=local)
    s.set_data(X, n_global=n)
    del X
    torch.cuda.empty_cache()
    beat("data shard resident")
    allreduce = None
    comm = None
    # N > 1 over RCCL: the solver's own communicator (ABI 7), the score all-reduce captured in the
    # replayed slot graphs and the loop driven by run_slots; gloo (the one-GPU rehearsal) and
    # MIDAGMA_BENCH_COMM=host: the host-driven step_partial -> dist.all_reduce -> step_finish
    lib_comm = world > 1 and dist.get_backend() == "nccl" and os.environ.get("MIDAGMA_BENCH_COMM", "library") == "library"
    ext = torch.cuda.ExternalStream(s.stream, device=dev)
    if lib_comm:
        s.attach_comm()
    elif world > 1:
        zt = torch.zeros(s.zbuf_len, dtype=torch.float64, device=dev)
        s.bind_zbuf(zt.data_ptr(), zt.numel())
        # hipEvents around every all-reduce on the solver stream (the stream it runs on):
        # the communication share of the step, averaged over the timed steps
        ev = []

        def allreduce(timed=False):
            with torch.cuda.stream(ext):
                if timed:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    dist.all_reduce(zt)
                    b.record()
                    ev.append((a, b))
                else:
                    dist.all_reduce(zt)
    K, Wm = args.steps, args.warmup
    s.begin(np.zeros((d, d)), 1.0, Wm + K + 64, 1.0, 3e-4, tol=-1.0, lambda1=0.03)

    host_enqueue = []

    def steps(m, timed=False):
        if allreduce is None:
            t_ = time.perf_counter()
            s.run_slots(m)
            if timed:
                host_enqueue.append(time.perf_counter() - t_)
        else:
            for _ in range(m):
                s.step_partial()
                allreduce(timed)
                s.step_finish()

    steps(Wm)
    s.sync()
    beat("warm-up steps done")
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps(K, timed=True)
    s.sync()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t1 = time.perf_counter()
    beat("timed steps done")
    r = s.poll()
    elapsed = torch.tensor([t1 - t0], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    elapsed = float(elapsed.item())
    ok = (r.status == 0 and r.iters == Wm + K)
    Wf = np.zeros((d, d))
    s.end(Wf)
    replicas = None
    if world > 1:
        if lib_comm:
            # the in-graph all-reduce is not separable inside the replayed slot: the same in-place
            # all-reduce of the score buffer timed alone, eagerly, on the solver stream
            with torch.cuda.stream(ext):
                for _ in range(3):
                    s.comm_allreduce_zbuf()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(20):
                    s.comm_allreduce_zbuf()
                b.record()
            b.synchronize()
            ev = [(a, b)]
            ar_scale = 1.0 / 20
        else:
            ar_scale = 1.0
        ar_ms = float(np.mean([a.elapsed_time(b) for a, b in ev])) * ar_scale
        t = torch.tensor([ar_ms, -ar_ms], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        ar_max, ar_min = float(t[0]), -float(t[1])
        comm = comm_summary(ar_max, ar_min, elapsed / K * 1e3, 8 * s.zbuf_len, dist.get_world_size(),
                            dist.get_backend())
        comm["path"] = ("in-library RCCL communicator: the all-reduce captured in the replayed slot graph, run_slots "
                        "drives the loop (allreduce_ms: the same all-reduce timed alone, 20 eager calls)" if lib_comm
                        else "host-driven: step_partial -> dist.all_reduce on the solver stream -> step_finish, "
                             "one Python round per step")
        if lib_comm and host_enqueue:
            comm["host_enqueue_ms_per_step"] = sum(host_enqueue) / K * 1e3
        # the rank count the in-library RCCL communicator itself reports (midagma_comm_ranks)
        comm["rccl_ranks"] = s.comm_ranks if lib_comm else None
        comm["path_kind"] = "library" if lib_comm else "host"
        # W must be bit-identical on every rank: compare (sum, sum of squares) over ranks
        v = np.array([Wf.sum(), (Wf * Wf).sum()])
        t = torch.tensor(np.concatenate([v, -v]), dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        m = t.cpu().numpy()
        replicas = bool(m[0] == -m[2] and m[1] == -m[3])
        ok = ok and replicas
    out = dict(ms_per_step=elapsed / K * 1e3, value=K / elapsed, verified_iters=int(r.iters), verified=ok,
               n_local=n_k, prof=None, D=s.D, sem_gen_s=t_gen, replicas_identical=replicas, comm=comm,
               W=Wf, cov=None, steps_total=Wm + K,
               loop_state=np.array([r.iters, r.status, r.halvings, r.lr_final], dtype=np.float64))
    if not getattr(args, "full", True):  # a plain run ends with its timed steps
        s.close()
        return out
    # value check: cov = X^T X / n of the same (centered, sharded) X from the device Gram,
    # all-reduced over ranks; rank 0 runs the oracle's reference algorithm on it (linear.py:244)
    s.data_gram()
    if lib_comm:
        s.comm_allreduce_zbuf()
    elif world > 1:
        with torch.cuda.stream(ext):
            dist.all_reduce(zt)
    s.cov_from_zbuf(float(n))
    cov = s.get_cov() if rank == 0 else None
    # the per-kernel profile below runs rank 0's kernels alone (no all-reduce): restart from the
    # final W so it times the same matrices
    s.begin(Wf, 1.0, 64, 1.0, 3e-4, tol=-1.0, lambda1=0.03)
    # (with the in-library communicator the profiled slot graph carries the all-reduce: every rank
    # replays it the same number of times, rank 0 reports)
    prof = s.profile_parts(args.profile_reps) if (rank == 0 or lib_comm) else {}
    if rank != 0:
        prof = {}
    beat("data leg profiled")
    out.update(prof=prof, cov=cov)
    s.close()
    return out


def bench_group(args, ndev):
    """The headline workload (config 4: d=1000, n=1e6, l2, data mode) from ONE process driving
    `ndev` GPUs (ABI 11, midagma_amd.solver.HipGroup): member k holds rank k's rows
    (generated on device k), an RCCL communicator per device from ncclCommInitAll, the score
    all-reduce captured in each member's slot graphs, one library thread per device.  Timed: one
    group minimize of --steps Adam steps from W = 0 (mu=1, s=1, lr=3e-4, tol=-1), after a warm-up
    call that sizes the tables and captures the graphs.  Runs in a child process of its own
    (`--group-leg`), so its RCCL state is separate from the ranks'."""
    import torch
    from midagma_amd.solver import HipGroup
    d, n, K = args.d, args.n, args.steps
    shards, t_gen = [], 0.0
    for k in range(ndev):
        X, n_k, t = make_shard(d, n, ndev, k, args.seed, torch.device("cuda", k))
        shards.append(X)
        t_gen = max(t_gen, t)
    dev0 = shards[0].device
    colsum = sum(X.sum(0).to(dev0) for X in shards)     # the global column sums (linear.py:411)
    for X in shards:
        X -= (colsum / n).to(X.device)
    for X in shards:
        if X.is_cuda:
            torch.cuda.synchronize(X.device)
    t0 = time.perf_counter()
    g = HipGroup(d, "l2", devices=list(range(ndev)))
    t_create = time.perf_counter() - t0
    for k, X in enumerate(shards):
        g.members[k].set_data(X, n_global=n)
    del shards, X
    torch.cuda.empty_cache()
    W = np.zeros((d, d))
    # warm-up: tables sized for K steps and the graphs captured (stops at its first checkpoint,
    # iteration 1: |dobj / 1e16| <= 1e300)
    g.minimize(W, 1.0, K, 1.0, 3e-4, tol=1e300, lambda1=0.03, checkpoint=1)
    # a short call of K1 steps first: (t_K - t_K1) / (K - K1) is the per-step cost without the
    # call's fixed part (threads, begin, the W download and replica check), which the one-process-
    # per-GPU line's timed region does not contain either
    K1 = max(1, K // 5)
    W = np.zeros((d, d))
    t0 = time.perf_counter()
    g.minimize(W, 1.0, K1, 1.0, 3e-4, tol=-1.0, lambda1=0.03, checkpoint=1000)
    el1 = time.perf_counter() - t0
    W = np.zeros((d, d))
    t0 = time.perf_counter()
    r = g.minimize(W, 1.0, K, 1.0, 3e-4, tol=-1.0, lambda1=0.03, checkpoint=1000)
    el = time.perf_counter() - t0
    per = (el - el1) / (K - K1) if K > K1 else el / K
    out = dict(value=1.0 / per, unit="steps/s", ms_per_step=per * 1e3, steps=K, n_gpus=ndev, iters=int(r.iters),
               call_ms=el * 1e3, call_steps_per_s=K / el, short_call_ms=el1 * 1e3, short_call_steps=K1,
               call_fixed_ms=(el - per * K) * 1e3,
               verified=bool(r.iters == K and r.success and np.isfinite(W).all()), rccl_ranks=g.comm_ranks,
               emulated=g.emulated, group_create_s=t_create, sem_gen_s=t_gen,
               workload=f"config4: d={d}, n={n}, l2, data mode, rows sharded over {ndev} GPU(s) of ONE process",
               path=("midagma_group (ABI 11): one process, ncclCommInitAll over the devices, the score all-reduce "
                     "captured in every member's slot graphs, one library thread per device; the members' W bits "
                     "and states checked equal at the end"),
               timing="(t(steps) - t(steps // 5)) / (steps - steps // 5) over two HipGroup.minimize calls from W = 0 "
                      "(wall clock; call_ms / call_steps_per_s: the long call whole, begin, replayed slots, the final "
                      "W download and replica check included)")
    g.close()
    return out


def run_group_leg(args, ndev, timeout=None):
    """bench_group in a child process (no launcher environment): its JSON, or the failure."""
    import subprocess
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "GROUP_RANK", "ROLE_RANK",
                        "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID", "MIDAGMA_BENCH_WORKER",
                        "MIDAGMA_BENCH_HEARTBEAT")}
    env.setdefault("NCCL_ALGO", "Ring")
    cmd = [sys.executable, os.path.abspath(__file__), "--group-leg", "--gpus", str(ndev), "--steps", str(args.steps),
           "--d", str(args.d), "--n", str(args.n), "--seed", str(args.seed)]
    timeout = timeout or float(os.environ.get("MIDAGMA_BENCH_GROUP_S", "900"))
    t0 = time.time()
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    except subprocess.TimeoutExpired:
        return {"verified": False, "error": f"group leg did not finish in {timeout:.0f} s"}
    js = [x for x in r.stdout.splitlines() if x.startswith("{")]
    if r.returncode != 0 or not js:
        return {"verified": False, "error": f"group leg exited {r.returncode}", "stderr_tail": r.stderr[-1500:]}
    out = json.loads(js[-1])
    out["child_wall_s"] = round(time.time() - t0, 1)
    return out


def bench_cov(args, device):
    from midagma_amd.simulate import make_dataset
    from midagma_amd.solver import HipSolver
    d, n = args.d, args.cov_n
    X, _, _ = make_dataset(d, n, seed=args.seed)
    X -= X.mean(0, keepdims=True)
    cov = X.T @ X / float(n)
    s = HipSolver(d, "l2", "cov", device=device)
    s.set_cov(cov)
    K = args.cov_steps
    s.begin(np.zeros((d, d)), 1.0, K + 100, 1.0, 3e-4, tol=-1.0, lambda1=0.03)
    s.run_slots(20)
    s.sync()
    t0 = time.perf_counter()
    s.run_slots(K)
    s.sync()
    t1 = time.perf_counter()
    r = s.poll()
    W = np.zeros((d, d))
    s.end(W)
    prof = {}
    if getattr(args, "full", True):
        s.begin(W, 1.0, 1000, 1.0, 3e-4, tol=-1.0, lambda1=0.03)
        prof = s.profile_parts(20)
    s.close()
    return dict(value=K / (t1 - t0), ms_per_step=(t1 - t0) / K * 1e3, steps=K, verified=(r.status == 0 and
                r.iters == K + 20), prof=prof, cov=cov, W=W, steps_total=K + 20,
                loop_state=np.array([r.iters, r.status, r.halvings, r.lr_final], dtype=np.float64))


_MLP_CPU_CHILD = r"""
import json, sys, time
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from oracle.mlp_oracle import OracleMLP, load_params, nonlinear_minimize
th, d, n = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
torch.set_num_threads(th)
P = np.load(sys.argv[5])
m = OracleMLP([d, 10, 1])
load_params(m, {k: P[k] for k in P.files if k != "X"})
X = torch.from_numpy(P["X"])
nonlinear_minimize(m, X, 2, 2e-4, 0.02, 0.005, 0.1, 1.0, tol=-1)
K = 20
t0 = time.perf_counter()
ok, it = nonlinear_minimize(m, X, K, 2e-4, 0.02, 0.005, 0.1, 1.0, tol=-1, checkpoint=10 ** 9)
assert ok and it == K, (ok, it)
print(json.dumps({"t": (time.perf_counter() - t0) / K}))
"""


def bench_mlp(args, device, with_cpu):
    """Config 5 (BASELINE): DagmaNonlinear Adam steps at dims [200, 10, 1], n=1000 -- the
    reference's minimize loop in PyTorch-ROCm with the HIP log-det h_func; replicas only
    (SURVEY 8e).  CPU: the oracle restatement (torch CPU, slogdet) in child processes."""
    import subprocess
    import tempfile
    import torch
    from midagma_amd.nonlinear import DagmaMLP, DagmaNonlinear
    from midagma_amd.simulate import make_dataset
    d, n = 200, 1000
    X, _, _ = make_dataset(d, n, seed=args.seed)
    torch.manual_seed(args.seed)
    model = DagmaMLP(dims=[d, 10, 1]).to(torch.device("cuda", device))
    with torch.no_grad():
        model.fc1.weight.normal_(0, 0.3 / np.sqrt(10 * d))
    params = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items() if k != "I"}
    K = args.mlp_steps
    Xd = torch.from_numpy(X).to(torch.device("cuda", device))
    dn = DagmaNonlinear(model, device=device)
    dn.X = Xd
    dn.checkpoint = 10 ** 9
    dn.minimize(20, 2e-4, 0.02, 0.005, 0.1, 1.0, tol=-1)
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    ok = dn.minimize(K, 2e-4, 0.02, 0.005, 0.1, 1.0, tol=-1)
    torch.cuda.synchronize(device)
    dt = time.perf_counter() - t0
    final = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items() if k in params}
    out = dict(value=K / dt, unit="steps/s", ms_per_step=dt / K * 1e3, steps=K, verified=bool(ok),
               workload="config5: DagmaNonlinear.minimize, DagmaMLP dims [200, 10, 1], n=1000, 1 GPU "
                        "(the reference's loop; objective as fused HIP kernels: fc1 terms, warm-started log-det, MLP "
                        "tail, scalar objective, multi-tensor Adam; fc1 GEMMs on rocBLAS; the step replayed as a "
                        "hipGraph; the timed minimize call includes its own graph capture; untimed warm-up: the 20-step "
                        "call the timed one continues)")
    if getattr(dn, "_ld", None) is not None:
        steps_ld, exact_ld = dn._ld.stats()
        out["logdet"] = {"steps": steps_ld, "gauss_jordan_steps": exact_ld,
                         "note": "steps of the timed call whose log-det ran the Gauss-Jordan chain (the first and the "
                                 "last, whose objective the loop reads, plus any whose warm-started inverse was not "
                                 "certified); the rest took the product-form series"}
    # Value check: the reference's MLP trajectory is itself chaotic past a few hundred steps (a
    # 1e-15 relative change of the initial parameters moves them by 4e-4 at step 1020 and 6e-3 at
    # 2020 in the oracle; tools/mlp_chaos.py, profiles/r03_mlp_chaos.log), so the 1e-9 comparison
    # runs a separate 20 + 300-step replay of the same path (graphs, warm-started log-det) from
    # the same parameters; the timed window's own deviation is reported beside it.
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if k in params:
                v.copy_(torch.from_numpy(params[k]))
    dn2 = DagmaNonlinear(model, device=device)
    dn2.X = dn.X
    dn2.checkpoint = 10 ** 9
    dn2.minimize(20, 2e-4, 0.02, 0.005, 0.1, 1.0, tol=-1)
    dn2.minimize(300, 2e-4, 0.02, 0.005, 0.1, 1.0, tol=-1)
    torch.cuda.synchronize(device)
    final_check = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items() if k in params}
    out["_check"] = dict(params=params, X=X, calls=[20, 300], final=final_check, timed_calls=[20, K],
                         timed_final=final)
    if with_cpu:
        best = None
        phys = host_cpus()["physical_cores"]
        sweep = {}
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "mlp.npz")
            np.savez(path, X=X, **params)
            for th in thread_sweep(phys):
                env = dict(os.environ, OMP_NUM_THREADS=str(th), HIP_VISIBLE_DEVICES="")
                try:
                    r = subprocess.run([sys.executable, "-c", _MLP_CPU_CHILD, REPO, str(th), str(d), str(n), path],
                                       capture_output=True, text=True, timeout=600, env=env)
                    t = json.loads(r.stdout.strip().splitlines()[-1])["t"]
                    log(f"cpu oracle MLP d={d}: {1 / t:.1f} steps/s at {th} threads")
                    sweep[str(th)] = 1.0 / t
                    if best is None or t < best[0]:
                        best = (t, th)
                except Exception as e:  # noqa: BLE001
                    log(f"cpu oracle MLP at {th} threads failed: {e!r}")
        if best is not None:
            out["cpu_baseline"] = dict(value=1.0 / best[0], unit="steps/s", cores=best[1], kind="port", note=PORT_NOTE,
                                       physical_cores=phys, sweep=sweep,
                                       sample="oracle DagmaNonlinear.minimize (torch CPU, slogdet h_func as "
                                              f"nonlinear.py:84), 20 steps per thread count, threads "
                                              f"{thread_sweep(phys)}, best shown")
            out["vs_cpu"] = out["value"] * best[0]
    return out


def bench_logistic(args, device, n, steps):
    """the logistic loss in data mode at full speed (linear.py:245-246):
    per step expit(X W) in the epilogue of the X W GEMM (EPI_SIGMOID), then X^T S, on 1 GPU.
    X: a logistic SEM (Bernoulli rows) from the GPU generator; cov = X^T X / n from the device
    Gram (linear.py:428; logistic does not centre X)."""
    import torch
    from midagma_amd.solver import HipSolver
    d = args.d
    dev = torch.device("cuda", device)
    X, n_k, _ = make_shard(d, n, 1, 0, args.seed + 7, dev, sem="logistic")
    # the value check's copy of X (n = 1e6: 8 GB of host memory, freed after the check)
    Xh = X.cpu().numpy() if (n <= 100_000 or not args.no_check) else None
    s = HipSolver(d, "logistic", "data", device=device)
    s.set_data(X, n_global=n)
    del X
    torch.cuda.empty_cache()
    s.data_gram()
    s.cov_from_zbuf(float(n))
    s.begin(np.zeros((d, d)), 1.0, steps + 64, 1.0, 3e-4, tol=-1.0, lambda1=0.03)
    s.run_slots(3)
    s.sync()
    t0 = time.perf_counter()
    s.run_slots(steps)
    s.sync()
    t1 = time.perf_counter()
    r = s.poll()
    prof = s.profile_parts(3)
    check = None
    if Xh is not None:
        # n = 1e4: 20 steps; n = 1e6: 2 steps (an oracle step there takes ~10 s) on the one-pass
        # sigmoid kernel, where W = 0 makes the first gradient exact and the envelope ~0, so the
        # bar is 1e-9 (the floor) unless the reference's own order envelope is wider
        Kc = 20 if n <= 100_000 else 2
        Wc = np.zeros((d, d))
        s.minimize(Wc, 1.0, Kc, 1.0, 3e-4, tol=-1.0, lambda1=0.03)
        check = dict(W=Wc, X=Xh, cov=s.get_cov(), K=Kc, floor=1e-5 if n <= 100_000 else 1e-9,
                     threads=8 if n <= 100_000 else 16)
    sig_form = s.debug_sig_split()
    s.close()
    flops = 2.0 * n * d * d
    t_sig = prof["gemm_xw"] * 1e-3
    return dict(value=steps / (t1 - t0), unit="steps/s", ms_per_step=(t1 - t0) / steps * 1e3, steps=steps,
                verified=(r.status == 0 and r.iters == steps + 3),
                workload=f"logistic: d={d}, n={n}, data mode (X W GEMM with the sigmoid epilogue, X^T S), 1 GPU",
                kernel_ms={k: round(v, 4) for k, v in prof.items()},
                sigmoid_gemm={"kernel": "gemm_pipe_kernel<1, 0, 1> (EPI_SIGMOID)" if sig_form == 1 else
                              "gemm_pipe_kernel<1, 0, 7> (EPI_SIGMOID_SPLIT: two serial K halves)",
                              "ms": prof["gemm_xw"],
                              "achieved_tflops": flops / t_sig / 1e12 if t_sig > 0 else None,
                              "frac_fp64_peak": flops / t_sig / 1e12 / FP64_MFMA_PEAK_TF if t_sig > 0 else None,
                              "algorithmic": f"2*n*d^2 = {flops:.3e} flop + n*d sigmoids"}, _check=check)


def bench_small(args, device, with_cpu):
    """Config 1 (BASELINE): d=20, n=1000, l2, cov mode -- the one-workgroup persistent kernel
    (csrc/small.hip).  Steps/s over a 20000-step window (stage 1: mu=1, s=1, lr=3e-4, tol=-1)
    and the default fit() wall-clock; the CPU oracle (the reference's algorithm, bit-exact to
    it at 1 BLAS thread) timed beside it on the same host."""
    from midagma_amd import DagmaLinear
    from midagma_amd.simulate import count_accuracy, make_dataset
    from midagma_amd.solver import HipSolver
    d, n, K = 20, 1000, 20000
    X, W_true, B_true = make_dataset(d, n, seed=args.seed)
    Xc = X - X.mean(0, keepdims=True)
    cov = Xc.T @ Xc / float(n)
    s = HipSolver(d, "l2", "cov", device=device)
    s.set_cov(cov)
    s.begin(np.zeros((d, d)), 1.0, K + 100, 1.0, 3e-4, tol=-1.0, lambda1=0.03)
    s.run_slots(20)
    s.sync()
    t0 = time.perf_counter()
    s.run_slots(K)
    s.sync()
    t1 = time.perf_counter()
    r = s.poll()
    Wt = np.zeros((d, d))
    s.end(Wt)
    s.close()
    DagmaLinear("l2", device=device).fit(X.copy(), lambda1=0.03)   # warm: code objects
    m = DagmaLinear("l2", device=device)
    f0 = time.perf_counter()
    W = m.fit(X.copy(), lambda1=0.03)
    wall = time.perf_counter() - f0
    iters = [e["iters"] for e in m.minimize_log]
    out = dict(value=K / (t1 - t0), unit="steps/s", ms_per_step=(t1 - t0) / K * 1e3, steps=K,
               verified=(r.status == 0 and r.iters == K + 20),
               workload="config1: d=20, n=1000, l2, cov mode, 1 GPU (one persistent workgroup, csrc/small.hip)",
               fit={"wall_s": wall, "total_iters": int(sum(iters)), "stage_iters": iters,
                    "accuracy": count_accuracy(B_true, W != 0)},
               reference_survey={"steps_per_s": 16430, "fit_wall_s": 3.13,
                                 "source": "BASELINE.md survey probe (the reference itself, 8-vCPU survey host)"})
    out["_check"] = dict(W=Wt, cov=cov, K=K + 20, X=X, W_fit=W, stage_iters=iters)
    if with_cpu:
        import tempfile
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "cov.npy")
            np.save(path, cov)
            t = _cpu_runs("cov", d, path, [1, 4], steps=2000)
        if t:
            th, v = _best(t)
            out["cpu_baseline"] = dict(value=v, unit="steps/s", cores=th, kind="port", note=PORT_NOTE,
                                       sweep={str(k): 1.0 / x for k, x in sorted(t.items())},
                                       sample="oracle cov-mode Adam steps at d=20: 2000 steps per thread count, "
                                              "threads [1, 4], best shown")
            out["vs_cpu"] = out["value"] / v
        tf = _cpu_runs("fit", d, n, [1], steps=1, timeout=300)
        if tf:
            out["fit"]["cpu_fit_wall_s"] = tf[1]
            out["fit"]["vs_cpu"] = tf[1] / wall
    return out


def bench_tcc(args, device, with_cpu):
    """the TCC trek regularizer inside the loop (notreks.trek_value_grad with its defaults:
    spectral penalty, 'approx_trek_graph', Perron pairs of A = [[W o W, S], [I, (W o W)^T]]) at d=20,
    config 1's data, 'opt' mode on 30 % of the upper pairs, weight 0.1: steps/s over 2000 Adam steps
    (csrc/tcc.hip: the one-workgroup Noda / Gauss-Jordan kernel), the CPU oracle's step with the same
    regularizer (numpy eig, as the reference) timed beside it, and a separate 200-step run from
    W = 0 checked against the oracle."""
    from midagma_amd.simulate import make_dataset
    from midagma_amd.solver import HipSolver
    d, n, K, Kc, weight = 20, 1000, 2000, 200, 0.1
    X, _, _ = make_dataset(d, n, seed=args.seed)
    Xc = X - X.mean(0, keepdims=True)
    cov = Xc.T @ Xc / float(n)
    rng = np.random.default_rng(args.seed)
    iu = np.array(np.triu_indices(d, 1)).T
    pairs = iu[rng.uniform(size=len(iu)) < 0.3]
    s = HipSolver(d, "l2", "cov", device=device)
    s.set_cov(cov)
    s.set_trek_tcc(pairs, mode="opt", weight=weight)
    s.begin(np.zeros((d, d)), 1.0, K + 100, 1.0, 3e-4, tol=-1.0, lambda1=0.03)
    s.run_slots(20)
    s.sync()
    t0 = time.perf_counter()
    s.run_slots(K)
    s.sync()
    t1 = time.perf_counter()
    r = s.poll()
    Wc = np.zeros((d, d))
    rc = s.minimize(Wc, 1.0, Kc, 1.0, 3e-4, tol=-1.0, lambda1=0.03, checkpoint=10 ** 9)
    s.close()
    ms = (t1 - t0) / K * 1e3
    out = dict(value=K / (t1 - t0), unit="steps/s", ms_per_step=ms, steps=K,
               verified=(r.status == 0 and r.iters == K + 20 and rc.iters == Kc),
               workload=f"f3: cov-mode loop at d={d}, n={n} (config 1's data) with the TCC regularizer in 'opt' mode, "
                        f"{len(pairs)} pairs (30 % of the upper triangle), weight {weight}, 1 GPU",
               reference_ms_per_step={"value": 1.33, "source": "the reference's minimize with the same regularizer, "
                                      "one thread, measured in the build container (DESIGN.md section 4)"})
    out["_check"] = dict(W=Wc, cov=cov, pairs=pairs, K=Kc, weight=weight)
    out["larger"] = [bench_tcc_larger(args, device, dd, warm, k) for dd, warm, k in ((100, 2000, 300), (1000, 200, 40))]
    if with_cpu:
        import tempfile
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "tcc.npz")
            np.savez(path, cov=cov, pairs=pairs, weight=weight)
            t = _cpu_runs("tcc", d, path, [1], steps=300)
        if t:
            th, v = _best(t)
            out["cpu_baseline"] = dict(value=v, unit="steps/s", cores=th, kind="port", note=PORT_NOTE,
                                       sample=f"oracle cov-mode Adam steps at d={d} with the TCC regularizer "
                                              f"(numpy eig of A and A^T each step, as the reference): 300 steps, 1 thread")
            out["vs_cpu"] = out["value"] / v
    return out


def bench_tcc_larger(args, device, d, warm, K):
    """TCC at 2d > 128 (the launch-chain form with the fixed-shift stage, csrc/tcc.hip): per Adam
    step from W = 0 (the first K steps, where the Perron gap is smallest) and later in the same call
    (K steps after `warm` more; slots run in batches of 8 until the step count is reached, so the
    time includes each hand-back's re-run), with the fast slots handed back in each window.  Timing only: the
    TCC GPU tier checks this path against the oracle (tests/test_gpu_tcc.py)."""
    from midagma_amd.simulate import make_dataset
    from midagma_amd.solver import HipSolver
    X, _, _ = make_dataset(d, 2 * d, seed=args.seed)
    X = X - X.mean(0, keepdims=True)
    rng = np.random.default_rng(args.seed)
    iu = np.array(np.triu_indices(d, 1)).T
    pairs = iu[rng.uniform(size=len(iu)) < 0.3]
    s = HipSolver(d, "l2", "cov", device=device)
    s.set_cov(X.T @ X / X.shape[0])
    s.set_trek_tcc(pairs, mode="opt", weight=0.1)
    s.begin(np.zeros((d, d)), 1.0, 2 * K + warm + 1000, 1.0, 3e-4, tol=-1.0, lambda1=0.03)
    out = dict(d=d, unit="ms per Adam step", pairs=int(len(pairs)), weight=0.1)

    def run_to(target):  # slots in small batches until `target` Adam steps (a hand-back's re-run,
        for _ in range(100000):  # and the no-op rest of its batch, take slots of their own)
            if s.poll().iters >= target:
                return
            s.run_slots(8)
        raise RuntimeError("tcc leg: no progress")

    for key, pre in (("from_W0", 0), ("later", warm)):
        run_to(s.poll().iters + pre)
        s.sync()
        b0, i0, t0 = s.debug_handbacks(), s.poll().iters, time.perf_counter()
        run_to(i0 + K)
        s.sync()
        dt = time.perf_counter() - t0
        it = int(s.poll().iters - i0)
        out[key] = dict(ms_per_step=dt / max(it, 1) * 1e3, steps=it, handbacks=int(s.debug_handbacks() - b0),
                        after_steps=int(i0))
    r = s.poll()
    s.close()
    out["verified"] = bool(r.status == 0)
    return out


def bench_cov_large(args, device):
    """Config 3: d=5000, n=5e4, l2, cov mode on one GPU -- the inverse-dominated
    size.  X is generated on the GPU (csrc/sem.hip) and prepared as fit() prepares a device X
    (linear.py:411, 428): the product's fixed-order column sums and in-place centring
    (midagma_colsum_dev, midagma_center_dev), the Gram X^T X on the FP64 MFMA (midagma_gram)
    and cov = G / n on the device (midagma_set_cov_dev)."""
    import torch
    from midagma_amd.solver import HipSolver, center_dev, colsum_dev, gram
    d, n = args.large_d, args.large_n
    dev = torch.device("cuda", device)
    X, _, _ = make_shard(d, n, 1, 0, args.seed, dev)
    s = HipSolver(d, "l2", "cov", device=device)
    torch.cuda.synchronize(dev)
    t_prep = time.perf_counter()
    with torch.cuda.device(dev):
        center_dev(X, colsum_dev(X), float(n))
        G = gram(X, device)
    s.set_cov_gram(G, float(n))
    t_prep = time.perf_counter() - t_prep
    del X, G
    torch.cuda.empty_cache()
    cov = s.get_cov()
    K = args.large_steps
    s.begin(np.zeros((d, d)), 1.0, K + 1000, 1.0, 3e-4, tol=-1.0, lambda1=0.03)
    s.run_slots(3)
    s.sync()
    t0 = time.perf_counter()
    s.run_slots(K)
    s.sync()
    t1 = time.perf_counter()
    r = s.poll()
    prof = s.profile_parts(3)
    # value check: 8 Adam steps from W = 0 with checkpoints every 4 (pivoted and fast slots)
    Kc = 8
    Wc = np.zeros((d, d))
    rc = s.minimize(Wc, 1.0, Kc, 1.0, 3e-4, tol=-1.0, lambda1=0.03, checkpoint=4)
    s.close()
    F = 4.0 * d ** 3
    return dict(value=K / (t1 - t0), unit="steps/s", ms_per_step=(t1 - t0) / K * 1e3, steps=K,
                verified=(r.status == 0 and r.iters == K + 3),
                workload=f"config3: d={d}, n={n}, l2, cov mode (reference algorithm), 1 GPU",
                kernel_ms={k: round(v, 4) for k, v in prof.items()},
                slot_tflops=F / ((t1 - t0) / K) / 1e12, slot_frac_fp64_peak=F / ((t1 - t0) / K) / 1e12 / 78.6,
                prep={"seconds": t_prep, "what": "centring, Gram and cov on the device through the product "
                                                  "(midagma_colsum_dev, _center_dev, _gram, _set_cov_dev)"},
                cov=cov, W_check=Wc, check_steps=Kc, check_iters=int(rc.iters))


_CPU_CHILD = r"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
from threadpoolctl import threadpool_limits
from oracle.dagma_oracle import LinearOracle
mode, d, extra = sys.argv[2], int(sys.argv[3]), sys.argv[4]
threads = [int(t) for t in sys.argv[5].split(",")]
steps = int(sys.argv[6])
warm = sys.argv[7] == "1"


def gauss(n, d, seed):
    # N(0,1) n x d in parallel chunks (independent streams; numpy releases the GIL)
    from concurrent.futures import ThreadPoolExecutor
    X = np.empty((n, d))
    ch = max(1, -(-n // 32))
    def fill(k):
        np.random.default_rng([seed, k]).standard_normal(out=X[k * ch:(k + 1) * ch])
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(fill, range(-(-n // ch))))
    return X


if mode == "fit":                       # config 1: the whole default fit() (linear.py:335-462)
    from midagma_amd.simulate import make_dataset
    X, _, _ = make_dataset(d, int(extra), seed=0)
    out = {}
    for th in threads:
        with threadpool_limits(limits=th):
            o = LinearOracle("l2")
            t0 = time.perf_counter()
            o.fit(X.copy(), lambda1=0.03)
            out[th] = time.perf_counter() - t0
            out_it = sum(st[4].iters for st in o.stages)
        print(json.dumps({"partial": out}), flush=True)
    print(json.dumps({"t": out, "iters": out_it}), flush=True)
    sys.exit(0)
if mode == "cov":                       # the reference algorithm: cov precomputed once
    o = LinearOracle("l2")
    o.cov, o.X, o.n = np.load(extra), None, 10000
elif mode == "tcc":                     # the reference algorithm with the TCC trek regularizer ('opt')
    T = np.load(extra)
    o = LinearOracle("l2")
    o.cov, o.X, o.n = T["cov"], None, 10000
    o.trek = dict(kind="tcc", pairs=T["pairs"], mode="opt", weight=float(T["weight"]))
elif mode == "data":                    # the workload's math: -(mu/n) X^T (X (I - W)) per step
    n = int(extra)
    o = LinearOracle("l2", score_mode="data")
    o.X, o.n, o.cov = gauss(n, d, 0), n, None
else:                                   # logistic: (mu/n) X^T expit(X W) - mu cov per step
    n = int(extra)
    o = LinearOracle("logistic")
    X = (gauss(n, d, 1) > 0).astype(np.float64)
    o.X, o.n, o.cov = X, n, X.T @ X / float(n)
o.d, o.eye, o.lambda1, o.checkpoint, o.inc, o.exc = d, np.eye(d), 0.03, 10 ** 9, None, None
# the objective is evaluated once per `checkpoint` (1000) steps in a fit; the timed window is
# the Adam step itself, so the final-iteration objective is not evaluated here
o._objective = lambda W, mu, s: (0.0, 0.0, 0.0)
out = {}
for th in threads:
    with threadpool_limits(limits=th):
        if warm:
            o.minimize(np.zeros((d, d)), 1.0, 1, 1.0, 3e-4, tol=-1.0)   # warm: pools, pages
        t0 = time.perf_counter()
        W, tr = o.minimize(np.zeros((d, d)), 1.0, steps, 1.0, 3e-4, tol=-1.0)
        out[th] = (time.perf_counter() - t0) / steps
        assert tr.iters == steps
    print(json.dumps({"partial": out}), flush=True)
print(json.dumps({"t": out}), flush=True)
"""


# --------------------------------------------------------------------------- value checks
# Every leg's W (or parameters) after its steps is compared with the CPU oracle's run of the
# same steps from the same start (oracle/: the numpy/scipy restatement of linear.py:165-333,
# bit-exact to the reference at one BLAS thread; test infrastructure -- the checker, never the
# thing measured).  The oracle runs in a child process without the GPU, after the GPU legs.
_CHECK_CHILD = r"""
import json, sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
from threadpoolctl import threadpool_limits
kind, inp, outp, th = sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5])
P = dict(np.load(inp))
t0 = time.perf_counter()
out = {}
with threadpool_limits(limits=th):
    if kind in ("l2", "logistic", "logistic_blocked"):
        from oracle.dagma_oracle import LinearOracle

        class Blocked(LinearOracle):
            # X^T expit(X W) summed in 64-row blocks: a summation order as valid as OpenBLAS's,
            # the reference's own order sensitivity (tests/test_gpu_parity.py _BlockedOracle)
            def score_grad(self, W, mu):
                from scipy.special import expit
                S = expit(self.X @ W)
                Z = np.zeros((self.d, self.d))
                blk = 64 if self.n <= 65536 else 1024  # (64-row products would take minutes at n=1e6)
                for c in range(0, self.n, blk):
                    Z += self.X[c:c + blk].T @ S[c:c + blk]
                return (mu / self.n) * Z - mu * self.cov

        o = (Blocked if kind == "logistic_blocked" else LinearOracle)("l2" if kind == "l2" else "logistic")
        o.cov = P["cov"]
        if kind == "l2":
            o.X, o.n = None, 1
        else:
            o.X, o.n = P["X"], P["X"].shape[0]
        d = o.cov.shape[0]
        o.d, o.eye, o.lambda1, o.checkpoint, o.inc, o.exc = d, np.eye(d), float(P["lambda1"]), 10 ** 9, None, None
        o._objective = lambda W, mu, s: (0.0, 0.0, 0.0)   # tol=-1: the objective decides nothing
        W, tr = o.minimize(np.zeros((d, d)), 1.0, int(P["K"]), 1.0, 3e-4, tol=-1.0)
        out = dict(W=W, iters=tr.iters, halvings=tr.halvings)
    elif kind == "tcc":
        from oracle.dagma_oracle import LinearOracle
        o = LinearOracle("l2")
        o.cov = P["cov"]
        o.X, o.n = None, 1
        d = o.cov.shape[0]
        o.d, o.eye, o.lambda1, o.checkpoint, o.inc, o.exc = d, np.eye(d), float(P["lambda1"]), 10 ** 9, None, None
        o.trek = dict(kind="tcc", pairs=P["pairs"], mode="opt", weight=float(P["weight"]))
        o._objective = lambda W, mu, s: (0.0, 0.0, 0.0)   # tol=-1: the objective decides nothing
        W, tr = o.minimize(np.zeros((d, d)), 1.0, int(P["K"]), 1.0, 3e-4, tol=-1.0)
        out = dict(W=W, iters=tr.iters)
    elif kind == "fit":
        from oracle.dagma_oracle import LinearOracle
        o = LinearOracle("l2")
        W = o.fit(P["X"].copy(), lambda1=float(P["lambda1"]))
        out = dict(W=W, stage_iters=np.array([st[4].iters for st in o.stages]))
    elif kind == "mlp":
        import torch
        torch.set_num_threads(th)
        from oracle.mlp_oracle import OracleMLP, load_params, nonlinear_minimize
        d = int(P["d"])
        m = OracleMLP([d, 10, 1])
        keys = [k for k in P if k not in ("X", "d", "calls")]
        load_params(m, {k: P[k] for k in keys})
        X = torch.from_numpy(P["X"])
        for K in P["calls"].tolist():
            ok, it = nonlinear_minimize(m, X, int(K), 2e-4, 0.02, 0.005, 0.1, 1.0, tol=-1, checkpoint=10 ** 9)
            assert ok and it == K, (ok, it, K)
        out = {k: v.detach().numpy().copy() for k, v in m.state_dict().items() if k in keys}
np.savez(outp, **out)
print(json.dumps({"t": time.perf_counter() - t0}), flush=True)
"""


def oracle_run(kind, inputs, threads=8, timeout=900):
    """The CPU oracle on `inputs` in a child process (no GPU, `threads` BLAS threads); its output
    arrays, or None (logged) when it failed or timed out."""
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        ip, op = os.path.join(td, "in.npz"), os.path.join(td, "out.npz")
        np.savez(ip, **inputs)
        env = dict(os.environ, HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS=str(threads),
                   OPENBLAS_NUM_THREADS=str(threads))
        t0 = time.perf_counter()
        try:
            r = subprocess.run([sys.executable, "-c", _CHECK_CHILD, REPO, kind, ip, op, str(threads)],
                               capture_output=True, text=True, timeout=timeout, env=env)
        except subprocess.TimeoutExpired:
            log(f"oracle check ({kind}) timed out after {timeout}s")
            return None
        if r.returncode != 0 or not os.path.exists(op):
            log(f"oracle check ({kind}) exited {r.returncode}: {r.stderr[-800:]}")
            return None
        out = dict(np.load(op))
    log(f"oracle check ({kind}): {time.perf_counter() - t0:.1f} s")
    return out


def w_check(W, ref, tol, K, what):
    """The value check one leg reports: max|W_gpu - W_oracle| after the same K steps."""
    if ref is None:
        return {"ok": False, "max_dW": None, "tol": tol, "steps": K, "oracle": what, "error": "oracle run failed"}
    dW = float(np.abs(np.asarray(W) - ref).max())
    return {"ok": bool(dW <= tol), "max_dW": dW, "tol": tol, "steps": K, "oracle": what}


def check_l2(W, cov, K, what, threads=8, timeout=900):
    """W after K l2 Adam steps (mu=1, s=1, lr=3e-4, lambda1=0.03, from W=0) against the
    oracle's reference-algorithm run (cov precomputed, linear.py:244) of the same K steps."""
    out = oracle_run("l2", {"cov": np.ascontiguousarray(cov), "K": K, "lambda1": 0.03}, threads, timeout)
    c = w_check(W, None if out is None else out["W"], 1e-9, K, what)
    if out is not None and int(out["iters"]) != K:
        c.update(ok=False, error=f"oracle ran {int(out['iters'])} steps")
    return c


def logistic_check(c, threads=8):
    """Logistic leg (linear.py:246): W after K steps against the oracle.  With binary X the
    entries on the L1 kink chatter with amplitude ~lr and their sign follows the last rounding
    bit of X^T expit(XW), in the reference as much as here, so the bar is
    the reference's own summation-order envelope -- the oracle with 64-row blocked sums -- as in
    tests/test_gpu_parity.py::test_logistic_data_mode_d100: no entry further than
    max(1e-5, 2x the envelope), no more entries beyond 1e-9 than the envelope moves (+50%)."""
    inp = {"X": c["X"], "cov": c["cov"], "K": c["K"], "lambda1": 0.03}
    threads = c.get("threads", threads)
    floor = c.get("floor", 1e-5)
    a = oracle_run("logistic", inp, threads)
    b = oracle_run("logistic_blocked", inp, threads)
    if a is None or b is None:
        return {"ok": False, "max_dW": None, "steps": c["K"], "error": "oracle run failed"}
    diff, env = np.abs(c["W"] - a["W"]), np.abs(b["W"] - a["W"])
    n_diff, n_env = int((diff > 1e-9).sum()), int((env > 1e-9).sum())
    ok = bool(diff.max() <= max(floor, 2 * env.max()) and n_diff <= 1.5 * n_env + 10)
    return {"ok": ok, "max_dW": float(diff.max()), "envelope_max": float(env.max()), "entries_beyond_1e-9": n_diff,
            "envelope_entries_beyond_1e-9": n_env, "steps": c["K"], "tol": f"max({floor:g}, 2 x envelope)",
            "oracle": "LinearOracle('logistic') and its row-blocked-sum variant (the reference's order envelope)"}


def value_checks(res, cov_res, large_res, small_res, mlp_res, logi, rank, world, fit4=None, tcc_res=None):
    """Every leg's value check (attached as `value_check`; `verified` requires it)."""
    if tcc_res is not None and "_check" in tcc_res:
        c = tcc_res.pop("_check")
        out = oracle_run("tcc", {"cov": c["cov"], "pairs": c["pairs"], "K": c["K"], "weight": c["weight"],
                                 "lambda1": 0.03}, threads=1)
        tcc_res["value_check"] = w_check(c["W"], None if out is None else out["W"], 1e-9, c["K"],
                                         "oracle minimize with the TCC regularizer (numpy eig Perron pairs, "
                                         "oracle/trek_oracle.py), same steps from W = 0")

    if fit4 is not None and "_check" in fit4:
        c = fit4.pop("_check")
        vc = check_l2(c["W"], c["cov"], c["K"], "oracle reference algorithm on the fit's device-Gram cov, "
                      "the fit's first 1000 stage-1 Adam steps from W = 0", threads=16)
        if c["iters"] != c["K"]:
            vc["ok"] = False
        fit4["value_check"] = vc
    if res is not None and rank == 0:
        res["value_check"] = check_l2(res["W"], res["cov"], res["steps_total"],
                                      "oracle reference algorithm (cov = X^T X / n of the same X from the device "
                                      "Gram, linear.py:244), same steps from W = 0")
        res["verified"] = bool(res["verified"] and res["value_check"]["ok"])
    if cov_res is not None:
        cov_res["value_check"] = check_l2(cov_res["W"], cov_res["cov"], cov_res["steps_total"],
                                          "oracle reference algorithm, same cov, same steps from W = 0 (the timed run)")
    if large_res is not None:
        c = check_l2(large_res["W_check"], large_res["cov"], large_res["check_steps"],
                     "oracle reference algorithm, same cov: a separate 8-step run from W = 0 with checkpoints "
                     "every 4 (pivoted and fast slots)", threads=16)
        if large_res["check_iters"] != large_res["check_steps"]:
            c["ok"] = False
        large_res["value_check"] = c
    if small_res is not None and "_check" in small_res:
        c = small_res.pop("_check")
        small_res["value_check"] = check_l2(c["W"], c["cov"], c["K"], "oracle reference algorithm, same cov, "
                                            "same steps from W = 0 (the timed window and its warm-up)", threads=1)
        f = oracle_run("fit", {"X": c["X"], "lambda1": 0.03}, threads=1)
        if f is not None:
            ref_it = [int(x) for x in f["stage_iters"]]
            sup = bool(np.array_equal(c["W_fit"] != 0, f["W"] != 0))
            # the last stage (mu=1e-4, s=0.6) is chaotic in the reference itself: one checkpoint of slack
            same = (len(ref_it) == len(c["stage_iters"]) and ref_it[:-1] == c["stage_iters"][:-1]
                    and abs(ref_it[-1] - c["stage_iters"][-1]) <= 1000)
            small_res["fit"]["value_check"] = {
                "ok": bool(sup and same), "support_identical": sup, "stage_iters_oracle": ref_it,
                "max_dW": float(np.abs(c["W_fit"] - f["W"]).max()),
                "oracle": "oracle DagmaLinear fit() defaults on the same X (linear.py:335-462)"}
    if mlp_res is not None and "_check" in mlp_res:
        c = mlp_res.pop("_check")
        inp = dict(c["params"], X=c["X"], d=c["X"].shape[1], calls=np.array(c["calls"]))
        out = oracle_run("mlp", inp, threads=16)

        def pdev(fin, ref):
            return {k: float(np.abs(fin[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max())) for k in fin}
        if out is None:
            mlp_res["value_check"] = {"ok": False, "error": "oracle run failed"}
        else:
            dev = pdev(c["final"], out)
            worst = max(dev.values())
            mlp_res["value_check"] = {
                "ok": bool(worst <= 1e-9), "max_dparam_rel": worst, "tol": 1e-9, "per_param": dev,
                "steps": int(sum(c["calls"])), "calls": c["calls"],
                "oracle": "oracle DagmaNonlinear.minimize (torch CPU, slogdet h_func), the same calls from the "
                          "same parameters, replayed on the GPU after the timed run through the same path; "
                          "|dp| / max(1, max|p|)"}
            inp_t = dict(inp, calls=np.array(c["timed_calls"]))
            out_t = oracle_run("mlp", inp_t, threads=16)
            if out_t is not None:
                dt_ = pdev(c["timed_final"], out_t)
                mlp_res["value_check"]["timed_window"] = {
                    "calls": c["timed_calls"], "max_dparam_rel": max(dt_.values()),
                    "note": "not held to 1e-9: the reference's trajectory is chaotic here (a 1e-15 relative "
                            "change of the start moves the oracle's parameters by 6e-3 at step 2020, "
                            "profiles/r03_mlp_chaos.log)"}
    for lg in logi or []:
        c = lg.pop("_check", None)
        if c is None:
            lg["value_check"] = {"ok": None, "note": "skipped (--no-check)"}
        else:
            lg["value_check"] = logistic_check(c)
    for leg in (cov_res, large_res, small_res, mlp_res, tcc_res):
        if leg is not None and "value_check" in leg:
            leg["verified"] = bool(leg["verified"] and leg["value_check"]["ok"])
    if small_res is not None and "value_check" in small_res.get("fit", {}):
        small_res["verified"] = bool(small_res["verified"] and small_res["fit"]["value_check"]["ok"])
    for lg in logi or []:
        if lg["value_check"].get("ok") is False:
            lg["verified"] = False


def host_cpus():
    """Host CPU facts for the baseline's `cores` statement: logical CPUs, physical cores
    (unique (package, core) pairs from sysfs), this process's affinity and cgroup quota."""
    import glob
    logical = os.cpu_count() or 1
    pairs = set()
    for c in glob.glob("/sys/devices/system/cpu/cpu[0-9]*/topology"):
        try:
            pairs.add((open(c + "/physical_package_id").read().strip(), open(c + "/core_id").read().strip()))
        except OSError:
            pass
    physical = len(pairs) or logical
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        quota = None if q == "max" else float(q) / float(per)
    except (OSError, ValueError):
        pass
    aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else logical
    return {"logical_cpus": logical, "physical_cores": physical, "affinity_cpus": aff, "cgroup_cpu_quota": quota}


def thread_sweep(phys, base=(1, 4, 8, 16)):
    """BASELINE.md's plan: threads in {1, 4, 8, 16, physical/2, physical}."""
    return sorted({t for t in base} | {max(1, phys // 2), phys})


def _cpu_runs(mode, d, extra, threads, steps, timeout=900, warm=True):
    """One child process (no GPU) times `steps` oracle Adam steps per thread count; all three
    BLAS/OpenMP pools pinned by threadpoolctl.  Returns {threads: seconds per step}."""
    import subprocess
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS=str(max(threads)),
               OPENBLAS_NUM_THREADS=str(max(threads)))
    try:
        r = subprocess.run([sys.executable, "-c", _CPU_CHILD, REPO, mode, str(d), str(extra),
                            ",".join(str(t) for t in threads), str(steps), "1" if warm else "0"],
                           capture_output=True, text=True, timeout=timeout, env=env)
        lines = [json.loads(x) for x in r.stdout.strip().splitlines() if x.startswith("{")]
        if r.returncode != 0:
            log(f"cpu oracle ({mode}) exited {r.returncode}: {r.stderr[-400:]}")
        got = lines[-1].get("t") or lines[-1].get("partial") if lines else {}
        return {int(k): float(v) for k, v in (got or {}).items()}
    except subprocess.TimeoutExpired as e:
        lines = [json.loads(x) for x in (e.stdout or b"").decode(errors="ignore").splitlines() if x.startswith("{")]
        log(f"cpu oracle ({mode}) timed out after {timeout}s")
        return {int(k): float(v) for k, v in (lines[-1].get("partial", {}) if lines else {}).items()}


def _best(runs, unit_per_step=1.0):
    th = min(runs, key=runs.get)
    return th, unit_per_step / runs[th]


def bench_fit(args, device):
    """Full-fit wall-clock (BASELINE metric, second half): DagmaLinear.fit with the reference's
    defaults (T=5, warm 3e4, max 6e4, s=[1,.9,.8,.7,.6], lr 3e-4, lambda1 0.03) at config 2."""
    from midagma_amd import DagmaLinear
    from midagma_amd.simulate import count_accuracy, make_dataset
    X, W_true, B_true = make_dataset(args.d, args.cov_n, seed=args.seed)
    m = DagmaLinear("l2", device=device)
    t0 = time.perf_counter()
    W = m.fit(X.copy(), lambda1=0.03)
    wall = time.perf_counter() - t0
    iters = [e["iters"] for e in m.minimize_log]
    acc = count_accuracy(B_true, W != 0)
    return dict(wall_s=wall, total_iters=int(sum(iters)), stage_iters=iters,
                calls=[{k: e[k] for k in ("mu", "s", "lr", "iters", "success", "early_stop")} for e in m.minimize_log],
                accuracy=acc, h_final=float(m.h_final), score_final=float(m.score_final))


def bench_fit_config4(args, world, rank, local, data_ms_per_step=None):
    """Full-fit wall-clock at the headline configuration (BASELINE metric, second half; VERDICT r03
    item 1): X (d=1000, n=1e6) generated on the GPU(s) -- each rank only its rows --, then
    DagmaLinear('l2').fit with the reference's defaults in cov mode: the centring and cov's Gram on
    the device (one all-reduce of the column sums and one of the d x d Gram across ranks), then the
    n-independent loop (linear.py:428, 441-453), replicated with no per-step communication.
    The wall clock is split into generation, data preparation and the loop."""
    import torch
    import torch.distributed as dist
    from midagma_amd import DagmaLinear
    from midagma_amd.simulate import count_accuracy, simulate_er_dag, simulate_weights
    from midagma_amd.solver import HipSolver
    dev = torch.device("cuda", local)
    d, n = args.d, args.n
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    X, n_k, t_gen = make_shard(d, n, world, rank, args.seed, dev)
    m = DagmaLinear("l2", device=local)
    t1 = time.perf_counter()
    W = m.fit(X, lambda1=0.03, n_global=n if world > 1 else None)
    torch.cuda.synchronize(dev)
    wall = time.perf_counter() - t0
    fit_wall = time.perf_counter() - t1
    del X
    torch.cuda.empty_cache()
    ft = dict(m.fit_timing)
    t = torch.tensor([wall, fit_wall, ft["prep_s"], ft["loop_s"]], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    wall, fit_wall, prep_s, loop_s = (float(x) for x in t.cpu())
    iters = [e["iters"] for e in m.minimize_log]
    rng = np.random.default_rng(args.seed)          # make_shard's graph, drawn again
    B_true = simulate_weights(simulate_er_dag(d, d, rng), rng) != 0
    out = dict(wall_s=wall, fit_s=fit_wall, sem_gen_s=t_gen, prep_s=prep_s, loop_s=loop_s, final_s=ft["final_s"],
               cov_on=ft["cov_on"], total_iters=int(sum(iters)), stage_iters=iters,
               calls=[{k: e[k] for k in ("mu", "s", "lr", "iters", "success", "early_stop")} for e in m.minimize_log],
               accuracy=count_accuracy(B_true, W != 0), h_final=float(m.h_final), score_final=float(m.score_final),
               loop_steps_per_s=sum(iters) / loop_s if loop_s > 0 else None, n_per_gpu=n_k,
               timing="wall_s = GPU SEM generation + fit(); prep_s = centring + Gram + all-reduces + set_cov; "
                      "loop_s = the path-following loop; max over ranks")
    if data_ms_per_step:
        out["data_mode_projected_wall_s"] = out["total_iters"] * data_ms_per_step * 1e-3
        out["data_mode_projection"] = ("projected, not run: the same total Adam steps at this run's data-mode "
                                       "ms_per_step (two n x d x d GEMMs per step), i.e. what fit(score_mode='data') "
                                       "would take")
    if rank == 0 and not args.no_check:
        # the fit's cov, 1000 Adam steps of stage 1 (mu=1, s=1, lr=3e-4) on the GPU, for the oracle
        s = HipSolver(d, "l2", "cov", device=local)
        s.set_cov(m.cov)
        Wc = np.zeros((d, d))
        r = s.minimize(Wc, 1.0, 1000, 1.0, 3e-4, tol=-1.0, lambda1=0.03, checkpoint=1000)
        s.close()
        out["_check"] = dict(W=Wc, cov=m.cov, K=1000, iters=r.iters)
    m._solver.close()
    return out


# every cpu_baseline object says how the port differs from the reference it restates
PORT_NOTE = ("conservative: the port computes the six gradient-norm diagnostics (linear.py:262-273) on "
             "checkpoint steps only, the reference on every step, so the port runs faster than the "
             "reference itself and GPU/CPU ratios are understated")


def cpu_baseline(args, cov):
    """CPU oracle (numpy/scipy restatement of the reference, bit-identical at 1 thread) on the
    host cores, in child processes with no GPU:
      * 'port' of THIS workload (data mode, n = args.n rows, measured at that n);
      * the reference algorithm (cov precomputed, O(d^3) per step, n-independent).
    Threads swept over {1, 4, 8, 16, physical/2, physical}; the n=1e6 data-mode
    step (two 2-TFLOP host GEMMs) is timed at the counts that can win, {8, 16, physical/2,
    physical}: 1 and 4 threads would take minutes per step."""
    import tempfile
    d = cov.shape[0]
    hc = host_cpus()
    phys = hc["physical_cores"]
    res = {"host": hc}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "cov.npy")
        np.save(path, cov)
        sweep = thread_sweep(phys)
        ref = _cpu_runs("cov", d, path, sweep, steps=20)
    for th, t in sorted(ref.items()):
        log(f"cpu reference algorithm d={d}: {1 / t:.2f} steps/s at {th} threads")
    if ref:
        th, v = _best(ref)
        res["reference_algorithm"] = dict(
            value=v, unit="steps/s", cores=th, kind="port", note=PORT_NOTE, physical_cores=phys,
            sweep={str(k): 1.0 / t for k, t in sorted(ref.items())},
            sample=f"oracle cov-mode Adam steps at d={d} (linear.py:244 with cov precomputed once, as fit() "
                   f"does), 20 steps per thread count, threads {sorted(ref)} (host: {phys} physical cores, "
                   f"{hc['logical_cpus']} logical, cgroup quota {hc['cgroup_cpu_quota']}), best shown")
    if args.workload == "data":
        cands = sorted({8, 16, max(1, phys // 2), phys})
        dat = _cpu_runs("data", d, args.n, cands, steps=2, timeout=1200, warm=False)
        for th, t in sorted(dat.items()):
            log(f"cpu data-mode port d={d} n={args.n}: {t:.2f} s/step at {th} threads")
        if dat:
            th, v = _best(dat)
            res["workload"] = dict(
                value=v, unit="steps/s", cores=th, kind="port", note=PORT_NOTE, physical_cores=phys,
                sweep={str(k): 1.0 / t for k, t in sorted(dat.items())},
                sample=f"oracle data-mode Adam step (G = -(mu/n) X^T (X (I-W)), the workload's math) measured "
                       f"at n={args.n}, d={d}: 2 steps per thread count, threads "
                       f"{sorted(dat)} (1 and 4 not run: minutes per step); host {phys} physical cores, "
                       f"{hc['logical_cpus']} logical, cgroup quota {hc['cgroup_cpu_quota']}; best shown")
    return res


def attach_cpu(line, cpu, value):
    """The CPU baselines on the line: `cpu_baseline` is the port of the workload's own math at the
    same n (`vs_cpu`); `cpu_reference_algorithm` is the reference's own algorithm (cov formed once,
    O(d^3) per step: what the reference's fit() runs at d=1000), and `vs_cpu_reference_algorithm`
    compares the headline with it -- the like-for-like comparison with the reference's CPU path."""
    if "workload" in cpu:
        line["cpu_baseline"] = cpu["workload"]
        line["vs_cpu"] = value / cpu["workload"]["value"]
    elif "reference_algorithm" in cpu:
        line["cpu_baseline"] = cpu["reference_algorithm"]
    if "reference_algorithm" in cpu:
        line["cpu_reference_algorithm"] = cpu["reference_algorithm"]
        line["vs_cpu_reference_algorithm"] = value / cpu["reference_algorithm"]["value"]


def _pmc_kernel(kernel, d, n_k):
    """Name under which tools/pmc_summary.py files the data-mode GEMM: both GEMMs are
    gemm_pipe_kernel<1, 0, 0> (A from X^T / X, plain B), told apart by their grids."""
    D = -(-d // 128) * 128
    if kernel == "gemm_xw":
        grid = (-(-n_k // 128)) * (D // 128)
    else:
        split = max(1, min(-(-n_k // 128) * 128 // 64 // 8, -(-1024 // (D // 128) ** 2), 32))
        grid = (D // 128) ** 2 * split
    return f"midagma::gemm_pipe_kernel<1, 0, 0> grid={grid}"


def _pmc_traffic(kernel, d, n, world, n_k):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC summary of this exact
    workload (profiles/*_pmc_bench_data_*.json; FETCH_SIZE x2 + WRITE_SIZE), else None."""
    import glob
    for f in sorted(glob.glob(os.path.join(REPO, "profiles", "*_pmc_bench_data_*.json")), reverse=True):
        try:
            j = json.load(open(f))
            w = j.get("workload", {})
            if (w.get("d"), w.get("n"), w.get("world")) != (d, n, world):
                continue
            k = j["kernels"].get(_pmc_kernel(kernel, d, n_k))
            if k:
                return k["hbm_bytes_corrected"], os.path.relpath(f, REPO)
        except Exception:  # noqa: BLE001
            continue
    return None, None


def _profile_roofline(d, n, world, n_k):
    """The dominant GEMM's roofline from the newest committed rocprofv3 summary of this exact data
    leg (profiles/*_rocprof_data*_kernel_stats.csv with its sibling *_bench_line.json, the JSON line
    the profiled run printed): both data-mode GEMMs are gemm_pipe_kernel<1, 0, 0>, so the summary's
    average is over both, and it is set beside the live mean of the two.  None when absent."""
    import csv
    import glob
    for f in sorted(glob.glob(os.path.join(REPO, "profiles", "*_rocprof_data*_kernel_stats.csv")), reverse=True):
        lf = f.replace("_kernel_stats.csv", "_bench_line.json")
        if not os.path.exists(lf):
            continue
        try:
            ln = json.load(open(lf))
            c = ln.get("config", {})
            if (c.get("d"), c.get("n"), ln.get("n_gpus")) != (d, n, world):
                continue
            for r in csv.DictReader(open(f)):
                if "gemm_pipe_kernel<1, 0, 0>" in r["Name"]:
                    avg_ms = float(r["AverageNs"]) * 1e-6
                    ach = 2.0 * n_k * d * d / (avg_ms * 1e-3) / 1e12
                    return {"source": os.path.relpath(f, REPO), "line": os.path.relpath(lf, REPO),
                            "kernel": "gemm_pipe_kernel<1, 0, 0> (X(I-W) and X^T Y launches together)",
                            "calls": int(r["Calls"]), "avg_ms": avg_ms, "achieved": ach,
                            "frac": ach / FP64_MFMA_PEAK_TF, "profiled_ms_per_step": ln.get("ms_per_step")}
        except Exception:  # noqa: BLE001
            continue
    return None


def dump_outputs(path, arrays):
    """--dump-outputs: what a caller of the timed path receives after its last timed step, one
    float64 .npy per name (W: d x d, 8 MB at d=1000; loop_state: iterations, status, halvings and
    the final learning rate)."""
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        relaunch_ranks(args)
    if (int(os.environ.get("WORLD_SIZE", "1")) > 1 and os.environ.get("MIDAGMA_BENCH_WORKER") != "1"
            and os.environ.get("MIDAGMA_BENCH_SUPERVISE", "1") == "1"):
        sys.exit(supervise_ranks(args))
    if args.group_leg:  # run_group_leg's child: one process, every GPU
        import torch  # noqa: F401
        print(json.dumps(bench_group(args, args.gpus)), flush=True)
        return
    import torch
    world, rank, local = setup_dist(args)
    beat("process group up")
    res = bench_data(args, world, rank, local) if args.workload == "data" and not args.no_data else None
    cov_res = None
    if rank == 0 and (args.workload == "cov" or (world == 1 and not args.no_cov)):
        cov_res = bench_cov(args, local)
    if args.dump_outputs and rank == 0:
        timed = res if args.workload == "data" else cov_res
        if timed is not None:
            dump_outputs(args.dump_outputs, {"W": timed["W"], "loop_state": timed["loop_state"]})
    fit_res = None
    if rank == 0 and world == 1 and not args.no_fit:
        fit_res = bench_fit(args, local)
    large_res = None
    if rank == 0 and world == 1 and not args.no_large and args.workload == "data":
        large_res = bench_cov_large(args, local)
    mlp_res = None
    if rank == 0 and world == 1 and not args.no_mlp and args.workload == "data":
        mlp_res = bench_mlp(args, local, with_cpu=not args.no_cpu)
    small_res = None
    if rank == 0 and world == 1 and not args.no_small and args.workload == "data":
        small_res = bench_small(args, local, with_cpu=not args.no_cpu)
    tcc_res = None
    if rank == 0 and world == 1 and not args.no_tcc and args.workload == "data":
        try:  # a failure of this leg is reported in it, not taken out on the rest of the line
            tcc_res = bench_tcc(args, local, with_cpu=not args.no_cpu)
        except Exception as e:  # noqa: BLE001
            log(f"tcc leg failed: {e!r}")
            tcc_res = {"verified": False, "error": repr(e)[:400]}
    logi = None
    if rank == 0 and world == 1 and not args.no_logistic and args.workload == "data":
        logi = [bench_logistic(args, local, nn, args.logistic_steps if nn > 100_000 else 200)
                for nn in (10_000, args.n)]
    fit4 = None
    if args.workload == "data" and not args.no_fit4:
        fit4 = bench_fit_config4(args, world, rank, local, res["ms_per_step"] if res else None)
        beat("full fit (config 4) done")
    if not args.no_check:
        value_checks(res, cov_res, large_res, small_res, mlp_res, logi, rank, world, fit4, tcc_res)
        beat("value checks done")
    if rank == 0 and res is not None and res["cov"] is not None and os.environ.get("MIDAGMA_BENCH_COV_OUT"):
        np.save(os.environ["MIDAGMA_BENCH_COV_OUT"], res["cov"])  # the supervisor's CPU baseline
    for leg in (small_res, mlp_res, tcc_res, *(logi or [])):
        if leg is not None:
            leg.pop("_check", None)
    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu and cov_res is not None:
        cpu = cpu_baseline(args, cov_res["cov"])
        if logi:
            hc = cpu["host"]
            t = _cpu_runs("logistic", args.d, 10_000, thread_sweep(hc["physical_cores"]), steps=2)
            if t:
                th, v = _best(t)
                logi[0]["cpu_baseline"] = dict(
                    value=v, unit="steps/s", cores=th, kind="port", note=PORT_NOTE, physical_cores=hc["physical_cores"],
                    sweep={str(k): 1.0 / x for k, x in sorted(t.items())},
                    sample=f"oracle logistic Adam step (linear.py:246) at d={args.d}, n=10000 binary X: 2 steps "
                           f"per thread count after a warm step, threads {sorted(t)}, best shown")
                logi[0]["vs_cpu"] = logi[0]["value"] / v
    if rank == 0 and res is None and args.workload == "data":   # --no-data: a profiling run of the other legs
        out = {k: v for k, v in (large_res or {}).items() if k not in ("cov", "W_check")}
        cov_out = None if cov_res is None else {k: v for k, v in cov_res.items()
                                                if not isinstance(v, np.ndarray) and k not in ("cov", "_check")}
        print(json.dumps({"cov_mode": cov_out, "config3": out, "full_fit": fit_res, "config5": mlp_res,
                          "config1": small_res, "logistic": logi, "full_fit_config4": fit4,
                          "tcc": tcc_res}), flush=True)
        return
    if rank == 0:
        d = args.d
        sem_gen = None
        if args.workload == "data":
            prof = res["prof"] or {}                # (None: a plain run profiles no kernels, no roofline)
            n_k = res["n_local"]
            gemm_flops = 2.0 * n_k * d * d          # each of X(I-W) and X^T Y
            t_xty, t_xw = prof.get("gemm_xty", 0) * 1e-3, prof.get("gemm_xw", 0) * 1e-3
            dom, t_dom = ("gemm_xty", t_xty) if t_xty >= t_xw else ("gemm_xw", t_xw)
            ach = gemm_flops / t_dom / 1e12 if t_dom > 0 else None
            value, ms = res["value"], res["ms_per_step"]
            metric = ("Adam steps/s, d=1000 linear DAGMA (l2, data mode, X row-sharded over the GPUs, RCCL "
                      "all-reduce of the score gradient per step)" if world > 1 else
                      "Adam steps/s, d=1000 linear DAGMA (l2, data mode, X resident on 1 GPU)")
            cfg = {"workload": f"config4: d={d}, n={args.n} linear-Gaussian SEM, l2, data mode, rows sharded over "
                               f"{world} GPU(s)", "d": d, "n": args.n, "n_per_gpu": n_k,
                   "parallelism": f"dp{world} (row shards, W replicated)"}
            traffic, traffic_src = _pmc_traffic(dom, d, args.n, world, n_k)
            t_mean = 0.5 * (t_xty + t_xw)
            ach_mean = gemm_flops / t_mean / 1e12 if t_mean > 0 else None
            roof = {"bound": "mfma", "kernel": dom, "achieved": ach, "peak": FP64_MFMA_PEAK_TF, "unit": "TFLOP/s",
                    "frac": (ach / FP64_MFMA_PEAK_TF) if ach else None,
                    # the two GEMMs' mean launch (what a rocprofv3 summary of the shared template averages)
                    "achieved_mean_both": ach_mean,
                    "frac_mean_both": (ach_mean / FP64_MFMA_PEAK_TF) if ach_mean else None,
                    "profile": _profile_roofline(d, args.n, world, n_k),
                    "traffic": traffic,
                    "traffic_source": traffic_src,
                    "algorithmic_bytes_per_launch": 8.0 * 2 * n_k * d + 8.0 * d * d,
                    "algorithmic_per_launch": f"2*n_k*d^2 = {gemm_flops:.3e} flop",
                    "kernel_ms": {k: round(v, 4) for k, v in prof.items()}}
            if res["prof"] is None:
                roof = None
            verified = res["verified"]
            t_gen = res["sem_gen_s"]
            sem_gen = {"what": "X shard generation on the GPU (csrc/sem.hip: Philox noise, structural equations "
                               "level by level, slab transpose), one call (after a 256-row call that loads the code object)", "rows": n_k, "d": d,
                       "seconds": t_gen, "output_GB_per_s": 8.0 * n_k * d / t_gen / 1e9,
                       "frac_hbm_peak_output_bytes": 8.0 * n_k * d / t_gen / 8.0e12}
        else:
            value, ms = cov_res["value"], cov_res["ms_per_step"]
            metric = "Adam steps/s, d=1000 linear DAGMA (l2, cov mode)"
            cfg = {"workload": f"config2: d={d}, n={args.cov_n}, l2, cov mode, 1 GPU", "d": d, "n": args.cov_n,
                   "parallelism": "single GPU"}
            roof = None
            verified = cov_res["verified"]
        line = {"metric": metric, "value": value, "unit": "steps/s", "n_gpus": world,
                "steps": args.steps if args.workload == "data" else args.cov_steps,
                "warmup": args.warmup, "ms_per_step": ms, "higher_is_better": True,
                "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic", "config": cfg,
                "verified": verified, "full": bool(args.full)}
        if args.workload == "data" and res.get("value_check") is not None:
            line["value_check"] = res["value_check"]
        elif args.workload == "cov" and cov_res.get("value_check") is not None:
            line["value_check"] = cov_res["value_check"]
        if args.workload == "data" and world > 1:
            line["replicas_identical"] = res.get("replicas_identical")
            line["comm"] = res.get("comm")
        if roof is not None:
            line["roofline"] = roof
        if sem_gen is not None:
            line["sem_generator"] = sem_gen
        if cov_res is not None:
            p = cov_res["prof"]
            F = 4.0 * d ** 3
            cr = {"value": cov_res["value"], "unit": "steps/s", "ms_per_step": cov_res["ms_per_step"],
                  "workload": f"config2: d={d}, n={args.cov_n}, cov mode (reference algorithm), 1 GPU",
                  "verified": cov_res["verified"], "kernel_ms": {k: round(v, 4) for k, v in p.items()},
                  # per Adam step of the timed run (fast slots with their GJ slots), not the
                  # profile's one-slot figures (kernel_ms "slot" is the pivoted GJ slot)
                  "slot_tflops": F / (cov_res["ms_per_step"] * 1e-3) / 1e12,
                  "slot_frac_fp64_peak": F / (cov_res["ms_per_step"] * 1e-3) / 1e12 / FP64_MFMA_PEAK_TF,
                  "value_check": cov_res.get("value_check")}
            if args.workload == "cov":
                line["roofline"] = {"bound": "mfma", "kernel": "slot", "achieved": cr["slot_tflops"],
                                    "peak": FP64_MFMA_PEAK_TF, "unit": "TFLOP/s", "frac": cr["slot_frac_fp64_peak"],
                                    "traffic": None}
            else:
                line["cov_mode"] = cr
        if cpu:
            attach_cpu(line, cpu, value)
            if "reference_algorithm" in cpu and cov_res is not None:
                line["cov_mode_vs_cpu_reference_algorithm"] = cov_res["value"] / cpu["reference_algorithm"]["value"]
        if large_res is not None:
            lr_ = {k: v for k, v in large_res.items() if k not in ("cov", "W_check", "check_steps", "check_iters")}
            if cpu is not None and not args.no_cpu:
                import tempfile
                phys = cpu["host"]["physical_cores"]
                cands = sorted({16, max(1, phys // 2), phys})
                with tempfile.TemporaryDirectory() as td:
                    path = os.path.join(td, "cov.npy")
                    np.save(path, large_res["cov"])
                    t = _cpu_runs("cov", args.large_d, path, cands, steps=2, timeout=900)
                if t:
                    th, v = _best(t)
                    lr_["cpu_reference_algorithm"] = dict(
                        value=v, unit="steps/s", cores=th, kind="port", note=PORT_NOTE, physical_cores=phys,
                        sweep={str(k): 1.0 / x for k, x in sorted(t.items())},
                        sample=f"oracle cov-mode Adam steps at d={args.large_d}: 2 steps per thread count after a "
                               f"warm step, threads {sorted(t)} (1-8 not run: tens of seconds per step), best shown")
                    lr_["vs_cpu"] = lr_["value"] / v
            line["config3"] = lr_
        if mlp_res is not None:
            line["config5"] = mlp_res
        if logi:
            line["logistic"] = logi
        if small_res is not None:
            line["config1"] = small_res
        if tcc_res is not None:
            line["tcc"] = tcc_res
        if fit4 is not None:
            f4 = dict(fit4)
            f4.pop("_check", None)
            f4["workload"] = (f"config4: DagmaLinear('l2').fit(X) defaults, d={d}, n={args.n}, X generated on the "
                              f"GPU{'s' if world > 1 else ''} and {'row-sharded over ' + str(world) + ' ranks' if world > 1 else 'device-resident'}"
                              f", cov mode (device centring + Gram, then the n-independent loop)")
            f4["verified"] = bool(f4.get("value_check", {}).get("ok", True))
            if cpu and "reference_algorithm" in cpu:
                ref_v = cpu["reference_algorithm"]["value"]
                f4["cpu_projected_wall_s"] = f4["total_iters"] / ref_v
                f4["cpu_projection"] = ("GPU fit's total Adam steps / CPU reference-algorithm steps/s at d=1000 "
                                        "(cov precomputed; the CPU's own X^T X at n=1e6 not included)")
                f4["vs_cpu_projected"] = f4["cpu_projected_wall_s"] / f4["wall_s"]
            line["full_fit_config4"] = f4
        if world == 1 and args.workload == "data" and not args.no_group:
            line["single_process"] = run_group_leg(args, 1)
        if fit_res is not None:
            fr = dict(fit_res)
            fr["workload"] = f"config2: DagmaLinear('l2').fit(X) defaults, d={d}, n={args.cov_n}, 1 GPU (cov mode)"
            if cpu and "reference_algorithm" in cpu:
                ref_v = cpu["reference_algorithm"]["value"]
                fr["cpu_projected_wall_s"] = fr["total_iters"] / ref_v
                fr["cpu_projection"] = ("GPU fit's total Adam steps / CPU reference-algorithm steps/s "
                                        "(SURVEY 8d: a d=1000 CPU fit is too long to run)")
                fr["vs_cpu_projected"] = fr["cpu_projected_wall_s"] / fr["wall_s"]
            line["full_fit"] = fr
        print(json.dumps(line), flush=True)
    beat("done")
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
