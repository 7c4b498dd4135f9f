"""Timing of the GPU pairwise permutation tests (midagma_amd.mi_tests, csrc/indep.hip).  GPU only.

    python tools/probe_indep.py [--out FILE.json] [--reps 3] [--configs small,large] [--device-x]

Configurations: 'small' d = 20, n = 1000, P = 300 (the configuration of the reference's linear.py
__main__), 'large' d = 100, n = 1000, P = 200 and 'cap' d = 4, n = 16384 (the engine's cap on n),
P = 20 (only when named), every pair i < j, both statistics, both permutation sources.
--device-x: X is a torch CUDA tensor in every call (no host copy of X is uploaded).  Per
(configuration, statistic, source) it prints one JSON line with

  bandwidth_s      host medians for the RBF bandwidths (hsic; mi.median_sigma2 per variable)
  bandwidth_kernel_s  device medians: the median kernel (device events), best of --reps
  bandwidth_call_s    device medians: HipIndep.median_bandwidths end to end, best of --reps
  wall_hostx_hostbw_s / wall_hostx_devbw_s / wall_devx_devbw_s   (hsic, device permutations)
                   mi.permutation_null end to end with a host X and host medians (the path before
                   the device medians), a host X and device medians, a device X and device medians
  host_perm_s      numpy: drawing the permutations (rng.permutation), summed over the chunks
  host_stage_s     numpy: the library's range check and copy into pinned memory
  upload_s         numpy: host-to-device copies (device events on the copy stream)
  perm_kernel_s    device: the Philox rank kernel (device events)
  stat_kernel_s    the statistic kernels (device events)
  serial_wall_s    numpy: the chunks driven one after another (no overlap), wall clock
  wall_s           the public call, mi.permutation_null, end to end (numpy: generation overlapping
                   the device), best of --reps after a warm-up call
  terms_per_s      pairs * (P + 1) * n^2 / stat_kernel_s: permuted n^2-terms per second
  evals_per_s      kernel evaluations (exp for hsic, abs for dcor) the kernels execute -- whole
                   64 x 64 tiles of the upper triangle -- per second of stat_kernel_s

Stage times are sums over batches; batches overlap, so they may exceed the wall time.  The warm-up
call loads the code objects and sizes the buffers; every timed call ends in a device synchronise
inside the library."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

CONFIGS = {"small": (20, 1000, 300), "large": (100, 1000, 200), "cap": (4, 16384, 20)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="small,large")
    ap.add_argument("--device-x", action="store_true")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("probe_indep: no GPU (this probe has no CPU path)")
    from midagma_amd import mi_tests as mi
    from midagma_amd.solver import HipIndep

    rows = []
    for name in args.configs.split(","):
        d, n, P = CONFIGS[name]
        Xh = np.random.default_rng(0).standard_normal((n, d))
        Xd = torch.as_tensor(Xh).cuda()
        X = Xd if args.device_x else Xh
        pairs = np.array([(i, j) for i in range(d) for j in range(i + 1, d)], dtype=np.int64)
        m = len(pairs)
        nt = (n + 63) // 64
        evals = m * (P + 1) * (nt * (nt + 1) // 2) * 4096
        terms = m * (P + 1) * n * n
        for T in ("hsic", "dcor"):
            t0 = time.perf_counter()
            s2 = [mi.median_sigma2(Xh[:, v]) for v in range(d)] if T == "hsic" else None
            bw_s = time.perf_counter() - t0
            eng = HipIndep(X)
            extra = {}
            if s2 is not None:
                eng.median_bandwidths()  # warm-up: code object, buffers
                best_bw = None
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    got = eng.median_bandwidths()
                    w = time.perf_counter() - t0
                    if best_bw is None or w < best_bw[0]:
                        best_bw = (w, eng.bandwidth_ms() / 1e3)
                assert np.array_equal(got, s2), "device medians differ from the host's"
                extra = dict(bandwidth_call_s=best_bw[0], bandwidth_kernel_s=best_bw[1])
                for key, Xm, bw in (("wall_hostx_hostbw_s", Xh, "host"), ("wall_hostx_devbw_s", Xh, "device"),
                                    ("wall_devx_devbw_s", Xd, "device")):
                    ws = []
                    for _ in range(1 if (bw == "host" and n > 4096) else args.reps + 1):
                        t0 = time.perf_counter()
                        mi.permutation_null(Xm, pairs, test=T, num_perm=P, seed=1, perms="device", return_null=False,
                                            bandwidths=bw)
                        ws.append(time.perf_counter() - t0)
                    extra[key] = min(ws[1:]) if len(ws) > 1 else ws[0]
            eng.run(T, pairs[:8], P, None, seed=1)  # warm-up: code objects, pre-pass, buffers

            # device permutations: one library call
            best = None
            for _ in range(args.reps):
                t0 = time.perf_counter()
                eng.run(T, pairs, P, None, seed=1)
                w = time.perf_counter() - t0
                if best is None or w < best[0]:
                    best = (w, eng.profile())
            walls = []
            for _ in range(args.reps + 1):  # the first is the warm-up
                t0 = time.perf_counter()
                mi.permutation_null(X, pairs, test=T, num_perm=P, seed=1, perms="device", return_null=False)
                walls.append(time.perf_counter() - t0)
            pr = best[1]
            rows.append(dict(config=name, d=d, n=n, P=P, pairs=m, test=T, perms="device", bandwidth_s=bw_s,
                             perm_kernel_s=pr["perm_kernel_ms"] / 1e3, stat_kernel_s=pr["stat_kernel_ms"] / 1e3,
                             run_wall_s=best[0], wall_s=min(walls[1:]), terms_per_s=terms / (pr["stat_kernel_ms"] / 1e3),
                             evals_per_s=evals / (pr["stat_kernel_ms"] / 1e3), device_x=bool(args.device_x), **extra))
            print(json.dumps(rows[-1]), flush=True)

            # numpy permutations, the chunks one after another: the stage split
            chunk = max(1, mi._HOST_CHUNK_BYTES // (4 * P * n))
            rng = np.random.default_rng(1)
            acc = dict(host_perm=0.0, host_stage=0.0, upload=0.0, stat=0.0)
            t_all = time.perf_counter()
            for q0 in range(0, m, chunk):
                q1 = min(m, q0 + chunk)
                t0 = time.perf_counter()
                pm = mi._numpy_perms(rng, q1 - q0, P, n)
                acc["host_perm"] += time.perf_counter() - t0
                eng.run(T, pairs[q0:q1], P, pm)
                pr = eng.profile()
                acc["host_stage"] += pr["host_stage_ms"] / 1e3
                acc["upload"] += pr["upload_ms"] / 1e3
                acc["stat"] += pr["stat_kernel_ms"] / 1e3
            serial = time.perf_counter() - t_all
            eng.close()
            reps = args.reps if name == "small" else 1  # (large: the host draws for > 10 s per call)
            if name == "cap":
                continue  # (the numpy-stream call repeats the stage split above: nothing new at 6 pairs)
            walls = []
            for _ in range(reps):
                t0 = time.perf_counter()
                mi.permutation_null(X, pairs, test=T, num_perm=P, seed=1, perms="numpy", return_null=False)
                walls.append(time.perf_counter() - t0)
            rows.append(dict(config=name, d=d, n=n, P=P, pairs=m, test=T, perms="numpy", bandwidth_s=bw_s,
                             host_perm_s=acc["host_perm"], host_stage_s=acc["host_stage"], upload_s=acc["upload"],
                             stat_kernel_s=acc["stat"], serial_wall_s=serial, wall_s=min(walls),
                             terms_per_s=terms / acc["stat"], evals_per_s=evals / acc["stat"]))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
