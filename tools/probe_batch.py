"""Many small-d default fits at once: `DagmaLinearBatch` against a sequential loop over
`DagmaLinear.fit` (diagnostic; not part of bench.py).

For d in {20, 32, 64} and B in {1, 16, 64, 256, 512, 1024}: default `fit`s of
make_dataset(d, 1000, seed=b), b < B.  Reports fits/s and aggregate Adam steps/s (the steps of
every minimize call, retries included) of the batched fit, its critical path in steps (the sum
over minimize calls of the slowest problem's steps), and the sequential loop: measured
for B <= 64 (one timed pass over the first 64 problems; B = 1 and 16 are its prefixes), projected
from the 64-problem rate beyond.  Wall times are host clocks around `fit`, which returns host
arrays (the device work has ended); the data is generated before and copied outside the timed
window.  Everything runs warm (one untimed fit of each kind per d first), in one process.

    python tools/probe_batch.py [--out profiles/batch_probe.json] [--d 20 32 64] [--B 1 16 ...]

`--trek pst` is a leg of its own (profiles/batch_trek_probe.json): default `fit`s at d = 20, n = 1000
with the PST regularizer (exp / mean, weight 0.1, 30 % of the upper-triangle pairs) for B in {1, 256},
the one-workgroup body (csrc/pst_blk.h) in the batch against a sequential loop over
`DagmaLinear(trek_reg=...).fit`, which runs the launch chain (csrc/trek.hip).  The sequential loop is
measured on the first `--seq-fits` problems and projected beyond; every batch size is timed
`--repeat` times, alternating, and all repeats are reported.

    python tools/probe_batch.py --trek pst [--out profiles/batch_trek_probe.json] [--B 1 256] [--seq-fits 3]
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401

from midagma_amd import DagmaLinear, DagmaLinearBatch  # noqa: E402
from midagma_amd.simulate import make_dataset  # noqa: E402

SEQ_MAX = 64


def _pst(d, weight=0.1, frac=0.3, seed=0):
    """A PSTRegularizer-like object (exp / mean, 'opt') over `frac` of the upper-triangle pairs."""
    iu = np.array(np.triu_indices(d, 1)).T
    pairs = iu[np.random.default_rng(seed).uniform(size=len(iu)) < frac]
    return SimpleNamespace(name="pst", mode="opt", weight=weight, enabled=lambda: True,
                           cfg={"I": pairs, "seq": "exp", "kwargs": {"agg": "mean"}})


def trek_leg(a):
    d = 20
    Bs = a.B or [1, 256]
    out_path = a.out or os.path.join(_REPO, "profiles", "batch_trek_probe.json")
    data = [make_dataset(d, 1000, seed=b)[0] for b in range(max(Bs))]
    reg = _pst(d)
    # warm: code objects of both paths, the library's caches, the allocator
    DagmaLinear("l2", trek_reg=reg).fit(make_dataset(d, 1000, seed=10_000)[0], T=2, warm_iter=500, max_iter=500)
    DagmaLinearBatch(trek_reg=reg).fit([make_dataset(d, 1000, seed=10_000 + k)[0] for k in range(2)])
    seq_t, seq_steps, seq_W = [], [], []
    for b in range(min(a.seq_fits, max(Bs))):
        X = data[b].copy()
        m = DagmaLinear("l2", trek_reg=reg)
        t = time.perf_counter()
        seq_W.append(m.fit(X))
        seq_t.append(time.perf_counter() - t)
        seq_steps.append(sum(r["iters"] for r in m.minimize_log))
        print(f"sequential fit {b}: {seq_t[-1]:.2f} s, {seq_steps[-1]} steps", flush=True)
    rows = []
    for rep in range(a.repeat):
        for B in Bs:
            Xs = [data[b].copy() for b in range(B)]
            m = DagmaLinearBatch(trek_reg=reg)
            t = time.perf_counter()
            W = m.fit(Xs)
            dt = time.perf_counter() - t
            steps = sum(r["iters"] for log in m.minimize_log for r in log)
            nb = min(B, len(seq_t))
            seq_wall = sum(seq_t[:nb]) * (B / nb)
            dev = max(float(np.abs(W[b] - seq_W[b]).max()) for b in range(nb))
            rows.append(dict(d=d, B=B, repeat=rep, batch_wall_s=dt, batch_loop_s=m.fit_timing["loop_s"],
                             batch_fits_per_s=B / dt, batch_steps=steps, batch_steps_per_s=steps / dt,
                             seq_wall_s=seq_wall, seq_fits_measured=nb, seq_projected=B > nb,
                             seq_fits_per_s=B / seq_wall, seq_steps_per_s=sum(seq_steps[:nb]) / sum(seq_t[:nb]),
                             speedup=seq_wall / dt, max_abs_dW_vs_sequential=dev))
            print(f"trek pst d={d} B={B:4d} #{rep}: batch {dt:8.3f} s {B / dt:8.2f} fits/s {steps / dt:11.0f} steps/s | "
                  f"sequential{' (projected)' if B > nb else ''} {seq_wall:8.2f} s {B / seq_wall:6.3f} fits/s | "
                  f"x{seq_wall / dt:.1f}  max|dW|={dev:.1e}", flush=True)
    out = dict(note="tools/probe_batch.py --trek pst on one MI355X, one process: default fit() of make_dataset(20, 1000, "
                    "seed=b) with PST exp/mean/opt, weight 0.1, 30 % of the upper-triangle pairs; DagmaLinearBatch "
                    "(the one-workgroup body) against a sequential DagmaLinear(trek_reg).fit loop (the launch chain; "
                    "measured on seq_fits_measured problems, projected beyond); wall times are host clocks around "
                    "fit(), which returns host arrays",
               device=torch.cuda.get_device_name(0), seq_fit_wall_s=seq_t, seq_fit_steps=seq_steps, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--d", type=int, nargs="+", default=[20, 32, 64])
    ap.add_argument("--B", type=int, nargs="+", default=None)
    ap.add_argument("--trek", choices=["pst"], default=None, help="the leg with the PST trek regularizer")
    ap.add_argument("--seq-fits", type=int, default=3, help="--trek: sequential fits measured")
    ap.add_argument("--repeat", type=int, default=2, help="--trek: timed passes over the batch sizes")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_batch: no GPU (a measurement has no CPU path)")
    if a.trek:
        return trek_leg(a)
    a.out = a.out or os.path.join(_REPO, "profiles", "batch_probe.json")
    a.B = a.B or [1, 16, 64, 256, 512, 1024]
    rows = []
    for d in a.d:
        data = [make_dataset(d, 1000, seed=b)[0] for b in range(max(a.B))]
        # warm: code objects, the library's caches, the allocator
        DagmaLinear("l2").fit(make_dataset(d, 1000, seed=10_000)[0])
        DagmaLinearBatch().fit([make_dataset(d, 1000, seed=10_000 + k)[0] for k in range(2)])
        # the sequential loop, one pass: per-fit wall time and Adam steps of problems 0..63
        seq_t, seq_steps, seq_W = [], [], []
        for b in range(min(SEQ_MAX, max(a.B))):
            X = data[b].copy()
            m = DagmaLinear("l2")
            t = time.perf_counter()
            seq_W.append(m.fit(X))
            seq_t.append(time.perf_counter() - t)
            seq_steps.append(sum(r["iters"] for r in m.minimize_log))
        print(f"d={d}: sequential {len(seq_t)} fits in {sum(seq_t):.2f} s", flush=True)
        for B in a.B:
            Xs = [data[b].copy() for b in range(B)]
            m = DagmaLinearBatch()
            t = time.perf_counter()
            W = m.fit(Xs)
            dt = time.perf_counter() - t
            steps = sum(r["iters"] for log in m.minimize_log for r in log)
            # the lockstep critical path: every minimize call lasts as long as its slowest problem
            crit: dict = {}
            for log in m.minimize_log:
                seen: dict = {}
                for r in log:
                    k = (r["mu"], seen.setdefault(r["mu"], 0))
                    seen[r["mu"]] += 1
                    crit[k] = max(crit.get(k, 0), r["iters"])
            same = all(np.array_equal(W[b], seq_W[b]) for b in range(min(B, len(seq_W))))
            nb = min(B, len(seq_t))
            seq_wall = sum(seq_t[:nb]) * (B / nb)  # measured up to 64 problems, projected beyond
            row = dict(d=d, B=B, batch_wall_s=dt, batch_loop_s=m.fit_timing["loop_s"], batch_fits_per_s=B / dt,
                       batch_steps=steps, batch_steps_per_s=steps / dt, batch_critical_steps=sum(crit.values()),
                       minimize_calls=max(len(log) for log in m.minimize_log),
                       seq_wall_s=seq_wall, seq_projected=B > nb, seq_fits_per_s=B / seq_wall,
                       seq_steps_per_s=sum(seq_steps[:nb]) / sum(seq_t[:nb]), speedup=seq_wall / dt,
                       equal_to_sequential=bool(same))
            rows.append(row)
            print(f"d={d} B={B:5d}: batch {dt:8.3f} s {B / dt:9.1f} fits/s {steps / dt:12.0f} steps/s | "
                  f"sequential{' (projected)' if B > nb else ''} {seq_wall:8.2f} s {B / seq_wall:7.2f} fits/s | "
                  f"x{seq_wall / dt:.1f}  equal={same}", flush=True)
    out = dict(note="tools/probe_batch.py on one MI355X, one process: default fit() of make_dataset(d, 1000, seed=b), "
                    "DagmaLinearBatch against a sequential DagmaLinear.fit loop (measured to 64 problems, projected "
                    "beyond); wall times are host clocks around fit()",
               device=torch.cuda.get_device_name(0), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
