"""Many small-d logistic fits at once: `DagmaLogisticBatch` against a sequential loop over
`DagmaLinear("logistic").fit` (diagnostic; not part of bench.py).

Binary X from the logistic SEM, make_dataset(20, 1000, seed=b, sem_type="logistic"), default `fit`
arguments.  Legs, all in one process on one GPU, everything warm (one untimed short fit of each
kind first):

  sequential  `DagmaLinear("logistic").fit` (the large-tile launch chain) on the first `--seq-fits`
              problems: wall time and Adam steps of each; larger B are projected from their mean.
  fit         `DagmaLogisticBatch.fit` at every B, `--repeat` timed passes (all reported): wall
              time, aggregate Adam steps/s, and, for the problems the sequential leg ran, whether
              the thresholded support equals the sequential fit's.
  grid        B = 256 on one X: the lambda1 grid stored once (shared) against 256 copies of X.
  slot        the device's own clock: `HipBatch.minimize_logistic` for `--slot-steps` Adam steps
              without early stop, steps/s per problem from the last checkpoint record's `elapsed`
              (the device real-time counter from the call's first slot) at B = 1, 256, 1024, and
              one point at n = 10^4 (B = 1 and 256), where one workgroup per problem stops paying.

Wall times are host clocks around `fit`, which returns host arrays (the device work has ended); the
data is generated and copied outside the timed window.

    python tools/probe_batch_logistic.py [--out profiles/batch_logistic_probe.json] [--B 1 16 256 1024]
"""
import argparse
import json
import os
import sys
import time

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401

from midagma_amd import DagmaLinear, DagmaLogisticBatch  # noqa: E402
from midagma_amd.simulate import make_dataset  # noqa: E402
from midagma_amd.solver import HipBatch  # noqa: E402

D, N = 20, 1000


def _data(seed, n=N):
    return make_dataset(D, n, seed=seed, sem_type="logistic")[0]


def _steps(m):
    return sum(r["iters"] for log in m.minimize_log for r in log)


def slot_rate(Xs, shared, steps, lam=0.03):
    """Adam steps/s of one problem by the device clock, `steps` steps without early stop: (the
    slowest problem's, the median over the problems)."""
    B = len(Xs)
    bt = HipBatch(D, B, device=0)
    try:
        covs = {}
        for X in Xs:
            if id(X) not in covs:
                covs[id(X)] = X.T @ X / float(X.shape[0])
        bt.set_cov(np.stack([covs[id(X)] for X in Xs]))
        bt.set_data(Xs[0] if shared else np.stack(Xs), shared=shared)
        W = np.zeros((B, D, D))
        bt.minimize_logistic(W, 1.0, 1.0, 3e-4, lam, 200, tol=-1.0, checkpoint=100)  # warm
        W[:] = 0.0
        t = time.perf_counter()
        res = bt.minimize_logistic(W, 1.0, 1.0, 3e-4, lam, steps, tol=-1.0, checkpoint=steps)
        wall = time.perf_counter() - t
        assert all(r.iters == steps for r in res)
        el = np.array([bt.checkpoints(b)[-1].elapsed for b in range(0, B, max(1, B // 64))])
    finally:
        bt.close()
    return dict(B=B, n=int(Xs[0].shape[0]), shared=bool(shared), steps=steps, wall_s=wall,
                device_steps_per_s_slowest=steps / float(el.max()),
                device_steps_per_s_median=steps / float(np.median(el)),
                device_us_per_step_median=1e6 * float(np.median(el)) / steps,
                aggregate_steps_per_s_wall=B * steps / wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_REPO, "profiles", "batch_logistic_probe.json"))
    ap.add_argument("--B", type=int, nargs="+", default=[1, 16, 256, 1024])
    ap.add_argument("--seq-fits", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--slot-steps", type=int, default=20000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_batch_logistic: no GPU (a measurement has no CPU path)")
    out = dict(note="tools/probe_batch_logistic.py on one MI355X, one process: default fit() of make_dataset(20, 1000, "
                    "seed=b, sem_type='logistic'); DagmaLogisticBatch (one workgroup per problem, X streamed in row "
                    "blocks) against a sequential DagmaLinear('logistic').fit loop (the large-tile launch chain; measured "
                    "on seq_fits problems, projected beyond); wall times are host clocks around fit(); the slot leg "
                    "reads the device's real-time counter from the checkpoint records",
               device=torch.cuda.get_device_name(0), d=D, n=N)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    data = [_data(b) for b in range(max(a.B))]
    # warm: code objects of both paths, the library's caches, the allocator
    short = dict(T=2, warm_iter=500, max_iter=500)
    DagmaLinear("logistic").fit(_data(10_000), **short)
    DagmaLogisticBatch().fit([_data(10_000 + k) for k in range(2)], **short)

    seq_t, seq_steps, seq_W = [], [], []
    for b in range(min(a.seq_fits, max(a.B))):
        m = DagmaLinear("logistic")
        X = data[b].copy()
        t = time.perf_counter()
        seq_W.append(m.fit(X))
        seq_t.append(time.perf_counter() - t)
        seq_steps.append(sum(r["iters"] for r in m.minimize_log))
        print(f"sequential fit {b}: {seq_t[-1]:.2f} s, {seq_steps[-1]} steps", flush=True)
    out.update(seq_fit_wall_s=seq_t, seq_fit_steps=seq_steps, seq_steps_per_s=sum(seq_steps) / sum(seq_t))
    save()

    rows = []
    for rep in range(a.repeat):
        for B in a.B:
            if rep > 0 and B > 256:
                continue  # (the largest batch is timed once)
            Xs = [data[b].copy() for b in range(B)]
            m = DagmaLogisticBatch()
            t = time.perf_counter()
            W = m.fit(Xs)
            dt = time.perf_counter() - t
            steps, nb = _steps(m), min(B, len(seq_t))
            seq_wall = sum(seq_t[:nb]) * (B / nb)
            same = [bool(np.array_equal(W[b] != 0, seq_W[b] != 0)) for b in range(nb)]
            rows.append(dict(B=B, repeat=rep, batch_wall_s=dt, batch_loop_s=m.fit_timing["loop_s"],
                             batch_fits_per_s=B / dt, batch_steps=steps, batch_steps_per_s=steps / dt,
                             seq_wall_s=seq_wall, seq_fits_measured=nb, seq_projected=B > nb, speedup=seq_wall / dt,
                             same_support_as_sequential=same))
            print(f"B={B:5d} #{rep}: batch {dt:8.3f} s {B / dt:8.2f} fits/s {steps / dt:11.0f} steps/s | sequential"
                  f"{' (projected)' if B > nb else ''} {seq_wall:8.2f} s | x{seq_wall / dt:.1f}  same support: "
                  f"{sum(same)}/{nb}", flush=True)
            out["fit_rows"] = rows
            save()

    # one X, a lambda1 grid of 256: stored once against 256 copies
    X, lams = data[0], list(np.linspace(0.005, 0.1, 256))
    grid = []
    for shared in (True, False, True, False):
        m = DagmaLogisticBatch()
        arg = X.copy() if shared else [X.copy() for _ in lams]
        t = time.perf_counter()
        m.fit(arg, lambda1=lams)
        dt = time.perf_counter() - t
        grid.append(dict(B=256, shared=shared, wall_s=dt, loop_s=m.fit_timing["loop_s"], prep_s=m.fit_timing["prep_s"],
                         steps=_steps(m), steps_per_s=_steps(m) / dt))
        print(f"grid B=256 shared={shared}: {dt:.3f} s, {_steps(m) / dt:.0f} steps/s", flush=True)
        out["grid_rows"] = grid
        save()

    slot = []
    for B in (1, 256, 1024):
        slot.append(slot_rate([data[b] for b in range(B)], False, a.slot_steps))
        print("slot", slot[-1], flush=True)
    slot.append(slot_rate([data[0]] * 256, True, a.slot_steps))
    print("slot", slot[-1], flush=True)
    big = [_data(20_000 + b, n=10_000) for b in range(4)]
    for B in (1, 256):
        slot.append(slot_rate([big[b % 4].copy() for b in range(B)], False, max(a.slot_steps // 10, 200)))
        print("slot", slot[-1], flush=True)
    out["slot_rows"] = slot
    # the launch chain's rate at n = 10^4 for the same point
    m = DagmaLinear("logistic")
    t = time.perf_counter()
    m.fit(big[0].copy(), T=1, max_iter=2000, warm_iter=2000)
    dt = time.perf_counter() - t
    st = sum(r["iters"] for r in m.minimize_log)
    out["seq_n10000"] = dict(steps=st, wall_s=dt, steps_per_s=st / dt)
    print("sequential n=10^4:", out["seq_n10000"], flush=True)
    save()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
