"""Bootstrap edge frequencies from one X: `DagmaLinearBatch.bootstrap` (resampling and covariances on
the device, csrc/boot.hip) against the host route it replaces, `DagmaLinearBatch.fit` on B gathered
copies `X[bootstrap_indices(seed, b, n)]` (diagnostic; not part of bench.py).

For d in {20, 64}, n in {1000, 100000} and B in {64, 256, 1024}, default fit arguments:
  * the three kernels' times of one warm `HipBatch.boot_cov` from device events (`boot_profile`) and
    the weighted Gram's FP64 rate on 2 B n DS^2 flops (DS = 16, 32 or 64: the padded d; the kernel
    issues the blocks on and above the diagonal only, so the rate is on the nominal flops);
  * the wall time of `bootstrap` on a host X and on a device X (host clocks around the call, which
    returns host arrays);
  * the host route in the same process: measured in full where B n d doubles stay below
    --host-bytes (default 1 GiB), else projected: gather and `fit` of the first --prefix replicates
    give the preparation time per replicate, and the loop and final times are the bootstrap's own
    (the same batched loop on the same number of problems).
Everything runs warm (one untimed call of each kind per (d, n) first).

    python tools/probe_boot.py [--out profiles/boot_probe.json] [--d 20 64] [--n 1000 100000] [--B 64 256 1024]
"""
import argparse
import json
import os
import sys
import time

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from midagma_amd import DagmaLinearBatch, bootstrap_indices  # noqa: E402
from midagma_amd.simulate import make_dataset  # noqa: E402
from midagma_amd.solver import HipBatch  # noqa: E402

SEED = 7


def host_route(X, B):
    """(wall, gather seconds, the fitted model, W) of fit on the first B gathered resamples."""
    n = X.shape[0]
    t = time.perf_counter()
    Xs = [X[bootstrap_indices(SEED, b, n)] for b in range(B)]
    t_gather = time.perf_counter() - t
    m = DagmaLinearBatch()
    W = m.fit(Xs)
    return time.perf_counter() - t, t_gather, m, W


def compare(mh, mb, P):
    """The two routes on their first P replicates: the covariances' largest entrywise difference in
    units of 2^-53 sqrt(cov_ii cov_jj), and how many replicates took another retry schedule (a
    `minimize` that succeeds on one rounding of cov and fails on the other changes s and lr)."""
    worst, other = 0.0, 0
    for b in range(P):
        ch, cb = mh.cov[b], mb.cov[b]
        sd = np.sqrt(np.diag(ch))
        worst = max(worst, float((np.abs(ch - cb) / np.outer(sd, sd)).max()) / 2.0 ** -53)
        other += [(r["s"], r["lr"], r["success"]) for r in mh.minimize_log[b]] != \
            [(r["s"], r["lr"], r["success"]) for r in mb.minimize_log[b]]
    return worst, other


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_REPO, "profiles", "boot_probe.json"))
    ap.add_argument("--d", type=int, nargs="+", default=[20, 64])
    ap.add_argument("--n", type=int, nargs="+", default=[1000, 100000])
    ap.add_argument("--B", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--prefix", type=int, default=16)
    ap.add_argument("--host-bytes", type=int, default=1 << 30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_boot: no GPU (a measurement has no CPU path)")
    rows = []
    for d in a.d:
        DS = 16 if d <= 16 else (32 if d <= 32 else 64)
        for n in a.n:
            X = make_dataset(d, n, seed=1)[0]
            Xd = torch.from_numpy(X).cuda()
            DagmaLinearBatch().bootstrap(X, 2, seed=SEED)  # warm: code objects, caches, the allocator
            host_route(X, 2)
            for B in a.B:
                bt = HipBatch(d, B, device=0)
                bt.boot_cov(Xd, SEED)
                bt.boot_cov(Xd, SEED)
                prof = bt.boot_profile()
                bt.close()
                flops = 2.0 * B * n * DS * DS
                m = DagmaLinearBatch()
                t = time.perf_counter()
                m.bootstrap(X, B, seed=SEED)
                boot_wall = time.perf_counter() - t
                boot_t = dict(m.fit_timing)
                W_boot = m.W_boot
                md = DagmaLinearBatch()
                t = time.perf_counter()
                md.bootstrap(Xd, B, seed=SEED)
                boot_dev_wall = time.perf_counter() - t
                same_dev = bool(np.array_equal(md.W_boot, W_boot))
                full = B * n * d * 8 <= a.host_bytes
                if full:
                    host_wall, t_gather, mh, W_host = host_route(X, B)
                    ft, P = mh.fit_timing, B
                    prep_per = (t_gather + ft["prep_s"]) / B
                    same_support = bool(np.array_equal(W_host != 0, W_boot != 0))
                    max_dw = float(np.abs(W_host - W_boot).max())
                else:
                    P = min(a.prefix, B)
                    _, t_gather, mh, W_host = host_route(X, P)
                    ft = mh.fit_timing
                    prep_per = (t_gather + ft["prep_s"]) / P
                    host_wall = prep_per * B + boot_t["loop_s"] + boot_t["final_s"]
                    same_support = bool(np.array_equal(W_host != 0, W_boot[:P] != 0))
                    max_dw = float(np.abs(W_host - W_boot[:P]).max())
                cov_u, other = compare(mh, m, P)
                moved = int((np.abs(W_host - W_boot[:P]).reshape(P, -1).max(axis=1) > 1e-6).sum())
                row = dict(d=d, n=n, B=B, DS=DS, compared=P, cov_diff_ulps=cov_u, other_schedule=other,
                           replicates_moved_over_1e6=moved, host_loop_s=ft["loop_s"] if full else None, **prof,
                           gram_tflops=flops / (prof["gram_ms"] * 1e-3) / 1e12,
                           boot_wall_s=boot_wall, boot_prep_s=boot_t["prep_s"], boot_loop_s=boot_t["loop_s"],
                           boot_final_s=boot_t["final_s"], boot_device_x_wall_s=boot_dev_wall,
                           device_x_equal=same_dev, host_wall_s=host_wall, host_projected=not full,
                           host_prep_per_replicate_s=prep_per, host_over_boot=host_wall / boot_wall,
                           same_support=same_support, max_abs_dw=max_dw)
                rows.append(row)
                print(f"d={d} n={n} B={B:5d}: centre {prof['center_ms']:7.3f} counts {prof['counts_ms']:7.3f} "
                      f"gram {prof['gram_ms']:8.3f} ({row['gram_tflops']:.2f} TF/s) finish {prof['finish_ms']:6.3f} ms | "
                      f"bootstrap {boot_wall:7.3f} s (device X {boot_dev_wall:7.3f}) | host route"
                      f"{' (projected)' if not full else ''} {host_wall:8.3f} s | x{host_wall / boot_wall:.2f} "
                      f"support={same_support} max|dW|={max_dw:.2g} cov diff {cov_u:.1f} u, "
                      f"{other}/{P} other retry schedules, {moved}/{P} moved > 1e-6", flush=True)
    out = dict(note="tools/probe_boot.py on one MI355X, one process, warm: DagmaLinearBatch.bootstrap of "
                    "make_dataset(d, n, seed=1), default fit arguments, against fit() on the gathered resamples "
                    "(projected from a prefix where host_projected); kernel times from device events of one "
                    "boot_cov on a device X; wall times are host clocks",
               device=torch.cuda.get_device_name(0), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
