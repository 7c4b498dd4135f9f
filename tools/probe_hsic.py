"""HSIC permutation tests from low-rank factors (`mi_tests.hsic_null`, csrc/hsic.hip) against the
n^2 kernel they stand beside (`permutation_null(test="hsic", perms="device")`, csrc/indep.hip), and at
the sizes the n^2 kernel cannot take (diagnostic; not part of bench.py).

One process, everything warm (one untimed call first), each figure taken twice, host clocks around
calls that return host arrays (so every call ends in a device synchronise).  The case is a gaussian
linear SEM with d = 20, P = 300 device permutations a pair, every pair, at n in --sizes; at a size
given as n:pairs only the first `pairs` pairs run and the all-pairs time is PROJECTED as
set_data + median + (factor + evaluation) * pairs / subset (an over-estimate of the factor share: all
20 columns are factored for any subset that touches them) and marked `projected`.  Per size: wall
time, its split into set_data (copy and sort), medians, factorisation, permutations and evaluation
(`HipHsic.profile`), the ranks, the bytes of Gc rows gathered an evaluation and the achieved
fraction of --peak-gbs (the device's memory bandwidth) in the evaluation kernel.  At n <= 16384 the
n^2 kernel is timed on the same X in the same session.

    python tools/probe_hsic.py [--out profiles/hsic_probe.json] [--sizes 1000 16384 100000 1000000:19]
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

from midagma_amd import mi_tests, utils  # noqa: E402
from midagma_amd.solver import HipHsic  # noqa: E402

P = 300
D = 20


def timed(fn, reps=2):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return out, r


def make_x(d, n):
    utils.set_random_seed(1)
    B = utils.simulate_dag(d, d, "ER")
    return utils.simulate_linear_sem_gpu(utils.simulate_parameter(B), n, "gauss")


def all_pairs(d):
    i, j = np.triu_indices(d, 1)
    return np.stack([i, j], axis=1).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_REPO, "profiles", "hsic_probe.json"))
    ap.add_argument("--sizes", nargs="*", default=["1000", "16384", "100000", "1000000:19"])
    ap.add_argument("--n2-sizes", nargs="*", type=int, default=[1000, 16384])
    ap.add_argument("--peak-gbs", type=float, default=8000.0, help="the device's memory bandwidth, GB/s")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_hsic: no GPU (a measurement has no CPU path)")
    rows = []
    for spec in a.sizes:
        n, _, sub = spec.partition(":")
        n = int(n)
        X = make_x(D, n)
        pairs = all_pairs(D)
        subset = pairs[:min(int(sub), len(pairs))] if sub else pairs
        row = dict(d=D, n=n, P=P, pairs=len(pairs), subset=len(subset))
        HipHsic(X[:, :2]).close()  # warm
        row["set_data_s"], eng = timed(lambda: HipHsic(X), reps=1)
        try:
            row["median_s"], _ = timed(lambda: eng.median_bandwidths())
            eng.run(subset[:1], 3, None, 0)  # warm (and the factors of two columns)
            eng.median_bandwidths()          # drop them: the timed runs factor every column again
            runs, prof = [], []
            for _ in range(2):
                t, _ = timed(lambda: eng.run(subset, P, None, 0), reps=1)
                runs.append(t[0])
                prof.append(eng.profile())
                eng.median_bandwidths()
            rank, resid = eng.factor(np.unique(subset))
        finally:
            eng.close()
        best = int(np.argmin(runs))
        row["run_subset_s"] = runs
        row["factor_s"] = [p["factor_ms"] / 1e3 for p in prof]
        row["perm_s"] = [p["perm_ms"] / 1e3 for p in prof]
        row["eval_s"] = [p["eval_ms"] / 1e3 for p in prof]
        row["ranks"] = rank.tolist()
        row["largest_residual"] = float(resid.max())
        rp = dict(zip(np.unique(subset).tolist(), ((rank.astype(np.int64) + 15) // 16 * 16).tolist()))
        evals = len(subset) * (P + 1)
        # the two factors' rows of every evaluation (that Fc's are loaded once a group of 4 is not credited)
        gathered = float(sum(n * 8 * (rp[int(i)] + rp[int(j)]) for i, j in subset)) * (P + 1)
        row["us_per_evaluation"] = row["eval_s"][best] / evals * 1e6
        row["gather_gb_per_s"] = gathered / row["eval_s"][best] / 1e9
        row["fraction_of_peak_bandwidth"] = row["gather_gb_per_s"] / a.peak_gbs
        scale = len(pairs) / len(subset)
        row["all_pairs_s"] = (row["set_data_s"][0] + min(row["median_s"]) + runs[best] * scale)
        row["projected"] = len(subset) < len(pairs)
        if n in a.n2_sizes and n <= 16384:
            mi_tests.permutation_null(X, pairs[:2], test="hsic", num_perm=3, perms="device", return_null=False)  # warm
            row["n2_kernel_s"], old = timed(lambda: mi_tests.permutation_null(X, pairs, test="hsic", num_perm=P,
                                                                              perms="device", return_null=False))
            new = mi_tests.hsic_null(X, pairs, num_perm=0, return_null=False)
            row["speedup_over_n2"] = min(row["n2_kernel_s"]) / row["all_pairs_s"]
            row["max_abs_stat_difference"] = float(np.abs(new[0] - old[0]).max())
        rows.append(row)
        print(json.dumps(row), flush=True)
        del X
        torch.cuda.empty_cache()
    out = dict(note="tools/probe_hsic.py on one MI355X, one process, warm; host clocks around calls that end in a "
                    "device synchronise, each taken twice (set_data once); factor_s is a host clock around the "
                    "synchronised factorisation, perm_s and eval_s are device events summed over the batches; "
                    "all_pairs_s = set_data + median + run, the run scaled by pairs / subset where `projected` is "
                    "true; fraction_of_peak_bandwidth counts the two factors' rows of every evaluation against "
                    f"{a.peak_gbs:.0f} GB/s",
               device=torch.cuda.get_device_name(0), sizes=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
