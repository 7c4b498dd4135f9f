"""All-pairs Pearson / Spearman on the GPU (`mi_tests.correlation_tests`, csrc/corr.hip) against the
host path it stands beside, `test_pairwise_independence(test="pearson" | "spearman")`: scipy once
per pair on a host copy of X (diagnostic; not part of bench.py).

For (d, n) in {(1000, 10^6), (100, 10^5)}, X from `utils.simulate_linear_sem_gpu` (a float64 CUDA
tensor), everything warm (one untimed call first), each timing taken twice:
  * `correlation_tests` for both tests: host clocks around the call, which returns host arrays;
  * its phases, each a host clock around a call that ends in a device synchronise:
      ranks      `solver.column_ranks` (the batched radix sort, tie runs, both transposes)
      corr       `solver.correlation` (column pass, centred staging, Gram, normalisation)
      gram_only  `solver.gram` on the same X: midagma_gram's staging without the centring and the
                 same GEMM, so corr - gram_only is what the column pass, the centring and the
                 normalisation add (reported as centring_derived)
      pvalues    the host p-values of the d x d matrix (`_stat_pvalue_from_rho`)
  * the sort's own bytes: per digit pass and key 8 B read by the histogram and 12 B read + 12 B
    written by the scatter, so 32 B x 8 passes x n x d if every pass is live, plus 8 B read and
    12 B written by the key transpose, 24 B by the tie pass and 16 B by the rank transpose; over
    the HBM rate of a float4 copy (6.29 TB/s) this gives the least time the passes could take,
    recorded beside the measured one.  The scatter's stores are 8- and 4-byte writes to 256 moving
    positions per wave, not full lines, which is where time above that bound goes;
  * the host path in the same session: the device-to-host copy of X, `scipy.stats.rankdata` on
    --cols columns, `pearsonr` and `spearmanr` on --pairs pairs, and their times PROJECTED to all
    d (d - 1) / 2 pairs (marked `projected`).

    python tools/probe_corr.py [--out profiles/corr_probe.json] [--sizes 1000x1000000 100x100000]
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

from midagma_amd import mi_tests, solver, utils  # noqa: E402

HBM_BYTES_PER_S = 6.29e12  # float4 copy, measured


def timed(fn, reps=2):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return out, r


def sort_bytes(n, d):
    per_key = 8 * 32 + (8 + 12) + 24 + 16
    return float(per_key) * n * d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_REPO, "profiles", "corr_probe.json"))
    ap.add_argument("--sizes", nargs="+", default=["1000x1000000", "100x100000"])
    ap.add_argument("--cols", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_corr: no GPU (a measurement has no CPU path)")
    from scipy import stats
    rows = []
    for size in a.sizes:
        d, n = (int(v) for v in size.split("x"))
        utils.set_random_seed(1)
        B = utils.simulate_dag(d, d, "ER")
        X = utils.simulate_linear_sem_gpu(utils.simulate_parameter(B), n, "gauss")
        row = dict(d=d, n=n, pairs=d * (d - 1) // 2)
        for T in ("pearson", "spearman"):
            mi_tests.correlation_tests(X, test=T)  # warm
            row[f"{T}_tests_s"], (stat, p) = timed(lambda: mi_tests.correlation_tests(X, test=T))
        row["ranks_s"], R = timed(lambda: solver.column_ranks(X))
        row["corr_s"], (rho, const) = timed(lambda: solver.correlation(X))
        row["corr_on_ranks_s"], _ = timed(lambda: solver.correlation(R))
        del R
        row["gram_only_s"], _ = timed(lambda: solver.gram(X))
        row["centring_derived_s"] = [c - g for c, g in zip(row["corr_s"], row["gram_only_s"])]
        rho_h = rho.cpu().numpy()
        for T in ("pearson", "spearman"):
            row[f"{T}_pvalues_s"], _ = timed(lambda: mi_tests._stat_pvalue_from_rho(rho_h, const, n, T))
        row["sort_bytes"] = sort_bytes(n, d)
        row["sort_hbm_bound_s"] = row["sort_bytes"] / HBM_BYTES_PER_S
        row["ranks_over_bound"] = min(row["ranks_s"]) / row["sort_hbm_bound_s"]
        # the host path
        row["d2h_s"], Xh = timed(lambda: X.cpu().numpy(), reps=1)
        k = min(a.cols, d)
        t = time.perf_counter()
        for c in range(k):
            stats.rankdata(Xh[:, c])
        row["host_rankdata_per_column_s"] = (time.perf_counter() - t) / k
        m = max(1, min(a.pairs, d - 1))
        for name, fn in (("pearsonr", stats.pearsonr), ("spearmanr", stats.spearmanr)):
            t = time.perf_counter()
            for j in range(1, m + 1):
                fn(Xh[:, 0], Xh[:, j])
            per = (time.perf_counter() - t) / m
            row[f"host_{name}_per_pair_s"] = per
            row[f"host_{name}_all_pairs_s_projected"] = per * row["pairs"] + row["d2h_s"][0]
        row["projected"] = ["host_pearsonr_all_pairs_s_projected", "host_spearmanr_all_pairs_s_projected"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del X, Xh
        torch.cuda.empty_cache()
    out = dict(note="tools/probe_corr.py on one MI355X, one process, warm; host clocks around calls that end in a "
                    "device synchronise, each taken twice; the host path's all-pairs times are projected from a few "
                    "pairs", device=torch.cuda.get_device_name(0), hbm_bytes_per_s=HBM_BYTES_PER_S, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
