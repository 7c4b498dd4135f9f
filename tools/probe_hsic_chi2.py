"""The HSIC chi-square test of every pair (`HipHsic.all_pairs`, csrc/hsic.hip's tiled pass) against the
only other route to the same numbers, the permutation engine without permutations
(`HipHsic.run(all pairs, P=0)`: one workgroup group a pair, both factors streamed for every pair)
(diagnostic; not part of bench.py).

One process, everything warm (one untimed call first), each figure taken twice; the passes are timed
by the library's device events (`all_pairs_profile`, `profile`), the factorisation by its
synchronised host clock, and a host clock around the whole call is recorded beside them.  The case is
a gaussian linear SEM with d columns and n rows.  A case is d:n[:budget GiB[:cols]]: with `cols` only
the first `cols` columns run (one column group of a larger problem) and the whole problem is
PROJECTED: the tiled pass by the number of tiles on and above the diagonal at the measured mean
r_pad, the factorisation and the vectors by d / cols; such a row is marked `projected`.  The yardstick
runs every pair up to --max-pairs and a subset of --subset pairs beyond, scaled and marked.

Per case: the shares of factorisation, tiled pass and vectors, the ranks, R = sum r_pad, the
algorithmic flops n R^2 (the upper triangle, 2 flops a multiply-add) and their fraction of --peak-tf
(the FP64 matrix peak the project uses), the executed flops (whole 128 x 128 tiles on and above the
diagonal), and the yardstick's time with the ratio.

    python tools/probe_hsic_chi2.py [--out profiles/hsic_chi2_probe.json] [--cases 20:100000 ...]
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

from midagma_amd import utils  # noqa: E402
from midagma_amd.solver import HipHsic  # noqa: E402

TILE = 128


def make_x(d, n):
    utils.set_random_seed(1)
    B = utils.simulate_dag(d, d, "ER")
    return utils.simulate_linear_sem_gpu(utils.simulate_parameter(B), n, "gauss")


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


def tiles_upper(R):
    t = -(-R // TILE)
    return t * (t + 1) // 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_REPO, "profiles", "hsic_chi2_probe.json"))
    ap.add_argument("--cases", nargs="*", default=["20:100000", "100:100000", "100:100000:16", "1000:10000:24",
                                                   "1000:1000000:64:48"])
    ap.add_argument("--peak-tf", type=float, default=78.0, help="the FP64 matrix peak, TFLOP/s")
    ap.add_argument("--max-pairs", type=int, default=5000)
    ap.add_argument("--subset", type=int, default=2000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_hsic_chi2: no GPU (a measurement has no CPU path)")
    rows = []
    for spec in a.cases:
        f = spec.split(":")
        d, n = int(f[0]), int(f[1])
        budget = int(float(f[2]) * 2**30) if len(f) > 2 else 0
        k = int(f[3]) if len(f) > 3 else d
        X = make_x(k, n)  # (a column group of a larger problem: the SEM of its columns alone)
        row = dict(d=d, n=n, cols=k, budget_bytes=budget, projected=k < d)
        HipHsic(X[:, :2]).close()  # warm
        row["set_data_s"], eng = wall(lambda: HipHsic(X))
        try:
            row["median_s"], _ = wall(lambda: eng.median_bandwidths())
            eng.all_pairs([0, 1], budget_bytes=budget)  # warm
            calls, prof = [], []
            for _ in range(2):
                eng.median_bandwidths()  # drop the factors: a timed call factors every column
                t, out = wall(lambda: eng.all_pairs(budget_bytes=budget))
                calls.append(t)
                prof.append(eng.all_pairs_profile())
            rank, _ = eng.factor(np.arange(k))
            rp = (rank.astype(np.int64) + 15) // 16 * 16
            R = int(rp.sum())
            best = int(np.argmin(calls))
            row.update(all_pairs_call_s=calls, factor_s=[p["factor_ms"] / 1e3 for p in prof],
                       tile_s=[p["tile_ms"] / 1e3 for p in prof], vector_s=[p["vector_ms"] / 1e3 for p in prof],
                       rank_min=int(rank.min()), rank_max=int(rank.max()), R=R)
            tile = row["tile_s"][best]
            algo = float(n) * R * R
            done = 2.0 * n * TILE * TILE * tiles_upper(R)
            row.update(algorithmic_flops=algo, executed_flops=done, algorithmic_tflops=algo / tile / 1e12,
                       fraction_of_fp64_matrix_peak=algo / tile / 1e12 / a.peak_tf,
                       executed_tflops=done / tile / 1e12)
            # the yardstick: the parent commit's only route to the same numbers
            i, j = np.triu_indices(k, 1)
            pairs = np.stack([i, j], axis=1).astype(np.int64)
            sub = pairs if len(pairs) <= a.max_pairs else pairs[np.linspace(0, len(pairs) - 1, a.subset).astype(int)]
            eng.run(sub[:1], 0, budget_bytes=budget)  # warm
            ys, ye = [], []
            for _ in range(2):
                t, old = wall(lambda: eng.run(sub, 0, budget_bytes=budget))
                ys.append(t)
                ye.append(eng.profile()["eval_ms"] / 1e3)
            scale = len(pairs) / len(sub)
            row.update(yardstick_pairs=len(sub), yardstick_projected=len(sub) < len(pairs),
                       yardstick_call_s=[t * scale for t in ys], yardstick_eval_s=[t * scale for t in ye])
            if len(sub) == len(pairs):
                row["max_abs_biased_difference"] = float(np.abs(out[1][i, j] - old[0]).max())
            row["speedup_pass_over_yardstick_eval"] = min(row["yardstick_eval_s"]) / (tile + row["vector_s"][best])
            if k < d:  # the whole problem from one column group
                Rd = int(round(R / k * d))
                row["projection"] = dict(
                    R=Rd, tile_s=tile * tiles_upper(Rd) / tiles_upper(R), factor_s=row["factor_s"][best] * d / k,
                    vector_s=row["vector_s"][best] * d / k,
                    yardstick_eval_s=min(ye) / len(sub) * (d * (d - 1) // 2))
        finally:
            eng.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
        del X
        torch.cuda.empty_cache()
    out = dict(note="tools/probe_hsic_chi2.py on one MI355X, one process, warm, each figure twice; tile_s and vector_s "
                    "are device events summed over the batches, factor_s a host clock around the synchronised "
                    "factorisation, *_call_s host clocks around calls that return host arrays; yardstick = "
                    "HipHsic.run(pairs, P=0), scaled by pairs / subset where yardstick_projected; algorithmic flops "
                    f"n R^2 against {a.peak_tf:.0f} TFLOP/s; rows with projected = true measured `cols` columns "
                    "and hold a `projection` for d",
               device=torch.cuda.get_device_name(0), cases=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
