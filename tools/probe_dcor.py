"""dCor permutation tests without the n^2 sum (`mi_tests.dcor_null` / `dcor_tests`, csrc/dcor.hip)
against the n^2 kernel they stand beside (`permutation_null(test="dcor", perms="device")`,
csrc/indep.hip), and at the sizes the n^2 kernel cannot take (diagnostic; not part of bench.py).

One process, everything warm (one untimed call first), each figure taken twice, host clocks around
calls that return host arrays (so every call ends in a device synchronise):
  * compare: `dcor_null(perms="device")` and `permutation_null(test="dcor", perms="device")` on
    every pair of the same X (gaussian linear SEM, d = 20, P = 300) at n in {1000, 16384};
  * sizes: the per-column pre-pass (`HipDcor(X)`: argsort, centring, row sums) and the run of a
    pair subset, for (d, n, pvalue) in --sizes; when the subset is smaller than all d (d - 1) / 2
    pairs the all-pairs time is PROJECTED as prepass + run * pairs / subset and listed under
    `projected`.  pvalue "perm" runs P = 300 device permutations a pair, "chi2" one evaluation.

    python tools/probe_dcor.py [--out profiles/dcor_probe.json] [--sizes 20x100000:perm:190 ...]
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

from midagma_amd import _lib, mi_tests, utils  # noqa: E402
from midagma_amd.solver import HipDcor  # noqa: E402

P = 300


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
    ap.add_argument("--out", default=os.path.join(_REPO, "profiles", "dcor_probe.json"))
    ap.add_argument("--compare", nargs="*", type=int, default=[1000, 16384])
    ap.add_argument("--sizes", nargs="*", default=["20x100000:perm:190", "20x1000000:perm:19", "100x100000:perm:200",
                                                   "1000x1000000:chi2:2000"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_dcor: no GPU (a measurement has no CPU path)")
    compare, sizes = [], []
    for n in a.compare:
        X = make_x(20, n)
        pairs = all_pairs(20)
        row = dict(d=20, n=n, P=P, pairs=len(pairs), block=int(_lib.lib().midagma_dcor_block(n)))
        mi_tests.dcor_null(X, pairs[:2], num_perm=3, perms="device", return_null=False)  # warm
        mi_tests.permutation_null(X, pairs[:2], test="dcor", num_perm=3, perms="device", return_null=False)
        row["dcor_null_s"], new = timed(lambda: mi_tests.dcor_null(X, pairs, num_perm=P, perms="device",
                                                                   return_null=False))
        row["permutation_null_s"], old = timed(lambda: mi_tests.permutation_null(X, pairs, test="dcor", num_perm=P,
                                                                                 perms="device", return_null=False))
        row["speedup"] = min(row["permutation_null_s"]) / min(row["dcor_null_s"])
        row["max_abs_stat_difference"] = float(np.abs(new[0] - old[0]).max())
        compare.append(row)
        print(json.dumps(row), flush=True)
        del X
    for spec in a.sizes:
        shape, pvalue, sub = spec.split(":")
        d, n = (int(v) for v in shape.split("x"))
        X = make_x(d, n)
        pairs = all_pairs(d)
        subset = pairs[:min(int(sub), len(pairs))]
        nperm, unbiased = (P, False) if pvalue == "perm" else (0, True)
        row = dict(d=d, n=n, pvalue=pvalue, P=nperm, pairs=len(pairs), subset=len(subset))
        HipDcor(X[:, :2]).close()  # warm
        row["prepass_s"], eng = timed(lambda: HipDcor(X), reps=1)
        try:
            eng.run(subset[:1], min(nperm, 2), None, 0, unbiased=unbiased)  # warm
            row["run_subset_s"], _ = timed(lambda: eng.run(subset, nperm, None, 0, unbiased=unbiased))
        finally:
            eng.close()
        per_eval = min(row["run_subset_s"]) / (len(subset) * (nperm + 1))
        row["us_per_evaluation"] = per_eval * 1e6
        row["all_pairs_s"] = row["prepass_s"][0] + min(row["run_subset_s"]) * len(pairs) / len(subset)
        row["projected"] = len(subset) < len(pairs)
        sizes.append(row)
        print(json.dumps(row), flush=True)
        del X
        torch.cuda.empty_cache()
    out = dict(note="tools/probe_dcor.py on one MI355X, one process, warm; host clocks around calls that end in a "
                    "device synchronise, each taken twice (the pre-pass once); all_pairs_s is projected from the "
                    "pair subset where `projected` is true", device=torch.cuda.get_device_name(0), compare=compare,
               sizes=sizes)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
