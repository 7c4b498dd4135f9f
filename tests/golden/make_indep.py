"""Fixtures for the pairwise permutation independence tests: tests/golden/indep.npz.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_indep.py

It imports the reference's `notreks.mi_tests` from /root/reference/src (read-only) and records data
only: inputs, the reference's results and, by wrapping the reference's `hsic_stat` / `dcor_stat`
while `test_pairwise_independence` runs, every permuted statistic.  tests/test_indep_cpu.py
certifies the file against a plain-numpy restatement; tests/test_gpu_indep.py compares
csrc/indep.hip with it.

Cases (name: X shape, num_perm) -- the smallest shapes that cross every boundary of the kernel's
64 x 64 tiling: n below one tile, one tile + 1, several tiles with a tail, and the workload's n:

    c5 5x3 P=24, c97 97x5 P=40, c200 200x4 P=33, c257 257x3 P=17, c1000 1000x3 P=8,
    c96 96x6 P=60 (column 1 = sin(3 x0) + noise, column 2 = 0.9 x0 + noise, column 3 constant)

The pair list of a case holds every i < j, then (1, 0), (1, 1) and (d-1, d-2): both orders and a
diagonal pair.  Stored per case and statistic T in {hsic, dcor}:
    {case}/X, {case}/seed, {case}/pairs, {case}/P,
    {case}/{T}/stat, /pvalue, /ge            (m,)
    {case}/{T}/null                          (m, P) every permuted statistic, in stream order
    {case}/perm_guard                        (m, P) int64: sum_a (a + 1) perm[a] of the numpy stream
c96 also: c96/{T}/I_b{0,1}_u{0,1}, the reference's get_I_from_full_pairwise_tests (alpha 0.05, the
case's P and seed) for bonferroni off/on and undirected off/on.  c97 also: c97/{pearson,spearman}/
stat, /pvalue.

Tie condition: the GPU sums in another order than numpy, so a permuted value within rounding of
the observed one could flip a count.  For every pair without a constant column the generator
asserts min_p |stat_p - stat_obs| / |stat_obs| >= 1e-6 (also over the pair lists of the get_I
runs); a case whose seed fails it moves to the next seed.
"""
import os
import sys

import numpy as np

sys.path.insert(0, "/root/reference/src")
from notreks import mi_tests as ref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
TIE_MIN = 1e-6
CASES = (("c5", 5, 3, 24), ("c97", 97, 5, 40), ("c200", 200, 4, 33), ("c257", 257, 3, 17), ("c1000", 1000, 3, 8),
         ("c96", 96, 6, 60))
STATS = ("hsic", "dcor")


def make_X(name, n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    if name == "c96":
        X[:, 1] = np.sin(3.0 * X[:, 0]) + 0.15 * rng.standard_normal(n)
        X[:, 2] = 0.9 * X[:, 0] + 0.2 * rng.standard_normal(n)
        X[:, 3] = 1.5
    else:
        X[:, 1] += 0.6 * X[:, 0]
    return X


def pair_list(d):
    pairs = [(i, j) for i in range(d) for j in range(i + 1, d)]
    return pairs + [(1, 0), (1, 1), (d - 1, d - 2)]


class Recorder:
    """Wraps the reference's statistic so every value it returns is kept, in call order."""

    def __init__(self, name):
        self.name, self.fn, self.vals = name + "_stat", getattr(ref, name + "_stat"), []

    def __enter__(self):
        setattr(ref, self.name, self)
        return self

    def __exit__(self, *exc):
        setattr(ref, self.name, self.fn)

    def __call__(self, x, y):
        v = self.fn(x, y)
        self.vals.append(float(v))
        return v


def ties_ok(X, pairs, vals):
    """vals: (m, P + 1), column 0 the observed statistic."""
    for (i, j), row in zip(pairs, vals):
        if np.ptp(X[:, i]) == 0 or np.ptp(X[:, j]) == 0:
            assert (row == 0).all()
            continue
        if np.abs(row[1:] - row[0]).min() < TIE_MIN * abs(row[0]):
            return False
    return True


def run_case(name, n, d, P, seed):
    X = make_X(name, n, d, seed)
    pairs = pair_list(d)
    m = len(pairs)
    out = {"X": X, "seed": np.int64(seed), "pairs": np.asarray(pairs, dtype=np.int64), "P": np.int64(P)}
    rng = np.random.default_rng(seed)
    w = np.arange(1, n + 1, dtype=np.int64)
    out["perm_guard"] = np.array([[int((rng.permutation(n).astype(np.int64) * w).sum()) for _ in range(P)]
                                  for _ in range(m)], dtype=np.int64)
    for T in STATS:
        with Recorder(T) as rec:
            res = ref.test_pairwise_independence(X, pairs, test=T, num_perm=P, seed=seed)
        vals = np.asarray(rec.vals).reshape(m, P + 1)
        if not ties_ok(X, pairs, vals):
            return None
        stat = np.array([r.stat for r in res])
        pval = np.array([r.pvalue for r in res])
        ge = (vals[:, 1:] >= vals[:, :1]).sum(axis=1).astype(np.int64)
        assert (stat == vals[:, 0]).all() and (pval == (ge + 1) / (P + 1)).all()
        out[f"{T}/stat"], out[f"{T}/pvalue"], out[f"{T}/ge"], out[f"{T}/null"] = stat, pval, ge, vals[:, 1:]
        if name == "c96":
            for b in (0, 1):
                for u in (0, 1):
                    with Recorder(T) as rec:
                        I = ref.get_I_from_full_pairwise_tests(X, alpha=0.05, test=T, num_perm=P, seed=seed,
                                                               bonferroni=bool(b), undirected=bool(u))
                    ip = ([(i, j) for i in range(d) for j in range(i + 1, d)] if u else
                          [(i, j) for i in range(d) for j in range(d) if i != j])
                    if not ties_ok(X, ip, np.asarray(rec.vals).reshape(len(ip), P + 1)):
                        return None
                    out[f"{T}/I_b{b}_u{u}"] = np.asarray(I, dtype=np.int64).reshape(-1, 2)
    if name == "c97":
        for T in ("pearson", "spearman"):
            res = ref.test_pairwise_independence(X, pairs, test=T)
            out[f"{T}/stat"] = np.array([r.stat for r in res])
            out[f"{T}/pvalue"] = np.array([r.pvalue for r in res])
    return out


def main():
    blob = {}
    for k, (name, n, d, P) in enumerate(CASES):
        for seed in range(100 * (k + 1), 100 * (k + 1) + 50):
            out = run_case(name, n, d, P, seed)
            if out is not None:
                break
            print(f"{name}: seed {seed} fails the tie condition, next seed")
        else:
            raise SystemExit(f"{name}: no seed meets the tie condition")
        print(f"{name}: seed {seed}, {len(out['pairs'])} pairs")
        for key, v in out.items():
            blob[f"{name}/{key}"] = v
    path = os.path.join(HERE, "indep.npz")
    np.savez_compressed(path, **blob)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
