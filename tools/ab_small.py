"""Bit-for-bit A/B of the one-workgroup small-d path (csrc/small.hip, small_eval.hip; diagnostic).

Runs a fixed list of small cases on the library MIDAGMA_LIB names (default: the product build) and
writes every result array to an .npz; `--compare` demands np.array_equal on every array of two such
files.  One run per library, each in a fresh process:

    MIDAGMA_LIB=/path/to/old.so python tools/ab_small.py --out a.npz
    python tools/ab_small.py --out b.npz
    python tools/ab_small.py --compare a.npz b.npz

The cases hit every instantiation of the slot kernel and every branch of the layer under it
(csrc/wgtile.h), on data from make_dataset(d, 200, seed):
  plain    HipSolver, float64, d in {5, 16, 17, 20, 32, 33, 48, 64}: 300 steps from W = 0 with
           checkpoint = 50 (Gauss-Jordan and product-form slots alternate); at one d per block edge
           with both masks, and with lr = 0.3, where the run halves (asserted; 60 steps with
           checkpoint = 10, so that the halvings fall between checkpoint slots and on them)
  w32      float32 W, d in {5, 20}
  tcc      d = 16, 20 (the 5 x 5 body), 32, modes opt and log
  pst      HipBatch, B = 3, d in {10, 20}, seq {exp, inv} x agg {mean, lse}, modes opt and log;
           trek_value with and without the gradient on the same handles
  logit    HipBatch, B = 3, d in {10, 20, 40}, binary X, n = 10 (one row block) and n = 70 (3 to 5
           blocks, a ragged last one), per-problem and shared X; score_logistic with and without G
Recorded per fit: W, iterations, status, halvings and every checkpoint field except `elapsed`.
`--compare` calls np.array_equal with equal_nan=True: a NaN both libraries write in the same place
(a diverged run's record) counts as equal; any other difference, a NaN on one side included, fails.
"""
import argparse
import os
import sys

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _REPO)
import numpy as np  # noqa: E402

from tests.blockinv_cases import SMALL_DS as _SMALL_DS  # noqa: E402  (small_block(d) -> the d of the slot tests)

SMALL_DS = tuple(sorted(d for ds in _SMALL_DS.values() for d in ds))  # 5, 16, 17, 20, 32, 33, 48, 64
EDGE_DS = (16, 20, 64)                      # one d per block edge (16, 32, 64)
N = 200


def _cov(d, seed):
    from midagma_amd.simulate import make_dataset
    X, _, _ = make_dataset(d, N, seed=seed)
    X = X - X.mean(0)
    return X.T @ X / X.shape[0]


def _pairs(d, seed, frac=0.3):
    iu = np.array(np.triu_indices(d, 1)).T
    return iu[np.random.default_rng(seed).uniform(size=len(iu)) < frac]


def _masks(d, seed):
    rng = np.random.default_rng(seed)
    inc = np.where(rng.uniform(size=(d, d)) < 0.1, 0.05, 0.0)
    exc = (rng.uniform(size=(d, d)) >= 0.1).astype(np.float64)
    np.fill_diagonal(inc, 0.0)
    np.fill_diagonal(exc, 0.0)
    return inc, exc


def _record(out, key, W, results):
    """W and, per problem, the result's counters and its checkpoint records without `elapsed`."""
    out[f"{key}/W"] = W.copy()
    for b, r in enumerate(results):
        out[f"{key}/res{b}"] = np.array([r.iters, r.status, r.halvings, int(r.early_stop), r.slots], dtype=np.int64)
        out[f"{key}/fin{b}"] = np.array([r.lr_final, r.obj_last, r.score_last, r.h_last])
        fields = [f for f in type(r.checkpoints[0])._fields if f != "elapsed"] if r.checkpoints else []
        out[f"{key}/ckpt{b}"] = np.array([[float(getattr(c, f)) for f in fields] for c in r.checkpoints])


def run_cases():
    import torch  # noqa: F401  (owns the HIP runtime)
    from midagma_amd import _lib
    from midagma_amd.simulate import make_dataset
    from midagma_amd.solver import HipBatch, HipSolver
    _lib.load()
    out = {}

    def single(key, d, *, lr=3e-4, steps=300, ckpt=50, masks=None, w32=False, tcc=None, lam=0.03):
        s = HipSolver(d, "l2", "cov")
        try:
            s.set_cov(_cov(d, d))
            if masks:
                s.set_masks(*masks)
            if w32:
                s.set_w_float32(True)
            if tcc:
                s.set_trek_tcc(_pairs(d, d), mode=tcc, weight=0.1)
            W = np.zeros((d, d))
            r = s.minimize(W, 1.0, steps, 1.0, lr, tol=-1.0, lambda1=lam, checkpoint=ckpt, want_checkpoints=True)
            _record(out, key, W, [r])
            return r
        finally:
            s.close()

    for d in SMALL_DS:
        single(f"plain/d{d}", d)
    for d in EDGE_DS:
        single(f"masks/d{d}", d, masks=_masks(d, d))
        r = single(f"halve/d{d}", d, lr=0.3, steps=60, ckpt=10)
        assert r.halvings >= 1, f"halve/d{d}: lr = 0.3 did not halve ({r})"
    for d in (5, 20):
        single(f"w32/d{d}", d, w32=True)
    for d in (16, 20, 32):
        for mode in ("opt", "log"):
            single(f"tcc/{mode}/d{d}", d, tcc=mode)

    B = 3
    for d in (10, 20):
        covs = np.stack([_cov(d, 100 + b) for b in range(B)])
        Wp = np.stack([0.3 * np.random.default_rng(7 + b).standard_normal((d, d)) for b in range(B)])
        for seq in ("exp", "inv"):
            for agg in ("mean", "lse"):
                for mode in ("opt", "log"):
                    key = f"pst/{seq}/{agg}/{mode}/d{d}"
                    bt = HipBatch(d, B)
                    try:
                        bt.set_cov(covs)
                        bt.set_trek(_pairs(d, d), seq, agg=agg, mode=mode, weight=[0.05, 0.1, 0.2])
                        W = np.zeros((B, d, d))
                        res = bt.minimize(W, 1.0, 1.0, 3e-4, 0.03, 300, tol=-1.0, checkpoint=50,
                                          want_checkpoints=True)
                        _record(out, key, W, res)
                        v, G = bt.trek_value(Wp, grad=True)
                        v0, _ = bt.trek_value(Wp, grad=False)
                        out[f"{key}/value"], out[f"{key}/grad"], out[f"{key}/value_nograd"] = v, G, v0
                    finally:
                        bt.close()

    for d in (10, 20, 40):
        for n in (10, 70):
            Xs = np.stack([make_dataset(d, n, seed=200 + b, sem_type="logistic")[0] for b in range(B)])
            Wp = np.stack([0.3 * np.random.default_rng(9 + b).standard_normal((d, d)) for b in range(B)])
            for shared in (False, True):
                key = f"logit/d{d}/n{n}/{'shared' if shared else 'own'}"
                Xb = np.stack([Xs[0]] * B) if shared else Xs
                bt = HipBatch(d, B)
                try:
                    bt.set_cov(np.stack([X.T @ X / float(n) for X in Xb]))
                    bt.set_data(Xs[0] if shared else Xs, shared=shared)
                    W = np.zeros((B, d, d))
                    res = bt.minimize_logistic(W, 1.0, 1.0, 3e-4, [0.01, 0.03, 0.05], 300, tol=-1.0, checkpoint=50,
                                               want_checkpoints=True)
                    _record(out, key, W, res)
                    loss, G = bt.score_logistic(Wp, grad=True)
                    loss0, _ = bt.score_logistic(Wp, grad=False)
                    out[f"{key}/loss"], out[f"{key}/G"], out[f"{key}/loss_nograd"] = loss, G, loss0
                finally:
                    bt.close()
    return out


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    keys = sorted(set(a.files) | set(b.files))
    bad = [k for k in keys if k not in a.files or k not in b.files or a[k].shape != b[k].shape or
           not np.array_equal(a[k], b[k], equal_nan=True)]
    cases = sorted({k.rsplit("/", 1)[0] for k in keys})
    for k in bad:
        if k in a.files and k in b.files and a[k].shape == b[k].shape and a[k].size:
            print(f"DIFFERS {k}: max|a - b| = {np.nanmax(np.abs(a[k] - b[k])):.3e}")
        else:
            print(f"DIFFERS {k}: missing or another shape")
    print(f"{len(cases)} cases, {len(keys)} arrays: {'all equal' if not bad else f'{len(bad)} arrays differ'}")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="run the cases, write their arrays here (.npz)")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    if not a.out:
        ap.error("--out or --compare")
    out = run_cases()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez(a.out, **out)
    print(f"{os.path.basename(os.environ.get('MIDAGMA_LIB', 'libmidagma_hip.so'))}: "
          f"{len({k.rsplit('/', 1)[0] for k in out})} cases, {len(out)} arrays -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
