"""Fixtures for the TCC regularizer's blocked-inverse regime, d >= 993: tests/golden/tcc_blocked.npz
(point cases) and tcc_blocked_traj.npz (trajectories; two files because together they pass 1 MiB).
tests/test_trek_oracle.py certifies the point cases on the CPU, tests/test_gpu_tcc.py compares
csrc/tcc.hip with both.

One oracle evaluation at d = 1000 is two 2000 x 2000 `numpy.linalg.eig` calls (some 14 s), too slow
to run inside a GPU test, so the Perron triples and the oracle's trajectories are recorded here.
The inputs are not stored: the tests regenerate them with the builders below and check the guards.

Point cases, d in POINT_D, case 'dense': W and pairs of `test_tcc_value_grad_matches_oracle_larger`
(np.random.default_rng(d)).  Stored: (rho, u, v) of `oracle.trek_oracle.tcc_perron`, the guards
W.sum(), W[1, :8], len(pairs), and spread_value / spread_grad: the relative difference of value and
gradient (max-norm) between that triple and an independent Perron solve of the same A (LU-based
inverse iteration at a Collatz-Wielandt upper bound of rho, `perron_shift_invert`).

Case 'dag' (W o W nilpotent, the reducible regime trek_tcc.npz calls `dag`; here a weighted DAG of
density 0.2 in a random variable order, weights scaled by 1 / sqrt(0.2 d)) is written only for a d at
which its spread is <= 1e-11 AND both eig vectors are strictly positive, which the CPU test's
certificate needs.  It is left out at d = 1088: A is reducible there, one entry of eig's v is exactly
0 (spread 1.4e-16 / 8.2e-14), and a vector with a zero entry certifies nothing.  It is in at the
five other sizes.

Trajectory cases, d in TRAJ_D: data and pairs of tests/test_gpu_tcc.py::_tcc_case(d), a start
W0 != 0 (`traj_w0`: 'dense' is the point case's W; 'plain400' the oracle's own W after 400 steps
without TCC), then `o.minimize(W0, 1.0, K, 1.0, 3e-4, tol=-1.0)` with TCC in 'opt' mode, K = 24.
The oracle must take all K steps (no halving, no stop).  Stored: W_K at N_POS seeded positions,
its row and column sums, the iteration count, the guards cov.sum(), cov[0, :8], W0.sum().

    python tests/golden/make_tcc_blocked.py                       # every case in worker processes, merged
    python tests/golden/make_tcc_blocked.py --d 1088 --kind traj --w0 dense --out part.npz   # one worker
    python tests/golden/make_tcc_blocked.py --merge a.npz b.npz   # parts -> the two fixture files
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
HERE = os.path.join(REPO, "tests", "golden")

POINT_D = (993, 1000, 1024, 1040, 1088, 1152)
TRAJ_D = (1000, 1088, 1152)
TRAJ_W0 = {1000: "dense", 1088: "dense", 1152: "dense"}   # which start the stored trajectory uses
K_TRAJ = 24
N_POS = 32768
SPREAD_MAX = 1e-11


# --- seeded inputs (shared with the tests) ---------------------------------------------------

def point_inputs(d, case="dense"):
    """(W, pairs) of a point case."""
    rng = np.random.default_rng(d)
    W = rng.uniform(-1, 1, (d, d)) * (0.6 / np.sqrt(d))
    np.fill_diagonal(W, 0)
    iu = np.array(np.triu_indices(d, 1)).T
    pairs = iu[rng.uniform(size=len(iu)) < 0.1]
    if case == "dag":   # a weighted DAG in a random variable order, in-degree-normalised weights
        B = np.tril(rng.uniform(size=(d, d)) < 0.2, -1)
        W = B * rng.uniform(0.5, 1.5, (d, d)) * rng.choice([-1.0, 1.0], (d, d)) / np.sqrt(0.2 * d)
        p = rng.permutation(d)
        W = np.ascontiguousarray(W[np.ix_(p, p)])
    return W, pairs


def traj_case(d, seed=7):
    """tests/test_gpu_tcc.py::_tcc_case: (oracle with TCC in 'opt' mode, pairs)."""
    from midagma_amd.simulate import make_dataset
    from oracle.dagma_oracle import LinearOracle
    X, _, _ = make_dataset(d, 2 * d, seed=seed)
    rng = np.random.default_rng(seed)
    iu = np.array(np.triu_indices(d, 1)).T
    pairs = iu[rng.uniform(size=len(iu)) < 0.3]
    o = LinearOracle("l2")
    o.prepare(X.copy(), 0.03, 1000)
    o.trek = dict(kind="tcc", pairs=pairs, mode="opt", weight=0.2)
    return o, pairs


def traj_w0(d, kind, o=None):
    """The trajectory's start: 'dense' (seeded by d), or 'plain400' (400 oracle steps without TCC)."""
    if kind == "dense":
        return point_inputs(d)[0]
    assert kind == "plain400", kind
    trek, o.trek = o.trek, None
    try:
        W0, tr = o.minimize(np.zeros((d, d)), 1.0, 400, 1.0, 3e-4, tol=-1.0)
    finally:
        o.trek = trek
    assert tr.iters == 400
    return W0


def traj_positions(d):
    """Flat indices into W_K at which the fixture keeps its entries."""
    return np.random.default_rng(100000 + d).integers(0, d * d, N_POS)


# --- the second, independent Perron solve ----------------------------------------------------

def perron_shift_invert(A, iters=200):
    """(rho, u, v) of a non-negative A without an eigendecomposition: power steps from the ones
    vector give a Collatz-Wielandt upper bound sigma >= rho (max_i (A x)_i / x_i over x_i > 0), then
    inverse iteration with one LU of sigma I - A for the right and (transposed) the left vector."""
    import scipy.linalg as spla
    n = A.shape[0]
    x = np.ones(n)
    for _ in range(60):
        x = A @ x
        x /= np.linalg.norm(x)
    pos = x > 0
    sigma = float(((A @ x)[pos] / x[pos]).max())
    lu = spla.lu_factor(sigma * np.eye(n) - A)
    out = []
    for trans in (0, 1):
        y = x.copy() if trans == 0 else np.ones(n) / np.sqrt(n)
        for _ in range(iters):
            z = spla.lu_solve(lu, y, trans=trans)
            z /= np.linalg.norm(z)
            done = np.abs(z - y).max() <= 1e-16
            y = z
            if done:
                break
        out.append(y if y.sum() >= 0 else -y)
    v, u = out
    rho = float(u @ (A @ v) / (u @ v))
    return rho, u, v


def gen_point(d, case):
    from oracle.trek_oracle import _tcc_matrices, tcc_from_perron, tcc_perron
    W, pairs = point_inputs(d, case)
    t0 = time.time()
    rho, u, v = tcc_perron(W, pairs, 1.0)
    t1 = time.time()
    A, _ = _tcc_matrices(W, np.asarray(pairs, dtype=np.int64), 1.0)
    rho2, u2, v2 = perron_shift_invert(A)
    val, g = tcc_from_perron(W, pairs, rho, u, v)
    val2, g2 = tcc_from_perron(W, pairs, rho2, u2, v2)
    sv = abs(val - val2) / abs(val)
    sg = float(np.abs(g - g2).max() / np.abs(g).max())
    res_v = np.abs(A @ v - rho * v).max() / rho
    res_u = np.abs(A.T @ u - rho * u).max() / rho
    print(f"point d={d} {case}: rho={rho:.12g} value={val:.6e} spread_value={sv:.2e} spread_grad={sg:.2e} "
          f"min u={u.min():.2e} min v={v.min():.2e} resid v={res_v:.1e} u={res_u:.1e} "
          f"eig {t1 - t0:.0f} s, second solve {time.time() - t1:.0f} s", flush=True)
    if case != "dense" and not (sv <= SPREAD_MAX and sg <= SPREAD_MAX and u.min() > 0 and v.min() > 0):
        print(f"point d={d} {case}: left out", flush=True)
        return {}
    k = f"{case}_d{d}"
    return {f"rho_{k}": np.array(rho), f"u_{k}": u, f"v_{k}": v, f"spread_value_{k}": np.array(sv),
            f"spread_grad_{k}": np.array(sg), f"guard_Wsum_{k}": np.array(W.sum()), f"guard_Wrow1_{k}": W[1, :8].copy(),
            f"guard_npairs_{k}": np.array(len(pairs))}


def gen_traj(d, kind):
    o, pairs = traj_case(d)
    W0 = traj_w0(d, kind, o)
    g_w0 = W0.sum()
    t0 = time.time()
    WK, tr = o.minimize(W0.copy(), 1.0, K_TRAJ, 1.0, 3e-4, tol=-1.0)
    print(f"traj d={d} {kind}: iters={tr.iters} halvings={tr.halvings} success={tr.success} "
          f"max|W_K - W0|={np.abs(WK - W0).max():.3e} {time.time() - t0:.0f} s", flush=True)
    if not (tr.iters == K_TRAJ and tr.success and tr.halvings == 0 and not tr.early_stop):
        raise SystemExit(f"traj d={d} {kind}: the oracle did not take {K_TRAJ} plain steps; change the seed")
    k = f"traj_d{d}"
    return {f"W_{k}": WK.ravel()[traj_positions(d)], f"rowsum_{k}": WK.sum(axis=1), f"colsum_{k}": WK.sum(axis=0),
            f"iters_{k}": np.array(tr.iters), f"w0_{k}": np.array(kind), f"guard_covsum_{k}": np.array(o.cov.sum()),
            f"guard_covrow0_{k}": o.cov[0, :8].copy(), f"guard_W0sum_{k}": np.array(g_w0)}


def merge(parts):
    """Workers' parts -> tcc_blocked.npz (point cases) and tcc_blocked_traj.npz (trajectories)."""
    point, traj = {}, {}
    for p in parts:
        with np.load(p) as f:
            for k in f.files:
                (traj if k.endswith(tuple(f"_traj_d{d}" for d in TRAJ_D)) else point)[k] = f[k]
    for name, out in (("tcc_blocked.npz", point), ("tcc_blocked_traj.npz", traj)):
        if out:
            path = os.path.join(HERE, name)
            np.savez_compressed(path, **out)
            print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=None, help="one size (a worker); default: all, then merge")
    ap.add_argument("--kind", choices=("point", "traj"), default="point")
    ap.add_argument("--w0", choices=("dense", "plain400"), default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs="+", default=None)
    a = ap.parse_args()
    if a.merge:
        merge(a.merge)
        return
    if a.d is not None:
        from threadpoolctl import threadpool_limits
        with threadpool_limits(limits=int(os.environ.get("TCC_BLOCKED_THREADS", "2"))):
            if a.kind == "point":
                out = {**gen_point(a.d, "dense"), **gen_point(a.d, "dag")}
            else:
                out = gen_traj(a.d, a.w0 or TRAJ_W0[a.d])
        np.savez(a.out, **out)
        return
    import tempfile
    tmp = tempfile.mkdtemp(prefix="tcc_blocked_")
    jobs = [("point", d) for d in POINT_D] + [("traj", d) for d in TRAJ_D]
    procs = [(f"{tmp}/{k}_{d}.npz", subprocess.Popen([sys.executable, __file__, "--d", str(d), "--kind", k,
                                                       "--out", f"{tmp}/{k}_{d}.npz"])) for k, d in jobs]
    for _, p in procs:
        if p.wait() != 0:
            raise SystemExit("worker failed")
    merge([f for f, _ in procs])


if __name__ == "__main__":
    main()
