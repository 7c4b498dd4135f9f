"""Bit-for-bit A/B of the single-fit solver handle (csrc/solver_impl.h and its parts; diagnostic).

Two library paths, every case in a fresh child process per library, every returned array saved,
np.array_equal demanded between the two sides:

    python tools/ab_solver.py --a /path/to/old.so --b midagma_amd/libmidagma_hip.so \
        --out profiles/solver_split_ab.json

The cases are the smallest shapes that reach each branch of enqueue_part1 / enqueue_part2 and each
set-up of the handle (60 to 150 steps from W = 0, checkpoint 40):
  cov l2   d = 20 (one-workgroup loop), d = 50 with float32 W (flat Gauss-Jordan on graph slots),
           d = 100 (D = 128, one 128 block, fast slots, no split-K), d = 300 (D = 512, B2 = 256,
           split-K 4: score GEMM fused into the trailing launch, control folded), d = 1100
           (D = 1152, inside the at_fold rule)
  masks    include-edge and exclude-edge masks at d = 100
  pst      exp and inv at d = 40 (graph slots)
  tcc      d = 20 (one-workgroup loop), d = 70 (2d > 128: the fixed stage on fast slots; the
           hand-back count is recorded and compared, not required to be zero)
  data     l2 d = 50 n = 500 (D = 64, flat inverse forked); l2 d = 200 n = 1000 (blocked, small
           shard); l2 d = 200 n = 17000 (n_pad > 16384: pivoted blocked inverse forked); logistic
           d = 200 n = 1000; l2 d = 256 n = 2048 with debug_xty_form(2) (Strassen X^T Y)
  group    HipGroup, emulate=True, two members on one device, d = 200, n = 1000
Recorded per case: W, the result's counters and final values, the hand-back count, every
checkpoint field except `elapsed`, and h_value / score / trek_value (with gradients) of the final W.

`--host-time` adds, per library and alternating, the host wall time of create + set_cov / set_data
+ a first 8-step minimize (the graph captures) at d = 1000 in cov and data mode (n = 10000): two
fresh processes per library, three handles each after a warm-up handle, and the median per side.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _REPO)
import numpy as np  # noqa: E402

CKPT = 40


def _x(d, n, seed, logistic=False):
    from midagma_amd.simulate import make_dataset
    X, _, _ = make_dataset(d, n, seed=seed, **({"sem_type": "logistic"} if logistic else {}))
    return X if logistic else X - X.mean(0)


def _cov(d, seed, n=400):
    X = _x(d, n, seed)
    return X.T @ X / n


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


def _record(out, W, r, handbacks):
    out["W"] = W.copy()
    out["res"] = np.array([r.iters, r.status, r.halvings, int(r.early_stop), r.slots, handbacks], dtype=np.int64)
    out["fin"] = np.array([r.lr_final, r.obj_last, r.score_last, r.h_last])
    fields = [f for f in type(r.checkpoints[0])._fields if f != "elapsed"] if r.checkpoints else []
    out["ckpt"] = np.array([[float(getattr(c, f)) for f in fields] for c in r.checkpoints])


def _cov_case(d, steps, *, w32=False, masks=None, pst=None, tcc=False):
    def run(out):
        from midagma_amd.solver import HipSolver
        s = HipSolver(d, "l2", "cov")
        s.set_cov(_cov(d, d))
        if w32:
            s.set_w_float32(True)
        if masks == "inc":
            s.set_masks(_masks(d, d)[0], None)
        if masks == "exc":
            s.set_masks(None, _masks(d, d)[1])
        if pst:
            s.set_trek(_pairs(d, d), pst, agg="mean", mode="opt", weight=0.1)
        if tcc:
            s.set_trek_tcc(_pairs(d, d), mode="opt", weight=0.1)
        W = np.zeros((d, d))
        r = s.minimize(W, 1.0, steps, 1.0, 3e-4, tol=-1.0, lambda1=0.03, checkpoint=CKPT, want_checkpoints=True)
        _record(out, W, r, s.debug_handbacks())
        out["h"], out["h_grad"] = s.h_value(W, 1.0)
        out["score"], out["score_grad"] = s.score_value(W)
        if pst or tcc:
            out["trek"], out["trek_grad"] = s.trek_value(W)
        s.close()
    return run


def _data_case(d, n, steps, loss="l2", xty=None):
    def run(out):
        from midagma_amd.solver import HipSolver
        X = _x(d, n, d + n, logistic=loss == "logistic")
        s = HipSolver(d, loss, "data")
        if xty:
            s.debug_xty_form(xty)
        if loss == "logistic":
            s.set_cov(X.T @ X / float(n))
        s.set_data(X, n_global=n)
        out["xty_form"] = np.array([s.xty_form])
        W = np.zeros((d, d))
        r = s.minimize(W, 1.0, steps, 1.0, 3e-4, tol=-1.0, lambda1=0.03, checkpoint=CKPT, want_checkpoints=True)
        _record(out, W, r, s.debug_handbacks())
        out["h"], out["h_grad"] = s.h_value(W, 1.0)
        s.score_partial(W)
        out["score"], out["score_grad"] = s.score_finish()
        s.close()
    return run


def _group_case(d, n, steps):
    def run(out):
        from midagma_amd.solver import HipGroup
        g = HipGroup(d, "l2", devices=[0, 0], emulate=True)
        g.set_data(_x(d, n, d + n))
        W = np.zeros((d, d))
        r = g.minimize(W, 1.0, steps, 1.0, 3e-4, tol=-1.0, lambda1=0.03, checkpoint=CKPT, want_checkpoints=True)
        _record(out, W, r, g.members[0].debug_handbacks())
        out["h"], out["h_grad"] = g.h_value(W, 1.0)
        out["score"], out["score_grad"] = g.score(W)
        g.close()
    return run


CASES = {
    "cov/d20": _cov_case(20, 150),
    "cov/d50_w32": _cov_case(50, 150, w32=True),
    "cov/d100": _cov_case(100, 150),
    "cov/d300": _cov_case(300, 120),
    "cov/d1100": _cov_case(1100, 90),
    "masks/inc_d100": _cov_case(100, 150, masks="inc"),
    "masks/exc_d100": _cov_case(100, 150, masks="exc"),
    "pst/exp_d40": _cov_case(40, 120, pst="exp"),
    "pst/inv_d40": _cov_case(40, 120, pst="inv"),
    "tcc/d20": _cov_case(20, 150, tcc=True),
    "tcc/d70": _cov_case(70, 120, tcc=True),
    "data/l2_d50_n500": _data_case(50, 500, 150),
    "data/l2_d200_n1000": _data_case(200, 1000, 120),
    "data/l2_d200_n17000": _data_case(200, 17000, 60),
    "data/logistic_d200_n1000": _data_case(200, 1000, 120, loss="logistic"),
    "data/l2_d256_n2048_strassen": _data_case(256, 2048, 90, xty=2),
    "group/emulated2_d200_n1000": _group_case(200, 1000, 120),
}


def _host_time(kind):
    """Seconds on the host from create to the end of a first 8-step minimize at d = 1000."""
    from midagma_amd.solver import HipSolver
    d, n = 1000, 10000
    X = np.random.default_rng(0).standard_normal((n, d))
    cov = X.T @ X / n
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s = HipSolver(d, "l2", kind)
    if kind == "cov":
        s.set_cov(cov)
    else:
        s.set_data(X, n_global=n)
    W = np.zeros((d, d))
    s.minimize(W, 1.0, 8, 1.0, 3e-4, tol=-1.0, lambda1=0.03, checkpoint=CKPT)
    dt = time.perf_counter() - t0
    s.close()
    return dt


def child(case, npz):
    import torch  # noqa: F401  (owns the HIP runtime)
    from midagma_amd import _lib
    _lib.load()
    if case.startswith("host/"):
        _host_time(case[5:])  # (the process's first handle also pays the runtime's start-up)
        np.savez(npz, seconds=np.array([_host_time(case[5:]) for _ in range(3)]))
        return 0
    out = {}
    CASES[case](out)
    np.savez(npz, **{k: np.asarray(v) for k, v in out.items()})
    return 0


def _run_child(lib, case, npz):
    env = dict(os.environ, MIDAGMA_LIB=os.path.abspath(lib))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--npz", npz], env=env,
                       capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f"{case} on {lib}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    return dict(np.load(npz))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", help="the reference library (the parent commit's build)")
    ap.add_argument("--b", help="the library under test")
    ap.add_argument("--out", help="JSON summary")
    ap.add_argument("--only", nargs="*", help="case names (default: all)")
    ap.add_argument("--host-time", action="store_true")
    ap.add_argument("--case", help=argparse.SUPPRESS)  # the child process
    ap.add_argument("--npz", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.case:
        return child(a.case, a.npz)
    if not (a.a and a.b):
        ap.error("--a and --b")
    report = {"a": os.path.basename(a.a), "b": os.path.basename(a.b), "cases": {}, "equal": True}
    tmp = tempfile.mkdtemp(prefix="ab_solver_")
    for name in (a.only or list(CASES)):
        # a failing child ends the run: nothing more starts on the device after a fault
        ra = _run_child(a.a, name, os.path.join(tmp, "a.npz"))
        rb = _run_child(a.b, name, os.path.join(tmp, "b.npz"))
        keys = sorted(set(ra) | set(rb))
        bad = [k for k in keys if k not in ra or k not in rb or ra[k].shape != rb[k].shape or
               not np.array_equal(ra[k], rb[k], equal_nan=True)]
        res = ra["res"]
        report["cases"][name] = {"arrays": len(keys), "equal": not bad, "differ": bad, "iters": int(res[0]),
                                 "slots": int(res[4]), "handbacks_a": int(res[5]), "handbacks_b": int(rb["res"][5]),
                                 "checkpoints": int(ra["ckpt"].shape[0])}
        report["equal"] = report["equal"] and not bad
        print(f"{name}: {len(keys)} arrays, iters {int(res[0])}, slots {int(res[4])}, hand-backs {int(res[5])}: "
              f"{'equal' if not bad else 'DIFFER ' + ' '.join(bad)}", flush=True)
    if a.host_time:
        ht = {}
        for kind in ("cov", "data"):
            runs = {"a": [], "b": []}
            for _ in range(2):  # a b a b
                for side, lib in (("a", a.a), ("b", a.b)):
                    runs[side].append(_run_child(lib, f"host/{kind}", os.path.join(tmp, "h.npz"))["seconds"].tolist())
            for side in ("a", "b"):
                flat = sorted(x for r in runs[side] for x in r)
                runs[side + "_median"] = flat[len(flat) // 2]
            ht[kind] = runs
            print(f"host create + set-up + first minimize, d = 1000 {kind}: a {runs['a']}  b {runs['b']}", flush=True)
        report["host_seconds_d1000"] = ht
    n_arr = sum(c["arrays"] for c in report["cases"].values())
    print(f"{len(report['cases'])} cases, {n_arr} arrays: {'all equal' if report['equal'] else 'DIFFERENCES'}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
    return 0 if report["equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
