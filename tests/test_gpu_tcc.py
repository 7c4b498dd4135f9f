"""TCC trek regularizer on the GPU (csrc/tcc.hip: Noda iteration on the Gauss-Jordan M-matrix
inverse) vs the reference's trek_value_grad / minimize (tests/golden/trek_tcc.npz) and the
oracle (oracle/trek_oracle.py::tcc_value_grad, numpy eig as the reference).

Tolerances: the Perron pair comes from a different (iterative) algorithm than LAPACK's
eigendecomposition, so value and gradient agree to the eigenvector conditioning, not bit for
bit: 1e-10 relative; W after the loop 1e-9 (the north star asks 1e-5)."""
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle.dagma_oracle import LinearOracle  # noqa: E402
from oracle.trek_oracle import tcc_value_grad  # noqa: E402


def _solver(d, cov):
    from midagma_amd.solver import HipSolver
    s = HipSolver(d, "l2", "cov", device=0)
    s.set_cov(cov)
    return s


@pytest.mark.parametrize("d", [8, 20])
@pytest.mark.parametrize("case", ["dense", "tiny", "dag"])
@pytest.mark.parametrize("w", [1.0, 2.0])
def test_tcc_value_grad_matches_reference(golden, d, case, w):
    f = golden("trek_tcc.npz")
    W, pairs = f[f"W_{case}_d{d}"], f[f"pairs_d{d}"]
    s = _solver(d, np.eye(d))
    s.set_trek_tcc(pairs, mode="opt", weight=0.5, w=w)
    v, g = s.trek_value(W)
    v_ref, g_ref = float(f[f"val_{case}_w{w:g}_d{d}"]), f[f"grad_{case}_w{w:g}_d{d}"]
    assert abs(v - v_ref) <= 1e-10 * abs(v_ref)
    assert np.abs(g - g_ref).max() <= 1e-10 * np.abs(g_ref).max()
    # again from the warm start the first call left: same answer
    v2, g2 = s.trek_value(W)
    assert abs(v2 - v_ref) <= 1e-10 * abs(v_ref)
    assert np.abs(g2 - g_ref).max() <= 1e-10 * np.abs(g_ref).max()
    s.close()


@pytest.mark.parametrize("d", [64, 300])
def test_tcc_value_grad_matches_oracle_larger(d):
    rng = np.random.default_rng(d)
    W = rng.uniform(-1, 1, (d, d)) * (0.6 / np.sqrt(d))
    np.fill_diagonal(W, 0)
    iu = np.array(np.triu_indices(d, 1)).T
    pairs = iu[rng.uniform(size=len(iu)) < 0.1]
    s = _solver(d, np.eye(d))
    s.set_trek_tcc(pairs, mode="opt", weight=1.0)
    v, g = s.trek_value(W)
    vr, gr = tcc_value_grad(W, pairs)
    assert abs(v - vr) <= 1e-10 * abs(vr)
    assert np.abs(g - gr).max() <= 1e-10 * np.abs(gr).max()
    s.close()


def test_tcc_at_zero_and_log_mode(golden):
    """W = 0 (a fit's start): A is nilpotent (no Perron gap) -- the gradient 2 W o G is exactly 0
    and the value finite; 'log' mode returns a zero gradient as the reference does."""
    f = golden("trek_tcc.npz")
    pairs = f["pairs_d20"]
    s = _solver(20, np.eye(20))
    s.set_trek_tcc(pairs, mode="opt", weight=0.5)
    v, g = s.trek_value(np.zeros((20, 20)))
    assert np.isfinite(v) and not g.any()
    s.set_trek_tcc(pairs, mode="log", weight=0.5)
    W = f["W_dense_d20"]
    v, g = s.trek_value(W)
    assert abs(v - float(f["val_dense_w1_d20"])) <= 1e-10 * abs(v) and not g.any()
    s.set_trek_tcc(np.zeros((0, 2), dtype=np.int64), mode="opt", weight=0.5)
    v, g = s.trek_value(W)
    assert v == 0.0 and not g.any()
    s.close()


@pytest.mark.parametrize("mode", ["opt", "log"])
@pytest.mark.parametrize("K", [1, 10, 90])
def test_minimize_with_tcc_matches_reference(golden, mode, K):
    f = golden("trek_tcc.npz")
    X = golden("data_d20_n1000_seed0.npz")["X"]
    o = LinearOracle("l2")
    o.prepare(X.copy(), 0.03, 40)
    s = _solver(20, o.cov)
    s.set_trek_tcc(f["pairs_d20"], mode=mode, weight=0.2)
    W = np.zeros((20, 20))
    res = s.minimize(W, 1.0, K, 1.0, 3e-4, tol=-1.0, lambda1=0.03, checkpoint=40)
    assert res.iters == int(f[f"traj_{mode}_it_K{K}"])
    assert np.abs(W - f[f"traj_{mode}_W_K{K}"]).max() <= 1e-9
    s.close()


@pytest.mark.parametrize("d,mode", [(20, "opt"), (20, "log"), (300, "opt")])
def test_minimize_with_tcc_checkpoints_match_oracle(golden, d, mode):
    """Checkpoint records with TCC: objective (+ weight * value in 'opt'), reg_trek_value,
    grad_trek_norm.  d=300 runs the blocked fast path with the 600 x 600 Perron problem."""
    from midagma_amd.simulate import make_dataset
    X, _, _ = make_dataset(d, 1000 if d == 20 else 600, seed=5)
    rng = np.random.default_rng(5)
    iu = np.array(np.triu_indices(d, 1)).T
    pairs = iu[rng.uniform(size=len(iu)) < 0.3]
    o = LinearOracle("l2")
    o.prepare(X.copy(), 0.03, 40)
    o.trek = dict(kind="tcc", pairs=pairs, mode=mode, weight=0.2)
    K = 90 if d == 20 else 45
    s = _solver(d, o.cov)
    s.set_trek_tcc(pairs, mode=mode, weight=0.2)
    W = np.zeros((d, d))
    res = s.minimize(W, 1.0, K, 1.0, 3e-4, tol=-1.0, lambda1=0.03, checkpoint=40, want_checkpoints=True)
    Wr, tr = o.minimize(np.zeros((d, d)), 1.0, K, 1.0, 3e-4, tol=-1.0)
    assert res.iters == tr.iters == K
    assert np.abs(W - Wr).max() <= 1e-9
    assert [c.iter for c in res.checkpoints] == [r["iter"] for r in tr.records]
    for c, r in zip(res.checkpoints, tr.records):
        assert abs(c.obj - r["obj_total"]) <= 1e-10 * abs(r["obj_total"])
        assert abs(c.reg_trek_value - r["reg_trek_value"]) <= 1e-9 * abs(r["reg_trek_value"])
        assert abs(c.grad_trek_norm - r["grad_trek_norm"]) <= 1e-9 * r["grad_trek_norm"] + 1e-15
    s.close()


def test_dagma_linear_tcc_fit_runs(golden):
    from midagma_amd import DagmaLinear
    f = golden("trek_tcc.npz")
    X = golden("data_d20_n1000_seed0.npz")["X"]
    pairs = f["pairs_d20"]
    reg = SimpleNamespace(name="tcc", mode="opt", weight=0.1, cycle_penalty="logdet",
                          cfg={"I": pairs, "version": "exact_trek_graph", "w": 1.0, "n_iter": 10, "eps": 1e-12,
                               "s": 1.0}, enabled=lambda: True)
    m = DagmaLinear("l2", trek_reg=reg)
    W = m.fit(X, lambda1=0.03, T=2, warm_iter=200, max_iter=300)
    assert W.shape == (20, 20) and np.isfinite(W).all()
    Wd = f["W_dense_d20"]
    obj, sc, h, tv = m._func(Wd, 0.1, 1.0)
    v_ref, _ = tcc_value_grad(Wd, pairs)   # the loop ignores cycle_penalty / version (notreks.py:691)
    assert abs(tv - v_ref) <= 1e-10 * abs(v_ref)


def _tcc_case(d, seed=7):
    from midagma_amd.simulate import make_dataset
    X, _, _ = make_dataset(d, 2 * d, seed=seed)
    rng = np.random.default_rng(seed)
    iu = np.array(np.triu_indices(d, 1)).T
    pairs = iu[rng.uniform(size=len(iu)) < 0.3]
    o = LinearOracle("l2")
    o.prepare(X.copy(), 0.03, 1000)
    o.trek = dict(kind="tcc", pairs=pairs, mode="opt", weight=0.2)
    return o, pairs


@pytest.mark.parametrize("d", [100, 300])
def test_tcc_short_chain_hands_back(d):
    """TCC with 2d > 128 on fast cov slots.  With the fixed-shift stage (one inverse at the warm
    start's Collatz-Wielandt bound, inverse iteration for v and u) the fast slot's chain is that
    stage alone, and a slot it does not settle hands back (tcc.hip tcc_handback_kernel); without it,
    a short Noda chain first: forced to hand back nearly every slot (1 step), by default (5 steps),
    and the whole chain on every slot (0).  The re-run is a pivoted slot with the whole chain.  W after
    60 steps from W = 0 (where the Perron gap is smallest and most fast slots hand back) within 1e-9
    of the oracle each time."""
    o, pairs = _tcc_case(d)
    K = 60
    Wr, tr = o.minimize(np.zeros((d, d)), 1.0, K, 1.0, 3e-4, tol=-1.0)
    backs = {}
    for fix, steps in ((False, 1), (False, None), (False, 0), (True, None)):
        s = _solver(d, o.cov)
        s.debug_tcc_fix(fix)
        if steps is not None:
            s.debug_tcc_fast_steps(steps)
        s.set_trek_tcc(pairs, mode="opt", weight=0.2)
        W = np.zeros((d, d))
        res = s.minimize(W, 1.0, K, 1.0, 3e-4, tol=-1.0, lambda1=0.03, checkpoint=1000)
        backs[fix, steps] = s.debug_handbacks()
        s.close()
        assert res.iters == K
        assert np.abs(W - Wr).max() <= 1e-9, (fix, steps, np.abs(W - Wr).max())
    assert backs[False, 1] >= K // 3  # forced: most fast slots handed back
    assert backs[False, 0] == 0


def test_tcc_fixed_stage_settles_warm_slots():
    """Past a fit's first steps the fixed-shift stage settles the fast slots by itself (d = 100:
    no more than 2 of the last 100 of 500 slots hand back), and W after the 500 steps is within 1e-9
    of the oracle's."""
    d, K0, K1 = 100, 400, 100
    o, pairs = _tcc_case(d)
    Wr, tr = o.minimize(np.zeros((d, d)), 1.0, K0 + K1, 1.0, 3e-4, tol=-1.0)
    s = _solver(d, o.cov)
    s.set_trek_tcc(pairs, mode="opt", weight=0.2)
    W = np.zeros((d, d))
    s.begin(W, 1.0, K0 + K1, 1.0, 3e-4, tol=-1.0, lambda1=0.03, checkpoint=1000)
    for _ in range(200):  # (a hand-back's re-run takes a slot of its own)
        if s.poll().iters >= K0:
            break
        s.run_slots(10)
    b0, i0 = s.debug_handbacks(), s.poll().iters
    for _ in range(200):
        if s.poll().iters >= K0 + K1:
            break
        s.run_slots(10)
    late = s.debug_handbacks() - b0
    res = s.end(W)
    s.close()
    assert res.iters == K0 + K1
    assert late <= 2, (late, K0 + K1 - i0)
    assert np.abs(W - Wr).max() <= 1e-9, np.abs(W - Wr).max()


def test_tcc_fast_blocks_match_the_pivoted_inverse_d1000():
    """d = 1000 (D2 = 2048, eight 256-blocks): the fixed-stage inverse of fast slots with every outer
    block but the last on the warm-started product-form series (tcc.hip tcc_inverse_fix) against
    the all-pivoted inverse: W after 80 steps from W = 0 (hand-backs included) within 1e-9.

    From W = 0 the fast-block leg hands back on 79 of its 80 steps (measured on an MI355X), so
    this run is in effect all-pivoted and carries no cap on the count; the fast blocks are compared
    with the oracle from W0 != 0 in test_minimize_with_tcc_blocked_matches_oracle."""
    d, K = 1000, 80
    o, pairs = _tcc_case(d)
    out = {}
    for fb in (False, True):
        s = _solver(d, o.cov)
        s.debug_tcc_fastblk(fb)
        s.set_trek_tcc(pairs, mode="opt", weight=0.2)
        W = np.zeros((d, d))
        res = s.minimize(W, 1.0, K, 1.0, 3e-4, tol=-1.0, lambda1=0.03, checkpoint=1000)
        assert res.iters == K
        out[fb] = (W.copy(), s.debug_handbacks())
        s.close()
    assert np.abs(out[True][0] - out[False][0]).max() <= 1e-9, np.abs(out[True][0] - out[False][0]).max()


# --- the blocked-inverse regime, d >= 993 (D2 >= 2048), against tests/golden/tcc_blocked*.npz ------
#
#   d     D2    block  outer blocks
#   993   2048  256    8     smallest d on the path, 62 padding rows
#   1000  2048  256    8     the benchmarked shape
#   1024  2048  256    8     no padding
#   1040  2112  -      -     binv_block(2112) = 0: the flat Gauss-Jordan (the seam inside the regime)
#   1088  2176  128    17    the 128-wide series, odd block count (the ping-pong starts in Aalt)
#   1152  2304  256    9     odd block count
_BLOCKED_POINT_D = (993, 1000, 1024, 1040, 1088, 1152)
_BLOCKED_TRAJ_D = (1000, 1088, 1152)


def _blocked_point_cases():
    import os
    f = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tcc_blocked.npz"))
    return [(d, case) for d in _BLOCKED_POINT_D for case in ("dense", "dag") if f"rho_{case}_d{d}" in f.files]


@pytest.mark.parametrize("d,case", _blocked_point_cases())
def test_tcc_value_grad_blocked_matches_oracle(golden, d, case):
    """trek_value at the shapes of the two-level blocked inverse against the oracle's closed form on
    the fixture's Perron triple (numpy eig, certified by tests/test_trek_oracle.py to 1e-11): the
    first call is cold (Noda on the pivoted blocked inverse), the second starts from the vectors
    the first left (the fixed-shift stage).  1e-10 relative, value and gradient, both times."""
    from oracle.trek_oracle import tcc_from_perron
    from tests.golden.make_tcc_blocked import point_inputs
    f = golden("tcc_blocked.npz")
    k = f"{case}_d{d}"
    W, pairs = point_inputs(d, case)
    assert W.sum() == float(f[f"guard_Wsum_{k}"]) and len(pairs) == int(f[f"guard_npairs_{k}"])
    assert np.array_equal(W[1, :8], f[f"guard_Wrow1_{k}"])
    vr, gr = tcc_from_perron(W, pairs, float(f[f"rho_{k}"]), f[f"u_{k}"], f[f"v_{k}"], 1e-12)
    s = _solver(d, np.eye(d))
    s.set_trek_tcc(pairs, mode="opt", weight=1.0)
    errs = []
    for call in ("cold", "warm"):
        v, g = s.trek_value(W)
        errs.append((call, abs(v - vr) / abs(vr), np.abs(g - gr).max() / np.abs(gr).max()))
        print(f"d={d} {case} {call}: value {errs[-1][1]:.2e} grad {errs[-1][2]:.2e} (relative)")
    s.close()
    for call, ev, eg in errs:
        assert ev <= 1e-10, (call, ev)
        assert eg <= 1e-10, (call, eg)


_blocked_traj_cache = {}


def _blocked_traj_inputs(d, f):
    """(cov, pairs, W0) of a trajectory case, built once for both fast-block settings; the guards
    tie them to the run the fixture recorded."""
    if d not in _blocked_traj_cache:
        from tests.golden.make_tcc_blocked import traj_w0
        o, pairs = _tcc_case(d)
        W0 = traj_w0(d, str(f[f"w0_traj_d{d}"]), o)
        assert o.cov.sum() == float(f[f"guard_covsum_traj_d{d}"])
        assert np.array_equal(o.cov[0, :8], f[f"guard_covrow0_traj_d{d}"])
        assert W0.sum() == float(f[f"guard_W0sum_traj_d{d}"])
        _blocked_traj_cache[d] = (o.cov, pairs, W0)
    return _blocked_traj_cache[d]


@pytest.mark.parametrize("fastblk", [False, True])
@pytest.mark.parametrize("d", _BLOCKED_TRAJ_D)
def test_minimize_with_tcc_blocked_matches_oracle(golden, d, fastblk):
    """24 steps with TCC from a dense W0 against the oracle's own 24 steps (tcc_blocked_traj.npz: W at
    32768 seeded positions, every row and column sum), with the fast blocks off and on.

    The hand-back cap (at most K // 4 of the fast-block run's slots re-run on the pivoted path) is
    not asserted at any d: measured on an MI355X, fast blocks on / off, 8 / 1 of 24 at d = 1000 and
    1088 and 12 / 2 at d = 1152 from the dense W0, and 8 / 1 at all three from the W after 400 plain
    steps.  So a third to a half of the fast-block run's slots pass on the pivoted path alone; the
    rest ran the product-form series, and the count is printed."""
    from tests.golden.make_tcc_blocked import K_TRAJ, traj_positions
    f = golden("tcc_blocked_traj.npz")
    cov, pairs, W0 = _blocked_traj_inputs(d, f)
    K = int(f[f"iters_traj_d{d}"])
    assert K == K_TRAJ
    s = _solver(d, cov)
    s.debug_tcc_fastblk(fastblk)
    s.set_trek_tcc(pairs, mode="opt", weight=0.2)
    W = W0.copy()
    res = s.minimize(W, 1.0, K, 1.0, 3e-4, tol=-1.0, lambda1=0.03, checkpoint=1000)
    backs = s.debug_handbacks()
    s.close()
    eW = np.abs(W.ravel()[traj_positions(d)] - f[f"W_traj_d{d}"]).max()
    eR = np.abs(W.sum(axis=1) - f[f"rowsum_traj_d{d}"]).max()
    eC = np.abs(W.sum(axis=0) - f[f"colsum_traj_d{d}"]).max()
    print(f"d={d} fastblk={fastblk}: hand-backs {backs} of {K}, max|dW| {eW:.2e}, row sums {eR:.2e}, "
          f"column sums {eC:.2e}")
    assert res.iters == K
    assert eW <= 1e-9
    assert eR <= d * 1e-9 and eC <= d * 1e-9
