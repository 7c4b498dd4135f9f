"""The logistic loss in the batch of small-d problems (csrc/logit_blk.h's row-block score phase,
`HipBatch.set_data` / `minimize_logistic` / `score_logistic`, `DagmaLogisticBatch`): the score
against numpy, trajectories against `LinearOracle("logistic")` and the single logistic solver,
bit-for-bit independence of a problem from the rest of the batch and from how X is stored, the
controller's branches in one call, the reference's fixture and a whole fit.

Shapes (d, n) sit on the tile and row-block edges: d at, below and above the 16 / 32 / 64 paddings,
n below one block, at a whole block, and ragged.  X is continuous (no L1-kink sign flips), so the
1e-9 trajectory bar applies without an envelope term, except where a test says otherwise."""
import functools

import numpy as np
import pytest
from scipy.special import expit

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from midagma_amd import _lib  # noqa: E402
from oracle.dagma_oracle import LinearOracle  # noqa: E402

SHAPES = [(1, 70), (16, 64), (17, 203), (20, 1000), (32, 129), (33, 257), (64, 200), (20, 7)]
LAMS = [0.0, 0.01, 0.02, 0.05, 0.1]
K, CKPT, LR = 300, 50, 3e-4
# every field of a checkpoint record but the device clock's
REC_FIELDS = tuple(f for f, _ in _lib.MidagmaCkpt._fields_ if f != "elapsed")
FIT_ARGS = dict(T=3, warm_iter=2000, max_iter=3000)


def _xs(d, n, B):
    rng = np.random.default_rng(100 + d)
    return [rng.normal(size=(n, d)) * 0.5 for _ in range(B)]


def _cov(X):
    return X.T @ X / float(X.shape[0])


def _batch(Xs, shared=False):
    """A HipBatch over the given X's (one X with shared: stored once), cov set as the reference forms it."""
    from midagma_amd.solver import HipBatch
    B, d = len(Xs), Xs[0].shape[1]
    bt = HipBatch(d, B, device=0)
    bt.set_cov(np.stack([_cov(X) for X in Xs]))
    if shared:
        assert all(X is Xs[0] for X in Xs)
        bt.set_data(Xs[0], shared=True)
    else:
        bt.set_data(np.stack(Xs))
    return bt


def _w_slabs(bt):
    out = np.empty((bt.B, 64, 64))
    assert bt.L.midagma_debug_batch_w_slabs(bt.h, _lib.dptr(out)) == 0
    return out


@functools.lru_cache(maxsize=None)
def _run5(d, n):
    """The B = 5 run of a shape, shared by the tests: (W, results with checkpoints, device W slabs)."""
    Xs = _xs(d, n, 5)
    bt = _batch(Xs)
    try:
        W = np.zeros((5, d, d))
        res = bt.minimize_logistic(W, 1.0, 1.0, LR, LAMS, K, tol=-1.0, checkpoint=CKPT, want_checkpoints=True)
        slabs = _w_slabs(bt)
    finally:
        bt.close()
    return W, res, slabs


@functools.lru_cache(maxsize=None)
def _oracle_run(d, n, b):
    o = LinearOracle("logistic")
    o.prepare(_xs(d, n, 5)[b].copy(), LAMS[b], CKPT)
    W, tr = o.minimize(np.zeros((d, d)), 1.0, K, 1.0, LR, tol=-1.0)
    return W, tr


@pytest.mark.parametrize("d,n", SHAPES)
def test_score_against_numpy(d, n):
    """`score_logistic` of B = 3 problems at a random W: the loss to 1e-10 relative, the gradient to
    1e-10 of max|G| (the bars of test_gpu_logistic._check_score).  A padded row or column that
    leaked its log 2 into the loss would move it by far more."""
    Xs = _xs(d, n, 3)
    rng = np.random.default_rng(7 + d)
    W = rng.normal(scale=0.02, size=(3, d, d))
    for b in range(3):
        np.fill_diagonal(W[b], 0.0)
    bt = _batch(Xs)
    try:
        loss, G = bt.score_logistic(W)
        loss_only, none = bt.score_logistic(W, grad=False)
    finally:
        bt.close()
    assert none is None and np.array_equal(loss, loss_only)
    for b, X in enumerate(Xs):
        Z = X @ W[b]
        ref_loss = (np.logaddexp(0.0, Z) - X * Z).sum() / n
        ref_G = X.T @ expit(Z) / n - _cov(X)
        print(f"d={d} n={n} b={b}: loss rel {abs(loss[b] - ref_loss) / abs(ref_loss):.2e}, "
              f"G rel {np.abs(G[b] - ref_G).max() / np.abs(ref_G).max():.2e}")
        assert abs(loss[b] - ref_loss) <= 1e-10 * abs(ref_loss)
        assert np.abs(G[b] - ref_G).max() <= 1e-10 * np.abs(ref_G).max()


@pytest.mark.parametrize("d,n", SHAPES)
def test_trajectory_against_the_oracle(d, n):
    """B = 5 problems (five X's, lambda1 = 0 .. 0.1), K = 300 steps from W = 0 without early stop:
    every W within 1e-9 of the oracle's, 6 checkpoint records whose objective and score agree to
    1e-10 relative, and the padding of the device W slabs exactly zero after the run (Z's padded
    columns are 0.5 colsum(X), which must never reach W)."""
    W, res, slabs = _run5(d, n)
    for b in range(5):
        Wo, tr = _oracle_run(d, n, b)
        assert res[b].iters == K == tr.iters and res[b].status == _lib.ST_DONE and res[b].halvings == 0
        assert len(res[b].checkpoints) == 6 == len(tr.checkpoints)
        print(f"d={d} n={n} b={b}: max|W - oracle| = {np.abs(W[b] - Wo).max():.2e}")
        assert np.abs(W[b] - Wo).max() <= 1e-9
        for rec, (it, obj, sc, h) in zip(res[b].checkpoints, tr.checkpoints):
            assert rec.iter == it
            assert abs(rec.obj - obj) <= 1e-10 * abs(obj), (b, it, rec.obj, obj)
            assert abs(rec.score - sc) <= 1e-10 * abs(sc), (b, it, rec.score, sc)
        assert np.array_equal(slabs[b, :d, :d], W[b])
        assert not slabs[b, d:, :].any() and not slabs[b, :, d:].any()


def _same_bits(Wa, ra, Wb, rb):
    assert np.array_equal(Wa, Wb)
    assert (ra.iters, ra.slots, ra.status, ra.halvings, ra.early_stop, ra.lr_final) == \
        (rb.iters, rb.slots, rb.status, rb.halvings, rb.early_stop, rb.lr_final)
    assert len(ra.checkpoints) == len(rb.checkpoints) > 0
    for x, y in zip(ra.checkpoints, rb.checkpoints):
        for f in REC_FIELDS:
            assert getattr(x, f) == getattr(y, f), (x.iter, f)


@pytest.mark.parametrize("d,n", [(17, 203), (64, 200)])
def test_a_problem_does_not_depend_on_the_batch_bit_for_bit(d, n):
    """Problem 2 of the B = 5 run, the same problem alone, and in a batch of 300 (more problems than
    compute units; the others are copies of its X with other lambda1) give the same bits in W and
    in every checkpoint field; so does one shared X against per-problem copies of it."""
    W5, res5, _ = _run5(d, n)
    X = _xs(d, n, 5)[2]
    bt = _batch([X])
    try:
        W1 = np.zeros((1, d, d))
        res1 = bt.minimize_logistic(W1, 1.0, 1.0, LR, LAMS[2], K, tol=-1.0, checkpoint=CKPT, want_checkpoints=True)
    finally:
        bt.close()
    _same_bits(W5[2], res5[2], W1[0], res1[0])
    B, at = 300, 137
    lams = [0.001 * (1 + b % 90) for b in range(B)]
    lams[at] = LAMS[2]
    out = {}
    for shared in (False, True):
        bt = _batch([X] * B if shared else [X.copy() for _ in range(B)], shared=shared)
        try:
            Wb = np.zeros((B, d, d))
            rb = bt.minimize_logistic(Wb, 1.0, 1.0, LR, lams, K, tol=-1.0, checkpoint=CKPT)
            out[shared] = (Wb, rb, bt.checkpoints(at), bt.checkpoints(0))
        finally:
            bt.close()
    for shared in (False, True):
        Wb, rb, ck, _ = out[shared]
        rb[at].checkpoints = ck
        _same_bits(W5[2], res5[2], Wb[at], rb[at])
    assert np.array_equal(out[False][0], out[True][0])  # all 300, shared against copies
    for x, y in zip(out[False][3], out[True][3]):
        for f in REC_FIELDS:
            assert getattr(x, f) == getattr(y, f), (x.iter, f)


@pytest.mark.parametrize("d,n", [(20, 1000), (64, 200)])
def test_against_the_single_logistic_solver(d, n):
    """Problem 2 against `HipSolver(d, "logistic", "data")` (the large-tile launch chain): W within
    1e-9, the same iteration count, status, halvings and early-stop flag."""
    from midagma_amd.solver import HipSolver
    W5, res5, _ = _run5(d, n)
    X = _xs(d, n, 5)[2]
    sol = HipSolver(d, "logistic", "data", device=0)
    try:
        sol.set_cov(_cov(X))
        sol.set_data(X, n_global=n)
        Ws = np.zeros((d, d))
        ref = sol.minimize(Ws, 1.0, K, 1.0, LR, tol=-1.0, lambda1=LAMS[2], checkpoint=CKPT)
    finally:
        sol.close()
    print(f"d={d} n={n}: max|W_batch - W_single| = {np.abs(W5[2] - Ws).max():.2e}")
    assert np.abs(W5[2] - Ws).max() <= 1e-9
    r = res5[2]
    assert (r.iters, r.status, r.halvings, r.early_stop) == (ref.iters, ref.status, ref.halvings, ref.early_stop)


def test_branches_in_one_call():
    """(17, 203), seed 5, lambda1 = 0, four problems on one X in one call: lr = 0.3 at s = 1 halves
    once and succeeds, lr = 0.3 at s = 0.9 leaves the domain and fails (linear.py:230-241), a plain
    run, and an inactive problem whose W comes back untouched.  Statuses, halvings and iteration
    counts are the oracle's; W of the plain and the halved problem within 1e-9."""
    d, n = 17, 203
    X = np.random.default_rng(5).normal(size=(n, d)) * 0.5
    lr = [0.3, 0.3, LR, LR]
    s = [1.0, 0.9, 1.0, 1.0]
    W = np.zeros((4, d, d))
    W[3] = np.random.default_rng(6).normal(scale=0.01, size=(d, d))
    W3 = W[3].copy()
    bt = _batch([X] * 4, shared=True)
    try:
        res = bt.minimize_logistic(W, 1.0, s, lr, 0.0, K, tol=-1.0, checkpoint=CKPT,
                                   active=[True, True, True, False])
    finally:
        bt.close()
    assert res[3] is None and np.array_equal(W[3], W3)
    for b in range(3):
        o = LinearOracle("logistic")
        o.prepare(X.copy(), 0.0, CKPT)
        Wo, tr = o.minimize(np.zeros((d, d)), 1.0, K, s[b], lr[b], tol=-1.0)
        print(f"problem {b}: iters {res[b].iters} / {tr.iters}, halvings {res[b].halvings} / {tr.halvings}, "
              f"status {res[b].status}")
        assert res[b].iters == tr.iters and res[b].halvings == tr.halvings and res[b].success == tr.success
        assert res[b].status == (_lib.ST_DONE if tr.success else _lib.ST_FAILED)
        if tr.success:
            assert np.abs(W[b] - Wo).max() <= 1e-9, b
    assert (res[0].halvings, res[0].iters) == (1, K) and (res[1].status, res[1].iters) == (_lib.ST_FAILED, 1)


@pytest.mark.parametrize("Kf", [1, 10, 100, 1000])
def test_the_reference_fixture(golden, Kf):
    """The reference's own minimize on its binary logit_X (traj_logistic_d20.npz, lambda1 = 0.05): W
    after K steps within max(1e-9, 2 env_K), env_K the fixture's (measured: 0, 0, 1.0e-17, 1.1e-16).

    What this pins: with binary X the exact score gradient of entry (17, 14) is 0 at W = 0
    (334 = colsum_17 / 2 = the co-occurrence count).  The reference's (mu / n X^T) @ expit(X W)
    scales X^T before the product and leaves +2.2e-16 there, whose sign picks the L1 subgradient
    branch; scaling the sum afterwards, 0.001 Z - 0.334, leaves 0.0 exactly and moved 20 entries by
    up to 1.65e-4.  The score phase scales X^T entry by entry before the product and adds an
    element's terms in ascending row order, as the reference does."""
    t = golden("traj_logistic_d20.npz")
    X = golden("data_meta.npz")["logit_X"].copy()
    d = X.shape[1]
    bt = _batch([X], shared=True)
    try:
        W = np.zeros((1, d, d))
        res = bt.minimize_logistic(W, 1.0, 1.0, LR, 0.05, Kf, tol=-1.0)
    finally:
        bt.close()
    assert res[0].success and res[0].iters == Kf == int(t[f"it_K{Kf}"])
    diff, env = np.abs(W[0] - t[f"W_K{Kf}"]), float(t[f"env_K{Kf}"])
    print(f"K={Kf}: max|W - W_ref| = {diff.max():.3e}, entries above 1e-9: {(diff > 1e-9).sum()}, env_K = {env:.1e}")
    assert diff.max() <= max(1e-9, 2 * env)


@functools.lru_cache(maxsize=None)
def _whole_fit():
    import os
    from midagma_amd import DagmaLogisticBatch
    golden_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    X = np.load(os.path.join(golden_dir, "data_meta.npz"))["logit_X"].copy()
    lams = [0.005, 0.01, 0.02, 0.05]
    m = DagmaLogisticBatch()
    W = m.fit(X, lambda1=lams, **FIT_ARGS)
    refs = []
    for lam in lams:
        o = LinearOracle("logistic")
        Wo = o.fit(X.copy(), lambda1=lam, **FIT_ARGS)
        refs.append((o, Wo))
    return m, W, refs


def test_whole_fit_stage_counts_and_supports():
    """`DagmaLogisticBatch.fit` on a lambda1 grid of 4 over the reference's logit_X (T = 3, 2000 / 3000
    iterations) against `LinearOracle("logistic").fit` per lambda1: the stages' iteration counts
    and the thresholded supports."""
    m, W, refs = _whole_fit()
    for b, (o, Wo) in enumerate(refs):
        got = [(r["iters"], r["success"]) for r in m.minimize_log[b]]
        want = [(tr.iters, tr.success) for (_, _, _, _, tr) in o.stages]
        print(f"lambda1 = {m.lambda1[b]}: stage iterations {[g[0] for g in got]} / {[w[0] for w in want]}, "
              f"edges {np.count_nonzero(W[b])} / {np.count_nonzero(Wo)}")
        assert got == want
        assert np.array_equal(W[b] != 0, Wo != 0)


def test_whole_fit_w_and_score_final():
    """The same fit: pre-threshold W within 1e-6 of the oracle's and score_final within 1e-9 relative
    (measured: W within 6.3e-14, score_final equal)."""
    m, W, refs = _whole_fit()
    dW = [float(np.abs(m.W_unthresholded[b] - o.W_unthresholded).max()) for b, (o, _) in enumerate(refs)]
    dS = [abs(m.score_final[b] - o.score_final) / abs(o.score_final) for b, (o, _) in enumerate(refs)]
    print("max|W - W_ref| per lambda1:", dW, "relative score_final difference:", dS)
    assert max(dW) <= 1e-6
    assert max(dS) <= 1e-9
