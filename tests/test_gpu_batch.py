"""A batch of small-d problems, one persistent workgroup each (csrc/batch.hip, `HipBatch`,
`DagmaLinearBatch`): problem b's W, counters and checkpoint records are bit-identical to the
single-problem path (`HipSolver` / `DagmaLinear`) on that problem alone, whatever the other
problems of the batch do (other endings, early stops, retries), with more problems than compute
units and over several launches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from midagma_amd import _lib  # noqa: E402
from midagma_amd.simulate import make_dataset  # noqa: E402
from oracle.dagma_oracle import LinearOracle  # noqa: E402

REC_FIELDS = ("obj", "score", "h", "lr", "w_norm", "max_abs_w", "min_abs_w_nonzero", "grad_raw_norm",
              "grad_step_norm", "grad_score_norm", "grad_dag_norm", "grad_l1_norm", "grad_inc_norm")


def _cov(d, seed, n=None):
    X, _, _ = make_dataset(d, n or max(200, 10 * d), seed=seed)
    X = X - X.mean(axis=0, keepdims=True)
    return X.T @ X / float(X.shape[0])


def _single(d, cov, mu, s, lr, lam, K, tol, checkpoint, masks=None):
    """(W, result with checkpoints) of the single-problem path; a singular matrix is raised there."""
    from midagma_amd.solver import HipSolver
    sol = HipSolver(d, "l2", "cov", device=0)
    try:
        sol.set_cov(cov)
        if masks is not None:
            sol.set_masks(*masks)
        W = np.zeros((d, d))
        res = sol.minimize(W, mu, K, s, lr, tol=tol, lambda1=lam, checkpoint=checkpoint, want_checkpoints=True)
    finally:
        sol.close()
    return W, res


def _same(res, ref):
    assert (res.iters, res.slots, res.status, res.halvings, res.early_stop, res.lr_final) == \
        (ref.iters, ref.slots, ref.status, ref.halvings, ref.early_stop, ref.lr_final)
    assert [c.iter for c in res.checkpoints] == [c.iter for c in ref.checkpoints]
    for x, y in zip(res.checkpoints, ref.checkpoints):
        for f in REC_FIELDS:
            assert getattr(x, f) == getattr(y, f), (x.iter, f)


@pytest.mark.parametrize("d", [1, 16, 17, 20, 32, 33, 64])
def test_batch_bit_identical_to_single(d):
    from midagma_amd.solver import HipBatch
    B, K = 5, 300
    lams = [0.01, 0.02, 0.03, 0.05, 0.1]
    covs = np.stack([_cov(d, 11 + b) for b in range(B)])
    bt = HipBatch(d, B, device=0)
    bt.set_cov(covs)
    W = np.zeros((B, d, d))
    res = bt.minimize(W, 1.0, 1.0, 3e-4, lams, K, tol=-1.0, checkpoint=50, want_checkpoints=True)
    bt.close()
    for b in range(B):
        Wr, ref = _single(d, covs[b], 1.0, 1.0, 3e-4, lams[b], K, -1.0, 50)
        assert res[b].iters == K and res[b].slots == K + 1 and len(res[b].checkpoints) == K // 50
        assert np.array_equal(W[b], Wr), b
        _same(res[b], ref)
    if d == 20:
        X, _, _ = make_dataset(20, 200, seed=13)
        o = LinearOracle("l2")
        o.prepare(X.copy(), lams[2], 50)
        Wo, tr = o.minimize(np.zeros((d, d)), 1.0, K, 1.0, 3e-4, tol=-1.0)
        assert tr.iters == K and np.abs(W[2] - Wo).max() <= 1e-9


def test_batch_heterogeneous_endings(golden):
    """One call: an lr halving at s = 1, the out-of-domain failure at s = 0.9 (linear.py:230-241, the
    reference's fixture branches.npz), a plain run and an inactive problem."""
    from midagma_amd.solver import HipBatch
    br = golden("branches.npz")
    X = golden("data_d20_n1000_seed0.npz")["X"].copy()
    o = LinearOracle("l2")
    o.prepare(X, 0.03, 1000)
    d, K = 20, 60
    lr, s = [0.3, 0.3, 3e-4, 3e-4], [1.0, 0.9, 1.0, 1.0]
    bt = HipBatch(d, 4, device=0)
    bt.set_cov(np.stack([o.cov] * 4))
    W = np.zeros((4, d, d))
    W[3] = 0.125 * np.arange(d * d).reshape(d, d)
    W3 = W[3].copy()
    res = bt.minimize(W, 1.0, s, lr, 0.03, K, tol=-1.0, active=[True, True, True, False], want_checkpoints=True)
    assert bt.checkpoints(3) == []
    bt.close()
    for b in range(3):
        Wr, ref = _single(d, o.cov, 1.0, s[b], lr[b], 0.03, K, -1.0, 1000)
        assert np.array_equal(W[b], Wr), b
        _same(res[b], ref)
    assert res[0].success and res[0].halvings == int(br["halve_nhalvings"]) and res[0].iters == int(br["halve_it"])
    assert np.abs(W[0] - br["halve_W"]).max() <= 1e-9
    assert res[1].status == _lib.ST_FAILED and not res[1].success and res[1].iters == int(br["ood_it"])
    assert np.abs(W[1] - br["ood_W"]).max() <= 1e-9
    assert res[2].status == _lib.ST_DONE and res[2].iters == K and res[2].halvings == 0
    assert res[3] is None and np.array_equal(W[3], W3)


def test_batch_different_early_stops_with_masks():
    from midagma_amd.solver import HipBatch
    d, B = 20, 4
    exc, inc = ((0, 1), (3, 2), (5, 7)), ((1, 0), (4, 9))
    o = LinearOracle("l2")
    o.prepare(make_dataset(d, 200, seed=11)[0], 0.03, 50, exc, inc)
    mi, me = o.masks(1.0)
    covs = np.stack([_cov(d, sd) for sd in (11, 12, 13, 14)])
    bt = HipBatch(d, B, device=0)
    bt.set_cov(covs)
    bt.set_masks(np.stack([mi] * B), np.stack([me] * B))
    W = np.zeros((B, d, d))
    res = bt.minimize(W, 1.0, 1.0, 3e-4, 0.03, 20000, tol=1e-6, checkpoint=50, want_checkpoints=True)
    bt.close()
    for b in range(B):
        Wr, ref = _single(d, covs[b], 1.0, 1.0, 3e-4, 0.03, 20000, 1e-6, 50, masks=(mi, me))
        assert res[b].early_stop and np.array_equal(W[b], Wr), b
        _same(res[b], ref)
        assert W[b][0, 1] == W[b][3, 2] == W[b][5, 7] == 0.0
    iters = [r.iters for r in res]
    print("early stops at", iters)
    assert len(set(iters)) > 1, iters


@pytest.mark.parametrize("d,B,K", [(16, 300, 5000), (64, 260, 200)])
def test_batch_more_problems_than_compute_units(d, B, K):
    """More workgroups than the device holds at once, and (K = 5000 slots > the 4096 of one launch)
    several launches: 6 distinct problems repeated over the batch, every copy bit-equal to its
    single solve."""
    from midagma_amd.solver import HipBatch
    lams = [0.01, 0.02, 0.03, 0.05, 0.1, 0.2]
    base = np.stack([_cov(d, 11 + k) for k in range(6)])
    which = np.arange(B) % 6
    bt = HipBatch(d, B, device=0)
    bt.set_cov(base[which])
    W = np.zeros((B, d, d))
    res = bt.minimize(W, 1.0, 1.0, 3e-4, [lams[k] for k in which], K, tol=-1.0, checkpoint=1000)
    ck = bt.checkpoints(B - 1)
    bt.close()
    for k in range(6):
        Wr, ref = _single(d, base[k], 1.0, 1.0, 3e-4, lams[k], K, -1.0, 1000)
        assert ref.iters == K
        for b in np.flatnonzero(which == k):
            assert np.array_equal(W[b], Wr), (k, b)
            assert (res[b].iters, res[b].slots, res[b].status) == (ref.iters, ref.slots, ref.status)
    last = (B - 1) % 6
    _, ref = _single(d, base[last], 1.0, 1.0, 3e-4, lams[last], K, -1.0, 1000)
    assert [(c.iter, c.obj, c.h) for c in ck] == [(c.iter, c.obj, c.h) for c in ref.checkpoints]


FIT_ARGS = dict(T=3, s=[1.0, .9, .8], warm_iter=300, max_iter=500, lr=0.3, checkpoint=100)


def _stage_rows(log):
    return [(r["s"], r["lr"], r["iters"], r["success"], r["halvings"]) for r in log]


def test_fit_equals_sequential_fits():
    from midagma_amd import DagmaLinear, DagmaLinearBatch
    seeds = range(11, 17)
    Xs = [make_dataset(20, 400, seed=sd)[0] for sd in seeds]
    s_arg = list(FIT_ARGS["s"])
    m = DagmaLinearBatch()
    W = m.fit([X.copy() for X in Xs], lambda1=0.03, **dict(FIT_ARGS, s=s_arg))
    assert s_arg == FIT_ARGS["s"] and W.shape == (6, 20, 20)
    for b, X in enumerate(Xs):
        one = DagmaLinear("l2")
        W1 = one.fit(X.copy(), lambda1=0.03, **dict(FIT_ARGS, s=list(FIT_ARGS["s"])))
        assert np.array_equal(W[b], W1), b
        assert m.h_final[b] == one.h_final and m.score_final[b] == one.score_final
        assert _stage_rows(m.minimize_log[b]) == _stage_rows(one.minimize_log)
    retries = [len(log) for log in m.minimize_log]
    print("minimize calls per problem:", retries)
    assert len(set(retries)) > 1, retries


def test_fit_lambda1_grid():
    from midagma_amd import DagmaLinear, DagmaLinearBatch
    X = make_dataset(20, 400, seed=11)[0]
    lams = [0.01, 0.03, 0.1]
    m = DagmaLinearBatch()
    W = m.fit(X.copy(), lambda1=lams, **dict(FIT_ARGS, s=list(FIT_ARGS["s"])))
    for b, lam in enumerate(lams):
        one = DagmaLinear("l2")
        W1 = one.fit(X.copy(), lambda1=lam, **dict(FIT_ARGS, s=list(FIT_ARGS["s"])))
        assert np.array_equal(W[b], W1), lam
        assert m.h_final[b] == one.h_final and m.score_final[b] == one.score_final
        assert _stage_rows(m.minimize_log[b]) == _stage_rows(one.minimize_log)


def test_fit_default_arguments():
    from midagma_amd import DagmaLinear, DagmaLinearBatch
    Xs = [make_dataset(20, 1000, seed=sd)[0] for sd in (0, 1, 2)]
    m = DagmaLinearBatch()
    W = m.fit(np.stack(Xs))
    for b, X in enumerate(Xs):
        one = DagmaLinear("l2")
        assert np.array_equal(W[b], one.fit(X.copy())), b
        assert m.h_final[b] == one.h_final and m.score_final[b] == one.score_final
        assert _stage_rows(m.minimize_log[b]) == _stage_rows(one.minimize_log)


def test_batch_errors():
    from midagma_amd.solver import HipBatch
    d, B = 8, 3
    bt = HipBatch(d, B, device=0)
    try:
        W = np.zeros((B, d, d))
        with pytest.raises(RuntimeError):
            bt.minimize(W, 1.0, 1.0, 3e-4, 0.03, 10)
        covs = np.stack([_cov(d, 11 + b) for b in range(B)])
        bad = covs.copy()
        bad[1, 2, 3] = np.nan
        with pytest.raises(ValueError):
            bt.set_cov(bad)
        with pytest.raises(RuntimeError):  # (the rejected cov was not installed)
            bt.minimize(W, 1.0, 1.0, 3e-4, 0.03, 10)
        bt.set_cov(covs)
        with pytest.raises(ValueError):
            bt.minimize(W, 1.0, 1.0, 3e-4, 0.03, 0)
        with pytest.raises(ValueError):
            bt.minimize(W, 1.0, 1.0, 3e-4, 0.03, 10, checkpoint=0)
        with pytest.raises(ValueError):
            bt.set_cov(covs[:2])
        assert all(r.iters == 10 for r in bt.minimize(W, 1.0, 1.0, 3e-4, 0.03, 10, tol=-1.0))
    finally:
        bt.close()


def test_batch_returns_to_baseline():
    """20 create / set_cov / minimize / close cycles leave the library's live byte count where it was
    (tests/test_gpu_lifetime.py's method)."""
    from midagma_amd.solver import HipBatch
    d, B = 20, 7
    covs = np.stack([_cov(d, 11 + b) for b in range(B)])
    live = _lib.load().midagma_debug_live_bytes
    base = int(live())
    for cycle in range(20):
        bt = HipBatch(d, B, device=0)
        bt.set_cov(covs)
        if cycle % 2:
            bt.set_masks(None, np.ones((B, d, d)))
        W = np.zeros((B, d, d))
        res = bt.minimize(W, 1.0, 1.0, 3e-4, 0.03, 40, tol=-1.0, checkpoint=10, want_checkpoints=True)
        assert all(r.iters == 40 and len(r.checkpoints) == 4 for r in res)
        assert int(live()) > base
        bt.close()
        assert int(live()) == base, cycle
