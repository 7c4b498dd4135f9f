"""The PST trek regularizer in a batch (csrc/pst_blk.h inside the small-d persistent loop,
`HipBatch.set_trek` / `trek_value`, `DagmaLinearBatch(trek_reg=...)`): the one-workgroup body against
the reference's fixtures and the oracle at every block size and squaring count, trajectories against
`LinearOracle.minimize`, independence of a problem from the rest of its batch (bit for bit), and the
public path against `DagmaLinear` on the launch chain."""
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from midagma_amd import _lib  # noqa: E402
from midagma_amd.simulate import make_dataset  # noqa: E402
from oracle.dagma_oracle import LinearOracle  # noqa: E402
from oracle.trek_oracle import pst_value_grad  # noqa: E402

AGGS = ("mean", "sum", "max", "lse")
REC_FIELDS = ("obj", "score", "h", "lr", "w_norm", "max_abs_w", "min_abs_w_nonzero", "grad_raw_norm",
              "grad_step_norm", "grad_score_norm", "grad_dag_norm", "grad_l1_norm", "grad_inc_norm",
              "reg_trek_value", "grad_trek_norm")


def _batch(d, B):
    from midagma_amd.solver import HipBatch
    return HipBatch(d, B, device=0)


def _centered(d, seed, n=1000):
    X, _, _ = make_dataset(d, n, seed=seed)
    return X - X.mean(axis=0, keepdims=True)


def _cov(d, seed):
    X = _centered(d, seed, max(200, 10 * d))
    return X.T @ X / float(X.shape[0])


def _upper_pairs(d, seed, frac=0.3):
    iu = np.array(np.triu_indices(d, 1)).T
    P = iu[np.random.default_rng(seed).uniform(size=len(iu)) < frac]
    return P if len(P) else iu[:1]


# ------------------------------------------------------------------ the body
@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("seq", ["exp", "inv"])
@pytest.mark.parametrize("d", [8, 20])
def test_body_matches_the_reference_fixtures(golden, d, seq, agg):
    """B = 3: the fixture W twice (the reference's own value and gradient) and 0.5 W (the oracle)."""
    z = golden("trek_pst.npz")
    W, pairs = z[f"W_d{d}"], z[f"pairs_d{d}"]
    Ws = np.stack([W, 0.5 * W, W])
    refs = [(float(z[f"val_{seq}_{agg}_d{d}"]), z[f"grad_{seq}_{agg}_d{d}"]),
            pst_value_grad(0.5 * W, pairs, seq, agg=agg)]
    bt = _batch(d, 3)
    try:
        bt.set_trek(pairs, seq, agg=agg, mode="opt", weight=1.0)
        v, g = bt.trek_value(Ws)
        v_only, none = bt.trek_value(Ws, grad=False)
    finally:
        bt.close()
    assert none is None and np.array_equal(v, v_only)
    for b, (v_ref, g_ref) in zip(range(3), (refs[0], refs[1], refs[0])):
        dv, dg = abs(v[b] - v_ref), np.abs(g[b] - g_ref).max()
        print(f"d={d} {seq}/{agg} b={b}: dv={dv:.2e} dg={dg:.2e}")
        assert dv <= 1e-11 * max(1.0, abs(v_ref))
        assert dg <= 1e-10 * max(1.0, np.abs(g_ref).max())


def _sparse_w(d, norm1, seed):
    """A random sparse W with ||W o W||_1 = norm1 (d = 1: the one diagonal entry)."""
    rng = np.random.default_rng(seed)
    W = rng.uniform(-1, 1, (d, d)) * (rng.uniform(size=(d, d)) < min(1.0, 4.0 / d))
    if d > 1:
        np.fill_diagonal(W, 0)
    if not np.any(W):
        W[0, d - 1] = 0.7
    return W * np.sqrt(norm1 / (W * W).sum(axis=0).max())


def _odd_pairs(d, seed):
    """A pair list with a duplicate, a reversed pair and a diagonal pair."""
    if d == 1:
        return np.array([[0, 0], [0, 0]])
    P = _upper_pairs(d, seed)
    return np.concatenate([P, P[:1], P[:1, ::-1], [[d - 1, d - 1]]])


@pytest.mark.parametrize("seq,norm1", [("exp", 0.1), ("exp", 1.0), ("exp", 6.0), ("inv", 0.1)])
@pytest.mark.parametrize("d", [1, 16, 17, 32])
def test_body_shapes_and_squaring_counts(d, seq, norm1):
    """Both block sizes at and beside their edges; ||W o W||_1 = 0.1, 1, 6 squares 0, 2 and 5 times.
    One aggregation per problem of the batch would need four handles: the four run in turn."""
    pairs = _odd_pairs(d, 3)
    Ws = np.stack([_sparse_w(d, norm1, 5), _sparse_w(d, norm1, 6), 0.3 * _sparse_w(d, norm1, 7)])
    bt = _batch(d, 3)
    try:
        for agg in AGGS:
            bt.set_trek(pairs, seq, agg=agg, mode="opt", weight=1.0)
            v, g = bt.trek_value(Ws)
            for b in range(3):
                v_ref, g_ref = pst_value_grad(Ws[b], pairs, seq, agg=agg)
                dv, dg = abs(v[b] - v_ref), np.abs(g[b] - g_ref).max()
                print(f"d={d} {seq}/{agg} norm={norm1} b={b}: dv/|v|={dv / abs(v_ref):.2e} "
                      f"dg/|g|={dg / max(np.abs(g_ref).max(), 1e-300):.2e}")
                assert dv <= 1e-10 * abs(v_ref)
                assert dg <= 1e-9 * np.abs(g_ref).max()
    finally:
        bt.close()


@pytest.mark.parametrize("seq", ["exp", "inv"])
@pytest.mark.parametrize("d", [16, 17])
def test_body_at_w_zero(d, seq):
    """W = 0: F = I (inv: I / (1 + eps)), so H vanishes off the diagonal: value 0, gradient exactly 0."""
    pairs = _upper_pairs(d, 3)
    bt = _batch(d, 2)
    try:
        bt.set_trek(np.concatenate([pairs, pairs[:1, ::-1]]), seq, agg="mean", mode="opt", weight=1.0)
        v, g = bt.trek_value(np.zeros((2, d, d)))
    finally:
        bt.close()
    assert np.array_equal(v, np.zeros(2)) and np.array_equal(g, np.zeros((2, d, d)))


# -------------------------------------------------------------- trajectories
@pytest.mark.parametrize("d,seq,mode,agg", [(8, "exp", "opt", "mean"), (20, "exp", "opt", "mean"),
                                            (32, "exp", "opt", "mean"), (8, "inv", "opt", "mean"),
                                            (20, "inv", "opt", "mean"), (32, "inv", "opt", "mean"),
                                            (8, "exp", "log", "mean"), (20, "exp", "log", "mean"),
                                            (32, "exp", "log", "mean"), (20, "exp", "opt", "lse")])
def test_minimize_with_trek_matches_oracle(d, seq, mode, agg):
    """`test_gpu_trek.py::test_minimize_with_trek_matches_oracle` per problem of a batch of 3 with its
    own data, lambda1 and weight; the third problem is inactive."""
    B, K = 3, 90
    lams, weights = [0.03, 0.05, 0.02], [0.2, 0.05, 0.4]
    pairs = _upper_pairs(d, 5)
    oracles = []
    for b in range(B):
        o = LinearOracle("l2")
        o.prepare(_centered(d, 5 + b), lams[b], 40)
        o.trek = dict(pairs=pairs, seq=seq, agg=agg, mode=mode, weight=weights[b])
        oracles.append(o)
    bt = _batch(d, B)
    try:
        bt.set_cov(np.stack([o.cov for o in oracles]))
        bt.set_trek(pairs, seq, agg=agg, mode=mode, weight=weights)
        W = np.zeros((B, d, d))
        W[2] = 0.125
        res = bt.minimize(W, 1.0, 1.0, 3e-4, lams, K, tol=-1.0, checkpoint=40, active=[True, True, False],
                          want_checkpoints=True)
    finally:
        bt.close()
    assert res[2] is None and np.array_equal(W[2], np.full((d, d), 0.125))
    for b in range(2):
        Wr, tr = oracles[b].minimize(np.zeros((d, d)), 1.0, K, 1.0, 3e-4, tol=-1.0)
        assert res[b].iters == tr.iters == K
        print(f"d={d} {seq}/{mode}/{agg} b={b}: max|dW|={np.abs(W[b] - Wr).max():.2e}")
        assert np.abs(W[b] - Wr).max() <= 1e-9
        assert [c.iter for c in res[b].checkpoints] == [r["iter"] for r in tr.records]
        for c, r in zip(res[b].checkpoints, tr.records):
            assert abs(c.obj - r["obj_total"]) <= 1e-10 * abs(r["obj_total"])
            assert abs(c.reg_trek_value - r["reg_trek_value"]) <= 1e-9 * abs(r["reg_trek_value"]) + 1e-13
            assert abs(c.grad_trek_norm - r["grad_trek_norm"]) <= 1e-9 * r["grad_trek_norm"] + 1e-13
        assert any(c.reg_trek_value > 0.0 for c in res[b].checkpoints)
        if mode == "log":
            assert all(c.grad_trek_norm == 0.0 for c in res[b].checkpoints)
        else:
            assert all(c.grad_trek_norm > 0.0 for c in res[b].checkpoints)


# -------------------------------------------------------------- independence
def _same(res, ref):
    assert (res.iters, res.slots, res.status, res.halvings, res.early_stop, res.lr_final) == \
        (ref.iters, ref.slots, ref.status, ref.halvings, ref.early_stop, ref.lr_final)
    assert [c.iter for c in res.checkpoints] == [c.iter for c in ref.checkpoints]
    for x, y in zip(res.checkpoints, ref.checkpoints):
        for f in REC_FIELDS:
            assert getattr(x, f) == getattr(y, f), (x.iter, f)


def _run(d, covs, lams, weights, pairs, K, checkpoint, seq="exp", trek=True):
    B = len(lams)
    bt = _batch(d, B)
    try:
        bt.set_cov(np.stack(covs))
        if trek:
            bt.set_trek(pairs, seq, agg="mean", mode="opt", weight=weights)
        W = np.zeros((B, d, d))
        res = bt.minimize(W, 1.0, 1.0, 3e-4, lams, K, tol=-1.0, checkpoint=checkpoint, want_checkpoints=True)
    finally:
        bt.close()
    return W, res


@pytest.mark.parametrize("d,seq", [(20, "exp"), (20, "inv"), (16, "exp")])
def test_problem_does_not_depend_on_its_batch(d, seq):
    B, K = 5, 200
    lams, weights = [0.01, 0.02, 0.03, 0.05, 0.1], [0.1, 0.2, 0.3, 0.05, 1.0]
    covs = [_cov(d, 11 + b) for b in range(B)]
    pairs = _upper_pairs(d, 5)
    W, res = _run(d, covs, lams, weights, pairs, K, 50, seq)
    for b in range(B):
        W1, r1 = _run(d, covs[b:b + 1], lams[b:b + 1], weights[b:b + 1], pairs, K, 50, seq)
        assert np.array_equal(W[b], W1[0]), b
        _same(res[b], r1[0])
        assert all(c.reg_trek_value > 0.0 and c.grad_trek_norm > 0.0 for c in res[b].checkpoints)


def test_more_problems_than_compute_units_over_several_launches():
    """300 workgroups, 5000 slots (more than one launch holds): 6 distinct problems repeated over the
    batch, every copy bit-equal to its batch of one."""
    d, B, K = 16, 300, 5000
    lams, weights = [0.01, 0.02, 0.03, 0.05, 0.1, 0.2], [0.1, 0.2, 0.3, 0.05, 1.0, 0.5]
    base = [_cov(d, 11 + k) for k in range(6)]
    which = np.arange(B) % 6
    pairs = _upper_pairs(d, 5)
    W, res = _run(d, [base[k] for k in which], [lams[k] for k in which], [weights[k] for k in which], pairs, K, 1000)
    for k in range(6):
        W1, r1 = _run(d, base[k:k + 1], lams[k:k + 1], weights[k:k + 1], pairs, K, 1000)
        assert r1[0].iters == K
        for b in np.flatnonzero(which == k):
            assert np.array_equal(W[b], W1[0]), (k, b)
            _same(res[b], r1[0])


@pytest.mark.parametrize("d", [20, 40])
def test_off_means_off(d):
    """After set_trek(mode='off'), or with no pairs, the batch is the batch that never set one."""
    B, K = 3, 120
    lams = [0.01, 0.03, 0.1]
    covs = [_cov(d, 11 + b) for b in range(B)]
    pairs = _upper_pairs(d, 5)
    W0, res0 = _run(d, covs, lams, None, None, K, 40, trek=False)
    for how in ("off", "empty"):
        bt = _batch(d, B)
        try:
            bt.set_cov(np.stack(covs))
            if d <= 32:
                bt.set_trek(pairs, "exp", mode="opt", weight=0.3)
            if how == "off":
                bt.set_trek(pairs, "exp", mode="off", weight=0.3)
            else:
                bt.set_trek(np.zeros((0, 2), dtype=np.int64), "exp", mode="opt", weight=0.3)
            W = np.zeros((B, d, d))
            res = bt.minimize(W, 1.0, 1.0, 3e-4, lams, K, tol=-1.0, checkpoint=40, want_checkpoints=True)
            v, g = bt.trek_value(W)
        finally:
            bt.close()
        assert np.array_equal(W, W0), how
        for b in range(B):
            _same(res[b], res0[b])
        assert not v.any() and not g.any()


# --------------------------------------------------------------- public path
def _reg(pairs, weight, seq="exp", mode="opt"):
    return SimpleNamespace(name="pst", mode=mode, weight=weight, cfg={"I": pairs, "seq": seq, "kwargs": {}},
                           enabled=lambda: True)


def test_fit_with_a_weight_grid_matches_the_launch_chain():
    from midagma_amd import DagmaLinear, DagmaLinearBatch
    d, weights = 20, [0.05, 0.4]
    Xs = [make_dataset(d, 1000, seed=sd)[0] for sd in (7, 8)]
    pairs = _upper_pairs(d, 7)
    args = dict(lambda1=0.03, T=2, warm_iter=200, max_iter=300, w_threshold=0.0)
    m = DagmaLinearBatch(trek_reg=_reg(pairs, 123.0))
    W = m.fit([X.copy() for X in Xs], trek_weight=weights, **args)
    assert W.shape == (2, d, d) and m.trek_final.shape == (2,)
    for b in range(2):
        one = DagmaLinear("l2", trek_reg=_reg(pairs, weights[b]))
        W1 = one.fit(Xs[b].copy(), **args)
        print(f"b={b}: max|dW|={np.abs(W[b] - W1).max():.2e}")
        assert np.abs(W[b] - W1).max() <= 1e-9
        v_ref, _ = pst_value_grad(m.W_est[b], pairs, "exp", grad=False)
        assert v_ref > 0.0 and abs(m.trek_final[b] - v_ref) <= 1e-11 * max(1.0, abs(v_ref))
    assert np.abs(W[0] - W[1]).max() > 1e-6  # (the weights differ, and so do the fits)


def test_set_trek_errors():
    pairs = np.array([[0, 1], [2, 3]])
    bt = _batch(33, 2)
    try:
        with pytest.raises(ValueError, match="d <= 32"):
            bt.set_trek(pairs, "exp", weight=0.1)
    finally:
        bt.close()
    bt = _batch(8, 2)
    try:
        with pytest.raises(ValueError, match="log"):
            bt.set_trek(pairs, "log", weight=0.1)
        with pytest.raises(ValueError, match="binom"):
            bt.set_trek(pairs, "binom", weight=0.1)
        with pytest.raises(ValueError, match="pair index"):
            bt.set_trek(np.array([[0, 8]]), "exp", weight=0.1)
        with pytest.raises(ValueError, match="finite"):
            bt.set_trek(pairs, "exp", weight=[0.1, np.inf])
        with pytest.raises(ValueError):
            bt.set_trek(pairs, "exp", weight=[0.1, 0.2, 0.3])
    finally:
        bt.close()


def test_batch_with_trek_returns_to_baseline():
    """20 create / set_cov / set_trek / minimize / trek_value / close cycles leave the library's live
    byte count where it was (`test_gpu_batch.py::test_batch_returns_to_baseline`'s method)."""
    d, B = 20, 7
    covs = np.stack([_cov(d, 11 + b) for b in range(B)])
    pairs = _upper_pairs(d, 5)
    live = _lib.load().midagma_debug_live_bytes
    base = int(live())
    for cycle in range(20):
        bt = _batch(d, B)
        bt.set_cov(covs)
        bt.set_trek(pairs, "inv" if cycle % 2 else "exp", weight=0.1)
        if cycle % 3 == 0:
            bt.set_trek(pairs, "exp", agg="lse", weight=np.linspace(0.1, 0.7, B))
        W = np.zeros((B, d, d))
        res = bt.minimize(W, 1.0, 1.0, 3e-4, 0.03, 40, tol=-1.0, checkpoint=10, want_checkpoints=True)
        assert all(r.iters == 40 and len(r.checkpoints) == 4 for r in res)
        v, g = bt.trek_value(W)
        assert v.shape == (B,) and g.shape == (B, d, d) and np.all(v > 0.0)
        assert int(live()) > base
        bt.close()
        assert int(live()) == base, cycle
