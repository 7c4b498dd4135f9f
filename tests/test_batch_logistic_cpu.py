"""The logistic batch without a device: the `midagma_blogit_*` entries of the C ABI, the argument
checks of `DagmaLogisticBatch`, and its lockstep stage / retry schedule against
`LinearOracle("logistic").fit` through a CPU double of `HipBatch`."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from midagma_amd import DagmaLogisticBatch, _lib
from oracle.dagma_oracle import LinearOracle, h_logdet, score

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOGIT_ENTRIES = ["midagma_blogit_minimize", "midagma_blogit_score", "midagma_blogit_set_data"]
FIT_ARGS = dict(T=3, warm_iter=2000, max_iter=3000)


def test_header_binding_and_library_agree_on_the_blogit_entries():
    src = open(os.path.join(REPO, "include", "midagma_hip.h")).read()
    declared = sorted(n for n in set(re.findall(r"\b(midagma_[a-z_0-9]+)\s*\(", src))
                      if n.startswith("midagma_blogit_"))
    assert declared == BLOGIT_ENTRIES
    assert sorted(n for n in _lib.EXPORTED if n.startswith("midagma_blogit_")) == BLOGIT_ENTRIES
    L = _lib.load()
    for name in BLOGIT_ENTRIES:
        assert hasattr(L, name), name
    assert L.midagma_abi_version() == 11  # additive entries


def test_blogit_entries_refuse_null_arguments_without_a_device():
    L = _lib.load()
    assert L.midagma_blogit_set_data(None, None, 10, 1) == _lib.E_ARG
    assert L.midagma_blogit_minimize(None, None, None, None, None, None, 10, 1e-6, .99, .999, 5, None,
                                     None) == _lib.E_ARG
    assert L.midagma_blogit_score(None, None, None, None) == _lib.E_ARG
    assert b"blogit_score" in L.midagma_batch_last_error(None)


class _DeviceTensor:
    """What `is_device_tensor` recognises, without torch or a device."""
    device = SimpleNamespace(type="cuda", index=0)
    shape = (50, 20)

    def data_ptr(self):
        return 0


def _no_backend(*a, **k):
    raise AssertionError("a backend was created before the arguments were checked")


def _model(**kw):
    return DagmaLogisticBatch(batch_factory=_no_backend, solver_factory=_no_backend, **kw)


def test_fit_rejects_bad_arguments_before_any_backend_is_built():
    X = (np.random.default_rng(0).uniform(size=(50, 20)) < 0.4).astype(np.float64)
    with pytest.raises(ValueError, match="one n"):
        _model().fit([X.copy(), X[:40].copy()])
    with pytest.raises(ValueError, match="trek"):
        _model(trek_reg=SimpleNamespace(enabled=lambda: True, name="pst"))
    _model(trek_reg=SimpleNamespace(enabled=lambda: False, name="pst"))  # (a disabled one is no regularizer)
    with pytest.raises(TypeError):
        _model().fit(X.copy(), lambda1=[0.01, 0.02], trek_weight=[0.1, 0.2])
    with pytest.raises(ValueError, match="float64"):
        _model(dtype=np.float32)
    with pytest.raises(ValueError):
        _model().fit([X.astype(np.float32)])
    with pytest.raises(ValueError, match="d <= 64"):
        _model().fit([np.zeros((100, 65))])
    with pytest.raises(ValueError, match="device tensor"):
        _model().fit([X.copy(), _DeviceTensor()])
    with pytest.raises(ValueError, match="device tensor"):
        _model().fit(_DeviceTensor())
    assert not hasattr(DagmaLogisticBatch, "bootstrap")


def test_the_l2_batch_names_the_logistic_class():
    from midagma_amd import DagmaLinearBatch
    with pytest.raises(ValueError, match="DagmaLogisticBatch"):
        DagmaLinearBatch(loss_type="logistic", batch_factory=_no_backend, solver_factory=_no_backend)


class OracleLogitBatch:
    """`HipBatch`'s logistic interface over `LinearOracle("logistic").minimize`, one problem after the
    other."""

    def __init__(self, d, B, device=0):
        self.d, self.B = d, B
        self.calls = [[] for _ in range(B)]
        self.data_calls = []
        OracleLogitBatch.last = self

    def set_cov(self, cov):
        self.cov = np.array(cov)

    def set_data(self, X, shared=False):
        self.data_calls.append((X, shared))
        self.X = [X] * self.B if shared else [X[b] for b in range(self.B)]

    def set_masks(self, mask_inc, mask_exc):
        assert mask_inc is None and mask_exc is None

    def _oracle(self, b, lambda1, checkpoint):
        o = LinearOracle("logistic")
        o.cov, o.lambda1, o.checkpoint, o.d = self.cov[b], lambda1, checkpoint, self.d
        o.eye, o.exc, o.inc, o.X, o.n = np.eye(self.d), None, None, self.X[b], self.X[b].shape[0]
        return o

    def minimize(self, *a, **k):
        raise AssertionError("the logistic class must call minimize_logistic")

    def minimize_logistic(self, W, mu, s, lr, lambda1, max_iter, tol=1e-6, beta_1=.99, beta_2=.999,
                          checkpoint=1000, active=None, want_checkpoints=False):
        out = [None] * self.B
        for b in range(self.B):
            if active is not None and not active[b]:
                continue
            o = self._oracle(b, lambda1[b], checkpoint)
            _, tr = o.minimize(W[b], mu, max_iter, s[b], lr[b], tol=tol, beta_1=beta_1, beta_2=beta_2)
            self.calls[b].append((mu, s[b], lr[b], tr.iters, tr.success))
            out[b] = SimpleNamespace(iters=tr.iters, success=tr.success, early_stop=tr.early_stop,
                                     halvings=tr.halvings, status=_lib.ST_DONE if tr.success else _lib.ST_FAILED)
        return out

    def score_logistic(self, W, grad=True):
        return np.array([score("logistic", W[b], self.cov[b], self.X[b])[0] for b in range(self.B)]), None

    def close(self):
        pass


class OracleSolver:
    def __init__(self, d, loss, mode, device=0):
        pass

    def h_value(self, W, s=1.0, grad=True):
        return h_logdet(W, s)

    def close(self):
        pass


def _binary(n, d, seed, p=0.35):
    return (np.random.default_rng(seed).uniform(size=(n, d)) < p).astype(np.float64)


def test_fit_matches_the_oracle_fit_per_problem_and_leaves_x_alone(golden):
    """Three X's (the reference's binary logit_X and two others of the same shape): every problem's
    sequence of (mu, s, lr, iters, success), its W, h_final and score_final equal
    `LinearOracle("logistic").fit` on that problem alone; X is neither centred nor written."""
    Xl = golden("data_meta.npz")["logit_X"].copy()
    n, d = Xl.shape
    Xs = [Xl, _binary(n, d, 3), np.random.default_rng(4).normal(size=(n, d)) * 0.5]
    given = [X.copy() for X in Xs]
    m = DagmaLogisticBatch(batch_factory=OracleLogitBatch, solver_factory=OracleSolver)
    W = m.fit(given, lambda1=0.05, **FIT_ARGS)
    for X, X0 in zip(given, Xs):
        assert np.array_equal(X, X0)
    back = OracleLogitBatch.last
    assert len(back.data_calls) == 1 and back.data_calls[0][1] is False
    assert back.data_calls[0][0].shape == (3, n, d)
    for b, X in enumerate(Xs):
        o = LinearOracle("logistic")
        W_ref = o.fit(X.copy(), lambda1=0.05, **FIT_ARGS)
        assert back.calls[b] == [(mu, s, lr, tr.iters, tr.success) for (_, mu, s, lr, tr) in o.stages]
        assert np.array_equal(W[b], W_ref)
        assert m.h_final[b] == o.h_final and m.score_final[b] == o.score_final
        assert [(r["s"], r["lr"], r["iters"], r["success"], r["halvings"]) for r in m.minimize_log[b]] == \
            [(s, lr, tr.iters, tr.success, tr.halvings) for (_, _, s, lr, tr) in o.stages]


def test_the_lambda1_grid_hands_one_shared_x_to_the_backend(golden):
    X = golden("data_meta.npz")["logit_X"].copy()
    X0 = X.copy()
    m = DagmaLogisticBatch(batch_factory=OracleLogitBatch, solver_factory=OracleSolver)
    lams = [0.02, 0.05]
    W = m.fit(X, lambda1=lams, T=2, warm_iter=300, max_iter=500)
    assert W.shape == (2, 20, 20) and np.array_equal(X, X0)
    back = OracleLogitBatch.last
    assert len(back.data_calls) == 1
    Xb, shared = back.data_calls[0]
    assert shared is True and Xb is X
    assert m.cov[0] is m.cov[1] and np.array_equal(m.cov[0], X0.T @ X0 / float(X0.shape[0]))
    for b, lam in enumerate(lams):
        assert np.array_equal(W[b], LinearOracle("logistic").fit(X0.copy(), lambda1=lam, T=2, warm_iter=300,
                                                                  max_iter=500))
