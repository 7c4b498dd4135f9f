"""The batch of small-d problems without a device: the C ABI's new entries, the argument checks of
`midagma_batch_create` and `DagmaLinearBatch`, and the lockstep stage / retry schedule of
`DagmaLinearBatch.fit` against `LinearOracle.fit` through a CPU double of `HipBatch`."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from midagma_amd import _lib
from midagma_amd.batch import DagmaLinearBatch
from midagma_amd.simulate import make_dataset
from oracle.dagma_oracle import LinearOracle, h_logdet, score

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_ENTRIES = ["midagma_batch_checkpoints", "midagma_batch_create", "midagma_batch_destroy",
                 "midagma_batch_last_error", "midagma_batch_minimize", "midagma_batch_set_cov",
                 "midagma_batch_set_masks"]


def test_header_binding_and_library_agree_on_the_batch_entries():
    src = open(os.path.join(REPO, "include", "midagma_hip.h")).read()
    declared = sorted(n for n in set(re.findall(r"\b(midagma_[a-z_0-9]+)\s*\(", src)) if n.startswith("midagma_batch_"))
    assert declared == BATCH_ENTRIES
    assert sorted(n for n in _lib.EXPORTED if n.startswith("midagma_batch_")) == BATCH_ENTRIES
    L = _lib.load()
    for name in BATCH_ENTRIES:
        assert hasattr(L, name), name
    assert L.midagma_abi_version() == 11  # additive entries


@pytest.mark.parametrize("d,B", [(0, 4), (65, 4), (20, 0), (20, 16385)])
def test_batch_create_validates_without_a_device(d, B):
    L = _lib.load()
    out = C.c_void_p()
    assert L.midagma_batch_create(C.byref(out), d, B, 0) == _lib.E_ARG
    assert not out.value
    assert b"batch_create" in L.midagma_batch_last_error(None)


def test_batch_entries_refuse_null_arguments_without_a_device():
    L = _lib.load()
    assert L.midagma_batch_create(None, 20, 4, 0) == _lib.E_ARG
    assert L.midagma_batch_set_cov(None, None) == _lib.E_ARG
    assert L.midagma_batch_set_masks(None, None, None) == _lib.E_ARG
    assert L.midagma_batch_minimize(None, None, None, None, None, None, 10, 1e-6, .99, .999, 5, None, None) == _lib.E_ARG
    assert L.midagma_batch_checkpoints(None, 0, None, 0) == _lib.E_ARG
    L.midagma_batch_destroy(None)


class _DeviceTensor:
    """What `is_device_tensor` recognises, without torch or a device."""
    device = SimpleNamespace(type="cuda", index=0)
    shape = (50, 20)

    def data_ptr(self):
        return 0


def _no_backend(*a, **k):
    raise AssertionError("a backend was created before the arguments were checked")


def _model(**kw):
    return DagmaLinearBatch(batch_factory=_no_backend, solver_factory=_no_backend, **kw)


def test_fit_rejects_bad_arguments_before_any_device_work():
    X = np.random.default_rng(0).standard_normal((50, 20))
    with pytest.raises(ValueError):
        _model(loss_type="logistic")
    with pytest.raises(ValueError):
        _model(dtype=np.float32)
    with pytest.raises(ValueError):
        _model(trek_reg=SimpleNamespace(enabled=lambda: True, name="tcc"))
    _model(trek_reg=SimpleNamespace(enabled=lambda: False, name="tcc"))  # (a disabled one is no regularizer)
    with pytest.raises(ValueError, match="d <= 64"):
        _model().fit([np.zeros((100, 65))])
    with pytest.raises(ValueError, match="share d"):
        _model().fit([X.copy(), np.zeros((50, 19))])
    with pytest.raises(ValueError, match="empty"):
        _model().fit([])
    with pytest.raises(ValueError, match="lambda1"):
        _model().fit([X.copy(), X.copy()], lambda1=[0.01, 0.02, 0.03])
    with pytest.raises(ValueError, match="device tensor"):
        _model().fit([X.copy(), _DeviceTensor()])
    with pytest.raises(ValueError, match="device tensor"):
        _model().fit(_DeviceTensor())
    with pytest.raises(ValueError):
        _model().fit([X.astype(np.float32)])


FIT_ARGS = dict(T=3, s=[1.0, .9, .8], warm_iter=300, max_iter=500, lr=0.3, checkpoint=100)


class OracleBatch:
    """`HipBatch`'s interface over `LinearOracle.minimize`, one problem after the other."""
    calls: list  # per problem: (mu, s, lr, iters, success) of every minimize that ran it

    def __init__(self, d, B, device=0):
        self.d, self.B = d, B
        self.calls = [[] for _ in range(B)]
        OracleBatch.last = self

    def set_cov(self, cov):
        self.cov = np.array(cov)

    def set_masks(self, mask_inc, mask_exc):
        assert mask_inc is None and mask_exc is None

    def minimize(self, W, mu, s, lr, lambda1, max_iter, tol=1e-6, beta_1=.99, beta_2=.999, checkpoint=1000,
                 active=None, want_checkpoints=False):
        out = [None] * self.B
        for b in range(self.B):
            if active is not None and not active[b]:
                continue
            o = LinearOracle("l2")
            o.cov, o.lambda1, o.checkpoint, o.d = self.cov[b], lambda1[b], checkpoint, self.d
            o.eye, o.exc, o.inc, o.X = np.eye(self.d), None, None, None  # (cov mode: X is not read)
            _, tr = o.minimize(W[b], mu, max_iter, s[b], lr[b], tol=tol, beta_1=beta_1, beta_2=beta_2)
            self.calls[b].append((mu, s[b], lr[b], tr.iters, tr.success))
            out[b] = SimpleNamespace(iters=tr.iters, success=tr.success, early_stop=tr.early_stop,
                                     halvings=tr.halvings, status=_lib.ST_DONE if tr.success else _lib.ST_FAILED)
        return out

    def close(self):
        pass


class OracleSolver:
    def __init__(self, d, loss, mode, device=0):
        pass

    def set_cov(self, cov):
        self.cov = cov

    def h_value(self, W, s=1.0, grad=True):
        return h_logdet(W, s)

    def score_value(self, W):
        return score("l2", W, self.cov)

    def close(self):
        pass


def test_fit_schedule_matches_the_oracle_fit_per_problem():
    """Stages in lockstep, retries per problem: seed 11 retries stages 1 and 2 once each (5 minimize
    calls), seed 15 retries stage 2 twice (6), so the two leave lockstep; each problem's sequence
    of (mu, s, lr, iters, success) and its result equal `LinearOracle.fit` on that problem alone."""
    seeds = (11, 15)
    Xs = [make_dataset(20, 400, seed=sd)[0] for sd in seeds]
    s_arg = list(FIT_ARGS["s"])
    m = DagmaLinearBatch(batch_factory=OracleBatch, solver_factory=OracleSolver)
    W = m.fit([X.copy() for X in Xs], lambda1=0.03, **dict(FIT_ARGS, s=s_arg))
    assert s_arg == FIT_ARGS["s"]  # the caller's list is not touched
    calls = OracleBatch.last.calls
    assert [len(c) for c in calls] == [5, 6]
    for b, X in enumerate(Xs):
        o = LinearOracle("l2")
        W_ref = o.fit(X.copy(), lambda1=0.03, **dict(FIT_ARGS, s=list(FIT_ARGS["s"])))
        assert calls[b] == [(mu, s, lr, tr.iters, tr.success) for (_, mu, s, lr, tr) in o.stages]
        assert np.array_equal(W[b], W_ref)
        assert m.h_final[b] == o.h_final and m.score_final[b] == o.score_final
        assert [(r["s"], r["lr"], r["iters"], r["success"]) for r in m.minimize_log[b]] == \
            [(s, lr, tr.iters, tr.success) for (_, _, s, lr, tr) in o.stages]
    # minimize calls per stage (a stage is a value of mu): the problems retry different stages
    per_stage = [[sum(1 for c in calls[b] if c[0] == mu) for mu in sorted({c[0] for c in calls[b]}, reverse=True)]
                 for b in range(2)]
    print("minimize calls per stage:", per_stage)
    assert all(len(p) == 3 for p in per_stage) and per_stage[0] != per_stage[1]


def test_fit_lambda1_grid_shares_one_centred_x():
    X = make_dataset(20, 400, seed=11)[0]
    X0 = X.copy()
    m = DagmaLinearBatch(batch_factory=OracleBatch, solver_factory=OracleSolver)
    lams = [0.01, 0.1]
    W = m.fit(X, lambda1=lams, **dict(FIT_ARGS, s=list(FIT_ARGS["s"])))
    assert W.shape == (2, 20, 20)
    assert np.array_equal(X, X0 - X0.mean(axis=0, keepdims=True))  # centred in place, once
    assert m.cov[0] is m.cov[1]
    for b, lam in enumerate(lams):
        o = LinearOracle("l2")
        assert np.array_equal(W[b], o.fit(X0.copy(), lambda1=lam, **dict(FIT_ARGS, s=list(FIT_ARGS["s"]))))
