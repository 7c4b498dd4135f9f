"""The PST trek regularizer of `DagmaLinearBatch` without a device: what the constructor accepts and
refuses, the argument checks of `fit` / `bootstrap`, the regularizer's way from the constructor to
`HipBatch.set_trek` and the schedule against `LinearOracle.fit` with its `trek` set, through CPU
doubles of `HipBatch` / `HipSolver`; and the two `midagma_btrek_*` entries of the C ABI."""
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
from oracle.trek_oracle import pst_value_grad

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BTREK_ENTRIES = ["midagma_btrek_set", "midagma_btrek_value"]
D = 20
PAIRS = np.array(np.triu_indices(D, 1)).T[::3]


def test_header_binding_and_library_agree_on_the_btrek_entries():
    src = open(os.path.join(REPO, "include", "midagma_hip.h")).read()
    declared = sorted(n for n in set(re.findall(r"\b(midagma_[a-z_0-9]+)\s*\(", src)) if n.startswith("midagma_btrek_"))
    assert declared == BTREK_ENTRIES
    assert sorted(n for n in _lib.EXPORTED if n.startswith("midagma_btrek_")) == BTREK_ENTRIES
    L = _lib.load()
    for name in BTREK_ENTRIES:
        assert hasattr(L, name), name
    assert L.midagma_abi_version() == 11  # additive entries


def test_btrek_entries_refuse_null_arguments_without_a_device():
    L = _lib.load()
    w = np.ones(2)
    P = np.array([[0, 1]], dtype=np.int64)
    pp = P.ctypes.data_as(C.POINTER(C.c_int64))
    assert L.midagma_btrek_set(None, 0, 0, 2, _lib.dptr(w), 1e-8, pp, 1) == _lib.E_ARG
    assert b"btrek_set" in L.midagma_batch_last_error(None)
    assert L.midagma_btrek_set(None, 0, 0, 2, None, 1e-8, None, 0) == _lib.E_ARG
    out = np.zeros(2)
    assert L.midagma_btrek_value(None, _lib.dptr(np.zeros((2, 3, 3))), _lib.dptr(out), None) == _lib.E_ARG
    assert b"btrek_value" in L.midagma_batch_last_error(None)
    assert L.midagma_btrek_value(None, None, None, None) == _lib.E_ARG


def _reg(name="pst", seq="exp", mode="opt", weight=0.1, pairs=PAIRS, enabled=True, **kwargs):
    return SimpleNamespace(name=name, mode=mode, weight=weight, cfg={"I": pairs, "seq": seq, "kwargs": kwargs},
                           enabled=lambda: enabled)


def _no_backend(*a, **k):
    raise AssertionError("a backend was created before the arguments were checked")


def _model(**kw):
    return DagmaLinearBatch(batch_factory=_no_backend, solver_factory=_no_backend, **kw)


@pytest.mark.parametrize("seq", ["exp", "inv", " EXP "])
def test_constructor_accepts_pst(seq):
    m = _model(trek_reg=_reg(seq=seq, agg="lse", eps_inv=1e-6))
    assert m._trek["seq"] == seq.lower().strip() and m._trek["agg"] == "lse" and m._trek["eps_inv"] == 1e-6
    assert m._trek["mode"] == "opt" and m._trek["weight"] == 0.1 and np.array_equal(m._trek["pairs"], PAIRS)


@pytest.mark.parametrize("reg", [_reg(seq="log"), _reg(seq="binom"), _reg(K_log=5), _reg(name="nope"),
                                 _reg(name="tcc")], ids=["log", "binom", "K_log", "unknown", "tcc"])
def test_constructor_refuses_what_the_batch_does_not_run(reg):
    with pytest.raises(ValueError):
        _model(trek_reg=reg)


@pytest.mark.parametrize("reg", [_reg(enabled=False), _reg(name="tcc", enabled=False), _reg(pairs=[]),
                                 _reg(pairs=None), None], ids=["disabled", "disabled-tcc", "empty", "no-I", "none"])
def test_constructor_treats_disabled_or_empty_as_none(reg):
    assert _model(trek_reg=reg)._trek is None


def test_arguments_are_checked_before_any_backend_exists():
    X33 = np.zeros((50, 33))
    with pytest.raises(ValueError, match="d <= 32"):
        _model(trek_reg=_reg()).fit([X33])
    with pytest.raises(ValueError, match="d <= 32"):
        _model(trek_reg=_reg()).bootstrap(X33, n_boot=4)
    X = np.random.default_rng(0).standard_normal((50, D))
    with pytest.raises(ValueError, match="trek_weight"):
        _model(trek_reg=_reg()).fit(X.copy(), lambda1=[0.01, 0.02, 0.03], trek_weight=[0.1, 0.2])
    with pytest.raises(ValueError, match="trek_weight"):
        _model(trek_reg=_reg()).fit([X.copy(), X.copy()], trek_weight=[0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="trek_weight"):
        _model().fit([X.copy()], trek_weight=0.1)  # (no regularizer to weigh)
    with pytest.raises(ValueError, match="scalar trek_weight"):
        _model(trek_reg=_reg()).bootstrap(X, n_boot=4, trek_weight=[0.1, 0.2, 0.3, 0.4])


FIT_ARGS = dict(T=3, s=[1.0, .9, .8], warm_iter=300, max_iter=500, lr=0.3, checkpoint=100)


class OracleBatch:
    """`HipBatch`'s interface over `LinearOracle.minimize` with its `trek`, one problem after the other."""

    def __init__(self, d, B, device=0):
        self.d, self.B = d, B
        self.calls = [[] for _ in range(B)]
        self.trek_calls, self.events = [], []
        self.trek = None
        OracleBatch.last = self

    def set_cov(self, cov):
        self.cov = np.array(cov)
        self.events.append("set_cov")

    def boot_cov(self, X, seed):
        Xc = X - X.mean(axis=0, keepdims=True)
        self.cov = np.stack([Xc.T @ Xc / float(len(X))] * self.B)
        self.events.append("boot_cov")

    def get_cov(self):
        return self.cov

    def set_masks(self, mask_inc, mask_exc):
        assert mask_inc is None and mask_exc is None

    def set_trek(self, pairs, seq="exp", *, agg="mean", mode="opt", weight=0.0, eps_inv=1e-8):
        self.trek = dict(pairs=np.array(pairs), seq=seq, agg=agg, mode=mode, eps_inv=eps_inv)
        self.weight = list(np.broadcast_to(np.asarray(weight, dtype=np.float64), (self.B,)))
        self.trek_calls.append((seq, agg, mode, list(self.weight), eps_inv))
        self.events.append("set_trek")

    def trek_value(self, W, grad=True):
        assert not grad
        return np.array([pst_value_grad(W[b], self.trek["pairs"], self.trek["seq"], agg=self.trek["agg"],
                                        eps_inv=self.trek["eps_inv"], grad=False)[0] for b in range(self.B)]), None

    def minimize(self, W, mu, s, lr, lambda1, max_iter, tol=1e-6, beta_1=.99, beta_2=.999, checkpoint=1000,
                 active=None, want_checkpoints=False):
        if "minimize" not in self.events:
            self.events.append("minimize")
        out = [None] * self.B
        for b in range(self.B):
            if active is not None and not active[b]:
                continue
            o = LinearOracle("l2")
            o.cov, o.lambda1, o.checkpoint, o.d = self.cov[b], lambda1[b], checkpoint, self.d
            o.eye, o.exc, o.inc, o.X = np.eye(self.d), None, None, None  # (cov mode: X is not read)
            if self.trek is not None:
                o.trek = dict(self.trek, weight=self.weight[b])
            _, tr = o.minimize(W[b], mu, max_iter, s[b], lr[b], tol=tol, beta_1=beta_1, beta_2=beta_2)
            self.calls[b].append((mu, s[b], lr[b], tr.iters, tr.success))
            out[b] = SimpleNamespace(iters=tr.iters, success=tr.success, early_stop=tr.early_stop,
                                     halvings=tr.halvings, status=_lib.ST_DONE if tr.success else _lib.ST_FAILED)
        return out

    def close(self):
        self.events.append("close")


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


def _doubles(**kw):
    return DagmaLinearBatch(batch_factory=OracleBatch, solver_factory=OracleSolver, **kw)


@pytest.mark.parametrize("seq", ["exp", "inv"])
def test_fit_with_pst_matches_the_oracle_fit_per_problem(seq):
    """Two d = 20 problems with their own weights: W, the (mu, s, lr, iters, success) sequence and
    trek_final equal `LinearOracle.fit` with `o.trek` on each problem alone."""
    Xs = [make_dataset(D, 400, seed=sd)[0] for sd in (11, 15)]
    weights = [0.2, 1.5]
    m = _doubles(trek_reg=_reg(seq=seq, weight=99.0, agg="sum"))
    # (w_threshold = 0: the returned W is the unthresholded one, at which trek_final is taken)
    W = m.fit([X.copy() for X in Xs], lambda1=0.03, trek_weight=weights, w_threshold=0.0,
              **dict(FIT_ARGS, s=list(FIT_ARGS["s"])))
    bt = OracleBatch.last
    assert bt.events == ["set_cov", "set_trek", "minimize", "close"]  # installed once, before the stages
    assert bt.trek_calls == [(seq, "sum", "opt", weights, 1e-8)]
    assert m.trek_final.shape == (2,)
    for b, X in enumerate(Xs):
        o = LinearOracle("l2")
        o.trek = dict(pairs=PAIRS, seq=seq, agg="sum", mode="opt", weight=weights[b], eps_inv=1e-8)
        W_ref = o.fit(X.copy(), lambda1=0.03, w_threshold=0.0, **dict(FIT_ARGS, s=list(FIT_ARGS["s"])))
        assert bt.calls[b] == [(mu, s, lr, tr.iters, tr.success) for (_, mu, s, lr, tr) in o.stages]
        assert np.array_equal(W[b], W_ref)
        assert m.trek_final[b] == pst_value_grad(W_ref, PAIRS, seq, agg="sum", grad=False)[0] > 0.0
    # the regularizer is felt: the same data without it ends elsewhere
    W_plain = _doubles().fit([X.copy() for X in Xs], lambda1=0.03, w_threshold=0.0,
                             **dict(FIT_ARGS, s=list(FIT_ARGS["s"])))
    assert not np.array_equal(W, W_plain)


GRID_ARGS = dict(T=2, s=[1.0, .9], warm_iter=100, max_iter=150, lr=0.3, checkpoint=50)


def test_trek_weight_grid_on_one_x():
    """(Short stages: what is checked is how X, lambda1 and the weights reach the batch.)"""
    X = make_dataset(D, 400, seed=11)[0]
    X0 = X.copy()
    weights = [0.0, 0.5, 2.0]
    m = _doubles(trek_reg=_reg())
    W = m.fit(X, trek_weight=weights, **GRID_ARGS)
    assert W.shape == (3, D, D)
    assert np.array_equal(X, X0 - X0.mean(axis=0, keepdims=True))  # centred in place, once
    assert m.cov[0] is m.cov[1] is m.cov[2]
    assert OracleBatch.last.trek_calls == [("exp", "mean", "opt", weights, 1e-8)]
    plain = _doubles().fit(X0.copy(), **GRID_ARGS)
    assert np.array_equal(W[0], plain[0]) and not np.array_equal(W[2], plain[0])  # weight 0 adds + 0.0 * grad
    # a lambda1 grid of the same length pairs up with the weights; a scalar weight is shared
    m.fit(X0.copy(), lambda1=[0.01, 0.02, 0.03], trek_weight=weights, **GRID_ARGS)
    assert OracleBatch.last.B == 3
    m.fit(X0.copy(), lambda1=[0.01, 0.02], trek_weight=0.25, **GRID_ARGS)
    assert OracleBatch.last.trek_calls == [("exp", "mean", "opt", [0.25, 0.25], 1e-8)]
    m.fit(X0.copy(), lambda1=[0.01, 0.02], **GRID_ARGS)
    assert OracleBatch.last.trek_calls == [("exp", "mean", "opt", [0.1, 0.1], 1e-8)]  # the regularizer's own


def test_bootstrap_installs_the_regularizer():
    X = make_dataset(D, 400, seed=11)[0]
    m = _doubles(trek_reg=_reg(seq="inv", mode="log", eps_inv=1e-6))
    freq = m.bootstrap(X, n_boot=2, trek_weight=0.7, **dict(FIT_ARGS, s=list(FIT_ARGS["s"])))
    bt = OracleBatch.last
    assert freq.shape == (D, D) and m.trek_final.shape == (2,) and np.all(m.trek_final > 0.0)
    assert bt.events == ["boot_cov", "set_trek", "minimize", "close"]
    assert bt.trek_calls == [("inv", "mean", "log", [0.7, 0.7], 1e-6)]
    m = _doubles()
    m.bootstrap(X, n_boot=2, **dict(FIT_ARGS, s=list(FIT_ARGS["s"])))
    assert OracleBatch.last.trek_calls == [] and np.array_equal(m.trek_final, np.zeros(2))
