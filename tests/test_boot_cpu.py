"""The bootstrap of `DagmaLinearBatch` without a device: the `midagma_boot_*` entries of the C ABI and
their argument checks, the resampling rule of `bootstrap_indices` against an independent restatement,
and `DagmaLinearBatch.bootstrap` against `LinearOracle.fit` on every resample through a CPU double of
`HipBatch`."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from midagma_amd import _lib
from midagma_amd.batch import DagmaLinearBatch, bootstrap_indices
from midagma_amd.simulate import make_dataset
from midagma_amd.solver import HipBatch
from oracle.dagma_oracle import LinearOracle
from tests import indep_numpy as inp
from tests.test_batch_cpu import FIT_ARGS, OracleBatch, OracleSolver, _DeviceTensor, _model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOOT_ENTRIES = ["midagma_boot_cov", "midagma_boot_get_cov", "midagma_boot_profile"]


def test_header_binding_and_library_agree_on_the_boot_entries():
    src = open(os.path.join(REPO, "include", "midagma_hip.h")).read()
    declared = sorted(n for n in set(re.findall(r"\b(midagma_[a-z_0-9]+)\s*\(", src)) if n.startswith("midagma_boot_"))
    assert declared == BOOT_ENTRIES
    assert sorted(n for n in _lib.EXPORTED if n.startswith("midagma_boot_")) == BOOT_ENTRIES
    L = _lib.load()
    for name in BOOT_ENTRIES:
        assert hasattr(L, name), name
    assert L.midagma_abi_version() == 11  # additive entries


def test_boot_entries_refuse_null_arguments_without_a_device():
    L = _lib.load()
    X = np.zeros((4, 3))
    out = np.zeros(9)
    xp = X.ctypes.data_as(C.c_void_p)
    assert L.midagma_boot_cov(None, xp, 4, 3, 0, 7, 0, 0) == _lib.E_ARG
    assert b"boot_cov" in L.midagma_batch_last_error(None)
    assert L.midagma_boot_cov(None, None, 4, 3, 0, 7, 0, 0) == _lib.E_ARG
    assert L.midagma_boot_get_cov(None, _lib.dptr(out)) == _lib.E_ARG
    assert b"boot_get_cov" in L.midagma_batch_last_error(None)
    assert L.midagma_boot_get_cov(None, None) == _lib.E_ARG
    assert L.midagma_boot_profile(None, None) == _lib.E_ARG


# ------------------------------------------------------------------ the resampling rule
def _indices_restated(seed, b, n):
    """The rule in Python integers over the test suite's own Philox."""
    j = np.arange(n)
    z = np.zeros(n, dtype=np.int64)
    o0, o1, _, _ = inp.philox4x32_10(j, z + b, z, z, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return [(((int(a) << 32) | int(c)) * n) >> 64 for a, c in zip(o0, o1)]


def test_bootstrap_indices_known_answer():
    idx = bootstrap_indices(7, 0, 1000)
    assert idx.dtype == np.int64 and idx.shape == (1000,)
    assert idx[:5].tolist() == [954, 406, 6, 390, 289]
    assert len(set(idx.tolist())) == 627


@pytest.mark.parametrize("seed", [7, 0x123456789ABCDEF0])
@pytest.mark.parametrize("n", [1, 2, 37, 1000])
@pytest.mark.parametrize("b", [0, 5])
def test_bootstrap_indices_match_the_restated_rule(seed, n, b):
    idx = bootstrap_indices(seed, b, n)
    assert idx.tolist() == _indices_restated(seed, b, n)
    assert idx.min() >= 0 and idx.max() < n


def test_bootstrap_indices_differ_between_replicates_and_seeds():
    a = bootstrap_indices(7, 0, 1000)
    assert not np.array_equal(a, bootstrap_indices(7, 1, 1000))
    assert not np.array_equal(a, bootstrap_indices(8, 0, 1000))
    assert np.array_equal(a, bootstrap_indices(7, 0, 1000))
    for bad in (0, 2**31):
        with pytest.raises(ValueError):
            bootstrap_indices(7, 0, bad)


# ------------------------------------------------------------------------- bootstrap
class OracleBootBatch(OracleBatch):
    """`OracleBatch` with `HipBatch.boot_cov` / `get_cov` as numpy states them: the resample
    gathered, centred, its Gram over n."""

    def boot_cov(self, X, seed, first=0, budget_bytes=None):
        n = X.shape[0]
        covs = []
        for b in range(self.B):
            Xb = X[bootstrap_indices(seed, first + b, n)]
            Xb = Xb - Xb.mean(axis=0, keepdims=True)
            covs.append(Xb.T @ Xb / float(n))
        self.cov = np.stack(covs)

    def get_cov(self):
        return self.cov.copy()


@pytest.mark.parametrize("data_seed", [11, 15])  # (the two that leave lockstep in test_batch_cpu.py)
def test_bootstrap_matches_the_oracle_fit_on_every_resample(data_seed):
    X = make_dataset(20, 400, seed=data_seed)[0]
    X0 = X.copy()
    n_boot, boot_seed = 3, 1234
    s_arg = list(FIT_ARGS["s"])
    m = DagmaLinearBatch(batch_factory=OracleBootBatch, solver_factory=OracleSolver)
    freq = m.bootstrap(X, n_boot, lambda1=0.03, seed=boot_seed, **dict(FIT_ARGS, s=s_arg))
    assert np.array_equal(X, X0) and s_arg == FIT_ARGS["s"]  # neither is touched
    assert m.W_boot.shape == (n_boot, 20, 20) and m.boot_seed == boot_seed
    assert m.fit_timing["cov_on"] == "device"
    calls = OracleBatch.last.calls
    for b in range(n_boot):
        o = LinearOracle("l2")
        W_ref = o.fit(X0[bootstrap_indices(boot_seed, b, 400)].copy(), lambda1=0.03,
                      **dict(FIT_ARGS, s=list(FIT_ARGS["s"])))
        assert np.array_equal(m.W_boot[b], W_ref), b
        assert calls[b] == [(mu, s, lr, tr.iters, tr.success) for (_, mu, s, lr, tr) in o.stages]
        assert m.h_final[b] == o.h_final and m.score_final[b] == o.score_final
        assert [(r["s"], r["lr"], r["iters"], r["success"]) for r in m.minimize_log[b]] == \
            [(s, lr, tr.iters, tr.success) for (_, _, s, lr, tr) in o.stages]
    print("minimize calls per replicate:", [len(c) for c in calls])
    assert freq is m.edge_freq and freq.shape == (20, 20)
    assert np.array_equal(freq, np.mean([(m.W_boot[b] != 0) for b in range(n_boot)], axis=0))
    assert 0.0 < freq.max() <= 1.0


def test_bootstrap_rejects_bad_arguments_before_any_backend():
    X = np.random.default_rng(0).standard_normal((50, 20))
    for n_boot in (0, HipBatch.MAX_B + 1):
        with pytest.raises(ValueError, match="n_boot"):
            _model().bootstrap(X, n_boot)
    with pytest.raises(ValueError, match="d <= 64"):
        _model().bootstrap(np.zeros((100, 65)), 4)
    with pytest.raises(ValueError, match="float64"):
        _model().bootstrap(X.astype(np.float32), 4)
    with pytest.raises(ValueError, match="lambda1"):
        _model().bootstrap(X, 4, lambda1=[0.01, 0.02, 0.03, 0.04])
    with pytest.raises(ValueError):
        _model().bootstrap([X, X], 4)
    with pytest.raises(TypeError):
        _model().bootstrap(X, 4, warm_iters=10)
    with pytest.raises(ValueError, match="device tensor"):  # fit itself keeps refusing one
        _model().fit(_DeviceTensor())
