"""Every cell of the FP64 GEMM dispatch (csrc/gemm.hip: launch_gemm's run-time (a_trans, bmode,
epi) -> template arguments, on both tiers) through the public HipSolver API, against numpy.

The shapes are the smallest that select each cell, so a swapped template argument cannot hide:

- D % 128 != 0 takes the 64 x 64 tile kernel (d = 50: D = 64, one tile; d = 150: D = 192, 3 x 3
  tiles), D % 128 == 0 the pipelined 128 x 128 tile kernel (d = 100: D = 128);
- at D = 128 the X (I - W) / sigmoid GEMM reads X^T (AMODE 1) or, with MIDAGMA_NO_XT set before
  set_data, X itself (AMODE 0);
- n = 1024 at d = 100 is 8 tiles, the smallest grid the serial split sigmoid (EPI_SIGMOID_SPLIT)
  accepts (tiles % 8 == 0);
- cov mode's score() multiplies the untransposed cov by I - W (B_IMINUS, AMODE 0) on either tier.

Tolerance: the project's score bar, 1e-10 relative on the loss and on max|G| (test_gpu_logistic's
_check_score).  numpy alone meets it between two summation orders at these shapes (X^T Y against
the same product summed in 64-row blocks: <= 2e-15 relative on every quantity checked here).
"""
import numpy as np
import pytest
from scipy.special import expit

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RTOL = 1e-10
SHAPES = [(50, 200), (150, 200), (100, 300)]


@pytest.fixture(scope="module")
def hip():
    from midagma_amd import _lib
    from midagma_amd.solver import device_count
    _lib.load()
    assert device_count() >= 1, "no ROCm device visible"
    return _lib


def _weights(d, seed=1):
    W = np.random.default_rng(seed).normal(scale=0.05, size=(d, d))
    np.fill_diagonal(W, 0.0)
    return W


def _centred(n, d):
    X = np.random.default_rng(100 * d + n).normal(size=(n, d))
    return X - X.mean(axis=0, keepdims=True)


def _binary(n, d):
    return (np.random.default_rng(100 * d + n).uniform(size=(n, d)) < 0.3).astype(np.float64)


def _data_solver(X, loss, form=None):
    from midagma_amd.solver import HipSolver
    n, d = X.shape
    s = HipSolver(d, loss, "data", device=0)
    if form is not None:
        s.debug_sig_split(form)
    s.set_cov(X.T @ X / n)
    s.set_data(X, n_global=n)
    return s


def _close(loss, G, ref_loss, ref_G):
    assert abs(loss - ref_loss) <= RTOL * abs(ref_loss), (loss, ref_loss)
    err = np.abs(G - ref_G).max()
    assert err <= RTOL * np.abs(ref_G).max(), (err, np.abs(ref_G).max())


def _check_l2(X):
    n, d = X.shape
    W = _weights(d)
    sol = _data_solver(X, "l2")
    sol.score_partial(W)
    loss, G = sol.score_finish()
    sol.close()
    diff = np.eye(d) - W
    rhs = (X.T @ X / n) @ diff
    _close(loss, G, 0.5 * np.trace(diff.T @ rhs), -rhs)


def _check_logistic(X, form):
    n, d = X.shape
    W = _weights(d)
    sol = _data_solver(X, "logistic", form)
    assert sol.debug_sig_split() == form
    sol.score_partial(W)
    loss, G = sol.score_finish()
    sol.close()
    Z = X @ W
    _close(loss, G, (np.logaddexp(0.0, Z) - X * Z).sum() / n, X.T @ expit(Z) / n - X.T @ X / n)


@pytest.mark.parametrize("d,n", SHAPES)
def test_l2_data_score(hip, d, n):
    """Y = X (I - W) (B_IMINUS), then X^T Y: 64-tile at D = 64 and 192, pipelined AMODE 1 at D = 128."""
    _check_l2(_centred(n, d))


def test_l2_data_score_without_xt(hip, monkeypatch):
    """D = 128 with X^T not kept: the pipelined kernel reads X row-major (AMODE 0, B_IMINUS)."""
    monkeypatch.setenv("MIDAGMA_NO_XT", "1")
    _check_l2(_centred(300, 100))


@pytest.mark.parametrize("d,n", SHAPES)
def test_logistic_score_one_pass(hip, d, n):
    """The one-pass sigmoid epilogue on both tiers (AMODE 1 at D = 128)."""
    _check_logistic(_binary(n, d), 1)


def test_logistic_score_one_pass_without_xt(hip, monkeypatch):
    monkeypatch.setenv("MIDAGMA_NO_XT", "1")
    _check_logistic(_binary(300, 100), 1)


@pytest.mark.parametrize("no_xt", [False, True])
def test_logistic_score_serial_split(hip, monkeypatch, no_xt):
    """EPI_SIGMOID_SPLIT at 8 tiles, reading X^T (AMODE 1) and X (AMODE 0)."""
    if no_xt:
        monkeypatch.setenv("MIDAGMA_NO_XT", "1")
    _check_logistic(_binary(1024, 100), 2)


@pytest.mark.parametrize("d", [100, 50])
def test_cov_score(hip, d):
    """cov mode score(): cov @ (I - W) with cov untransposed, pipelined at d = 100, 64-tile at d = 50."""
    from midagma_amd.solver import HipSolver
    X = _centred(4 * d, d)
    cov = X.T @ X / X.shape[0]
    W = _weights(d)
    s = HipSolver(d, "l2", "cov", device=0)
    s.set_cov(cov)
    loss, G = s.score_value(W)
    s.close()
    diff = np.eye(d) - W
    rhs = cov @ diff
    _close(loss, G, 0.5 * np.trace(diff.T @ rhs), -rhs)


def test_data_gram(hip):
    """data_gram(): X^T X through the X^T Y GEMM's description with Y = X (pipelined, AMODE 1)."""
    X = _centred(300, 100)
    s = _data_solver(X, "l2")
    s.data_gram()
    s.cov_from_zbuf(1.0)
    G = s.get_cov()
    s.close()
    ref = X.T @ X
    assert np.abs(G - ref).max() <= RTOL * np.abs(ref).max()
