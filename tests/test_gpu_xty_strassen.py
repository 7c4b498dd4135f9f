"""The data-mode X^T Y GEMM by one level of Strassen (csrc/gemm.hip, launch_xty_strassen): seven
half-size products in one launch, the X-side operand sums formed by set_data, the Y-side pairs in
the tile body's registers, one combine kernel.

- Score level: Z = X^T (X (I - W)) as step_partial leaves it in the bound score buffer, in the
  classical form (switch 1) and the Strassen form (switch 2), against a reference accurate to
  ~1e-19 (below).  W is dense with a different scale in each quadrant and X has column scales
  spread over e^+-1, so a swapped block, a wrong sign or a misplaced tile is an O(1) error.
  Bar: the Strassen form's max|dZ| / max|Z| is at most 8x the classical form's on the same inputs
  (a CPU experiment at n = 40000, d = 128 gave 1.5e-16 against 1.8e-16, ratio < 1; a wrong block
  is ~1e15 times that).
- Trajectories: 20 Adam steps (l2) against the oracle's data-mode steps to 1e-9, the bar of the
  other data-mode tests; 10 logistic steps, Strassen against classical, to 1e-9.
- Two Strassen runs are bit-identical; the size rule picks Strassen at D = 1024 with long shards
  and the classical form at D = 1152 and for short shards.

The reference: G = X^T X with every partial product exact (X cut per column into four 19-bit
integer slices, so a slice product summed over n <= 2^12 rows stays below 2^50 and float64 BLAS
adds it without rounding; 76 bits of every entry are kept), the sixteen slice products added in
np.longdouble, then Z = G (I - W) in np.longdouble.  Against the plain np.longdouble products it
differs by 1.2e-18 max|Z| at d = 256 (np.longdouble's own rounding over 2048 terms) and takes a
tenth of their time at d = 512.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle.dagma_oracle import LinearOracle  # noqa: E402

BITS, PARTS = 19, 4


def _slices(M):
    """M = scale * sum_k T_k 2^(-BITS (k + 1)) + O(2^(-BITS PARTS)), T_k integer-valued."""
    e = np.frexp(np.abs(M).max(axis=0))[1]
    R = np.ldexp(M, -e)            # |R| < 1, exact
    out = []
    for _ in range(PARTS):
        R = np.ldexp(R, BITS)
        T = np.trunc(R)
        out.append(T)
        R = R - T                  # exact: the fraction
    return out, np.ldexp(1.0, e).astype(np.longdouble)


def _gram_exact(X):
    assert X.shape[0] <= 4096      # slice products summed over the rows stay below 2^50
    T, scale = _slices(X)
    G = np.zeros((X.shape[1],) * 2, dtype=np.longdouble)
    for kl in range(2 * PARTS - 2, -1, -1):      # smallest terms first
        P = np.zeros_like(G)
        for k in range(PARTS):
            l = kl - k
            if 0 <= l < PARTS:
                P += (T[k].T @ T[l]).astype(np.longdouble)
        G += np.ldexp(P, -BITS * (kl + 2))
    return G * scale[:, None] * scale[None, :]


def _inputs(d, n, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)) * np.exp(rng.uniform(-1.0, 1.0, size=d))
    X -= X.mean(axis=0, keepdims=True)
    W = rng.standard_normal((d, d))
    h = d // 2
    for (i, j), sc in zip(((0, 0), (0, 1), (1, 0), (1, 1)), (0.01, 0.02, 0.03, 0.04)):
        W[i * h:(i + 1) * h, j * h:(j + 1) * h] *= sc
    np.fill_diagonal(W, 0.0)
    Zref = _gram_exact(X) @ (np.eye(d, dtype=np.longdouble) - W.astype(np.longdouble))
    return X, W, Zref


@pytest.fixture(scope="module")
def case256():
    return _inputs(256, 2048, seed=1)


@pytest.fixture(scope="module")
def case512():
    return _inputs(512, 3000, seed=2)


def _solver(X, form, split=None, loss="l2"):
    from midagma_amd.solver import HipSolver
    n, d = X.shape
    s = HipSolver(d, loss, "data", device=0)
    s.debug_xty_form(form, split)
    if loss == "logistic":
        s.set_cov(X.T @ X / n)
    s.set_data(X, n_global=n)
    return s


def _score_buffer(X, W, form, split=None):
    """Z as step_partial leaves it in the bound score buffer (D = d here)."""
    d = X.shape[1]
    s = _solver(X, form, split)
    assert s.D == d and s.xty_form == form == s.debug_xty_form()
    zt = torch.zeros(s.zbuf_len, dtype=torch.float64, device="cuda:0")
    s.bind_zbuf(zt.data_ptr(), zt.numel())
    s.begin(W, 1.0, 8, 1.0, 3e-4, tol=-1.0, lambda1=0.03)
    s.step_partial()
    s.sync()
    torch.cuda.synchronize()
    Z = zt[:d * d].cpu().numpy().reshape(d, d).copy()
    s.close()      # (before zt goes: the solver's graphs name it)
    return Z


def _err(Z, Zref):
    return float(np.abs(Z.astype(np.longdouble) - Zref).max() / np.abs(Zref).max())


def test_every_block_distinct(case256):
    """d = 256: one 128-tile per quadrant of every product, n = 2048."""
    X, W, Zref = case256
    e1 = _err(_score_buffer(X, W, 1), Zref)
    e2 = _err(_score_buffer(X, W, 2), Zref)
    print(f"d=256 n=2048: classical {e1:.3e}  strassen {e2:.3e}")
    assert e1 <= 1e-14               # the classical form itself is at rounding level
    assert e2 <= 8 * e1


@pytest.mark.parametrize("split", [0, 1])
def test_tile_map_ragged_rows(case512, split):
    """d = 512: four tiles per product; n = 3000 pads to 3072, the zero rows in the second half of
    the samples.  Split 0: the rule's (96 slices of one K tile here), split 1: one slice."""
    X, W, Zref = case512
    e1 = _err(_score_buffer(X, W, 1), Zref)
    e2 = _err(_score_buffer(X, W, 2, split), Zref)
    print(f"d=512 n=3000 split={split}: classical {e1:.3e}  strassen {e2:.3e}")
    assert e1 <= 1e-14
    assert e2 <= 8 * e1


def test_trajectory_l2_against_oracle(case256):
    X = case256[0]
    d, K = X.shape[1], 20
    o = LinearOracle("l2", score_mode="data")
    o.prepare(X.copy(), 0.03, 1000)
    Wr, tr = o.minimize(np.zeros((d, d)), 1.0, K, 1.0, 3e-4, tol=-1.0)
    s = _solver(o.X, 2)    # (the oracle's centred copy)
    assert s.xty_form == 2
    W = np.zeros((d, d))
    res = s.minimize(W, 1.0, K, 1.0, 3e-4, tol=-1.0, lambda1=0.03)
    s.close()
    assert res.iters == tr.iters == K and res.success
    print(f"l2 trajectory: max|dW| {np.abs(W - Wr).max():.3e}")
    assert np.abs(W - Wr).max() <= 1e-9


def test_trajectory_logistic_against_classical():
    rng = np.random.default_rng(5)
    X = (rng.uniform(size=(2048, 256)) < 0.3).astype(np.float64)
    out = {}
    for form in (1, 2):
        s = _solver(X, form, loss="logistic")
        assert s.xty_form == form
        W = np.zeros((256, 256))
        res = s.minimize(W, 1.0, 10, 1.0, 3e-4, tol=-1.0, lambda1=0.03)
        s.close()
        assert res.iters == 10 and res.success
        out[form] = W
    print(f"logistic trajectory: max|dW| {np.abs(out[2] - out[1]).max():.3e}")
    assert np.abs(out[1]).max() > 0
    assert np.abs(out[2] - out[1]).max() <= 1e-9


def test_two_runs_bit_identical(case256):
    X, W, _ = case256
    Za, Zb = _score_buffer(X, W, 2), _score_buffer(X, W, 2)
    assert np.array_equal(Za, Zb)
    runs = []
    for _ in range(2):
        s = _solver(X, 2)
        Wk = np.zeros_like(W)
        s.minimize(Wk, 1.0, 10, 1.0, 3e-4, tol=-1.0, lambda1=0.03)
        s.close()
        runs.append(Wk)
    assert np.array_equal(runs[0], runs[1])


@pytest.mark.parametrize("d,n,form", [(1000, 65536, 2), (1000, 32768, 1), (1100, 65536, 1)])
def test_size_rule(d, n, form):
    """The rule: D = 1024 with product K slices of 1024 rows (the threshold) picks Strassen; the
    same D with slices of 512 rows and D = 1152 (not a multiple of 256) stay classical."""
    from midagma_amd.solver import HipSolver
    g = torch.Generator(device="cuda:0").manual_seed(d + n)
    X = torch.randn(n, d, dtype=torch.float64, device="cuda:0", generator=g)
    s = HipSolver(d, "l2", "data", device=0)
    assert s.xty_form == 0
    s.set_data(X, n_global=n)
    assert s.xty_form == form
    if form == 2:   # and the long-shard score agrees with the classical form's
        W = np.zeros((d, d))
        W[0, 1] = 0.5
        s.score_partial(W)
        _, G2 = s.score_finish()
        s.debug_xty_form(1)
        s.set_data(X, n_global=n)
        assert s.xty_form == 1
        s.score_partial(W)
        _, G1 = s.score_finish()
        assert np.abs(G2 - G1).max() <= 1e-12 * np.abs(G1).max()
    s.close()
