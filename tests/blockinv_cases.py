"""The ill-conditioned matrix family and the inverse checker of the blocked-inverse tests
(tests/test_gpu_blockinv.py on the GPU, tests/test_blockinv_cases_cpu.py for the premises).

The W of the existing trajectories is near 0 (A = sI - W∘W ≈ I), where a wrong panel, trailing
tile or series pass moves nothing a test looks at.  make_W gives a W like the late part of a fit:
a weighted ER DAG (|w| in [0.5, 2] times `scale`) plus dense noise, so rho(W∘W) is 0.2 / 0.6 /
0.9 and cond_1(A) 1e1 / 5e2 / 3e4 for scale 0.3 / 0.6 / 0.8, still inside the M-matrix domain
(every entry of inv(A) positive).  Plain numpy / scipy, no GPU.
"""
import numpy as np
import scipy.linalg as sla

from midagma_amd import utils
from midagma_amd.simulate import make_dataset
from oracle.dagma_oracle import LinearOracle

# (scale, lr) of the slot tests: whole-matrix warm-start residuals far under the 0.25 gate
FAST_BANDS = ((0.3, 3e-4), (0.6, 3e-4), (0.8, 3e-6))
# A series pass squares the residual and a block is done once it is <= 1e-8 (nm_series.h), so a slot
# of p passes needs a warm start within 1e-8^(1/2^(p-1)): 1e-4 for the two passes every call starts
# with, 1e-2 for three.  The fast bands' first warm slot (residual 2e-3 .. 5e-2, from P(k-1) alone)
# therefore hands back once, by arithmetic; NEAR_BAND's (<= 2.5e-5) must converge in two passes.
NEAR_BAND = (0.6, 1e-7)
FAR_BAND = (0.8, 3e-4)     # first-slot residual ~1.8: the first warm slot must hand back
SEARCH_BAND = (0.8, 3e-2)  # the oracle's domain line search halves lr within 12 steps
# measured on the CPU with seed = d, s = 1: scale -> (rho(W∘W), cond_1(A)) at d = 100, 300
TABLE = {0.3: {100: (0.20, 8.0), 300: (0.21, 11.0)},
         0.6: {100: (0.56, 2e2), 300: (0.59, 5e2)},
         0.8: {100: (0.88, 6e3), 300: (0.94, 3e4)}}
RATIO_BAR = 8.0       # residual and forward error against LAPACK's own (see check_inverse)
FORWARD_MAX_D = 300   # the longdouble reference is O(d^3) without BLAS


def make_W(d, scale, seed, noise=0.3):
    utils.set_random_seed(seed)
    B = utils.simulate_dag(d, 2 * d, "ER")
    W = utils.simulate_parameter(B) * scale
    W += np.random.default_rng(seed).uniform(-1, 1, (d, d)) * noise / np.sqrt(d)
    np.fill_diagonal(W, 0)
    return W


def make_oracle(d, n=None, seed=None, checkpoint=1000, score_mode="cov"):
    """The covariance (and centred X) of the slot tests: make_dataset(d, 2d, seed=d)."""
    X, _, _ = make_dataset(d, 2 * d if n is None else n, seed=d if seed is None else seed)
    o = LinearOracle("l2", score_mode)
    o.prepare(X.copy(), 0.03, checkpoint)
    return o


def a_matrix(W, s=1.0):
    return s * np.eye(W.shape[0]) - W * W


def two_sided_residual(A, M):
    """max(max|I - A M|, max|I - M A|) in float64."""
    I = np.eye(A.shape[0])
    return max(float(np.abs(I - A @ M).max()), float(np.abs(I - M @ A).max()))


def refined_inverse(A, X0):
    """LAPACK's inverse refined by two Newton steps X += X (I - A X) in np.longdouble, with its own
    longdouble residual asserted <= 1e-17 max|X| (measured 1.2e-18 after one step at d = 300,
    scale 0.6).  The residual I - A X and the sum are longdouble; the correction's product X R runs
    in float64 (R is ~1e-15 and smaller, so its rounding is ~1e-31 of X), which saves two of the
    five BLAS-less longdouble products."""
    assert np.finfo(np.longdouble).eps < 2e-19, "np.longdouble is not the 80-bit extended type here"
    Al = A.astype(np.longdouble)
    X = X0.astype(np.longdouble)
    I = np.eye(A.shape[0], dtype=np.longdouble)
    for _ in range(2):
        R = I - Al @ X
        X = X + (X.astype(np.float64) @ R.astype(np.float64)).astype(np.longdouble)
    res = float(np.abs(I - Al @ X).max())
    assert res <= 1e-17 * float(np.abs(X).max()), res
    return X


def check_inverse(W, Mt, s=1.0, forward=None):
    """Mt against inv(sI - W∘W)^T.  Residual at every d: r = max(max|I - A M|, max|I - M A|) must be
    <= 8 r_ref, r_ref the same quantity of scipy.linalg.inv(A).  Forward error (d <= 300 unless
    `forward` says otherwise): max|M - X| <= 8 max(max|inv(A) - X|, 2^-50 max|X|) against the
    longdouble-refined X; the 2^-50 floor guards against a luckily exact LAPACK result.  The 8:
    unpivoted 32-block Gauss-Jordan in numpy needs 1.6x on this family, the other factor of 5 is
    allowance for MFMA accumulation order and the product-form series.  Returns the two ratios
    (residual, forward or None); a ratio above 8 is a finding, not a reason to raise the bar."""
    d = W.shape[0]
    assert Mt.shape == (d, d) and np.isfinite(Mt).all()
    A = a_matrix(W, s)
    M = Mt.T
    Mref = sla.inv(A)
    r, r_ref = two_sided_residual(A, M), two_sided_residual(A, Mref)
    res_ratio = r / r_ref
    fwd_ratio = None
    if forward if forward is not None else d <= FORWARD_MAX_D:
        X = refined_inverse(A, Mref)
        e_ref = max(float(np.abs(Mref - X).max()), 2.0 ** -50 * float(np.abs(X).max()))
        e = float(np.abs(M - X).max())
        fwd_ratio = e / e_ref
        assert e <= RATIO_BAR * e_ref, f"forward error {e:.3e} > 8 x {e_ref:.3e} (ratio {fwd_ratio:.2f})"
    assert r <= RATIO_BAR * r_ref, f"residual {r:.3e} > 8 x LAPACK's {r_ref:.3e} (ratio {res_ratio:.2f})"
    return res_ratio, fwd_ratio


def block_gj_inverse(A, nb=32):
    """Numpy stand-in for the flat kernel's algorithm: in-place Gauss-Jordan over nb-wide diagonal
    blocks without pivoting between blocks (each diagonal block by LAPACK)."""
    A = A.copy()
    d = A.shape[0]
    for k0 in range(0, d, nb):
        k1 = min(k0 + nb, d)
        P = sla.inv(A[k0:k1, k0:k1])
        rest = np.r_[0:k0, k1:d]
        R = P @ A[k0:k1][:, rest]
        Cc = A[rest][:, k0:k1]
        A[np.ix_(rest, rest)] -= Cc @ R
        A[k0:k1, rest] = R
        A[rest, k0:k1] = -Cc @ P
        A[k0:k1, k0:k1] = P
    return A


def inf_norm(R):
    return float(np.abs(R).sum(axis=1).max())


def warm_start_residuals(o, W0, lr, s=1.0):
    """The oracle's first two steps from W0: (||I - A(W1) M(W0)||_inf, ||I - A(W2)(2 M1 - M0)||_inf),
    the whole-matrix residuals of the first warm slot and of the first extrapolated start."""
    d = W0.shape[0]
    I = np.eye(d)
    W1, _ = o.minimize(W0.copy(), 1.0, 1, s, lr, tol=-1.0)
    W2, _ = o.minimize(W0.copy(), 1.0, 2, s, lr, tol=-1.0)
    M0, M1 = sla.inv(a_matrix(W0, s)), sla.inv(a_matrix(W1, s))
    return inf_norm(I - a_matrix(W1, s) @ M0), inf_norm(I - a_matrix(W2, s) @ (2 * M1 - M0))
