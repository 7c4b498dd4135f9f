"""The ill-conditioned matrix family and the inverse checker of the blocked-inverse tests
(tests/test_gpu_blockinv.py on the GPU, tests/test_blockinv_cases_cpu.py for the premises).

The W of the existing trajectories is near 0 (A = sI - W∘W ≈ I), where a wrong panel, trailing
tile or series pass moves nothing a test looks at.  make_W gives a W like the late part of a fit:
a weighted ER DAG (|w| in [0.5, 2] times `scale`) plus dense noise, so rho(W∘W) is 0.2 / 0.6 /
0.9 and cond_1(A) 1e1 / 5e2 / 3e4 for scale 0.3 / 0.6 / 0.8, still inside the M-matrix domain
(every entry of inv(A) positive).  Plain numpy / scipy, no GPU.

The second half holds the cells of the same family at d <= 64 for the one-workgroup loop
(tests/test_gpu_small_inverse.py, tests/test_small_cases_cpu.py).
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


# ---------------------------------------------------------------------------------------------
# The one-workgroup small-d loop (small.hip, d <= 64): tests/test_gpu_small_inverse.py on the GPU,
# tests/test_small_cases_cpu.py for the premises.  A warm slot there computes R = I - A^T X0 from
# X0 = P(k-1) (the first warm slot, and the slot after a halving) or 2 P(k-1) - P(k-2), and takes
# its form from g = d max|R|: two series passes (g <= 1e-4), three (g <= 1e-2), else Gauss-Jordan;
# and Gauss-Jordan whatever g when max|X0| > 512 (the one-sided series' other residual, Y S - I, is
# amplified by |inv(S)||S|: in numpy 3 - 5x LAPACK's up to max|inv| ~ 100, 10 - 19x on some slots at
# 546 - 1213; small.hip's comment says why 512).
SMALL_GATE_GJ, SMALL_GATE_THREE, SMALL_GATE_XMAX = 1e-2, 1e-4, 512.0
SMALL_MARGIN = 3.0                       # every slot's g is this factor away from both of its gates
# max|X0| needs no such factor: g is a difference of nearly equal terms and moves with the device's
# own inverses, max|X0| is the largest entry of an inverse the device holds to 1e-10 relative (the
# forward bar of the slot before).  5 % is room to spare; every product-form cell is below 100.
SMALL_XMAX_MARGIN = 1.05
SMALL_DS = {16: (5, 16), 32: (17, 20, 32), 64: (33, 48, 64)}   # small_block(d) -> the d of the slot tests
# band -> (scale of make_W, lr).  g is d max|R|, a bound on ||R||_inf that the make_W family (a
# sparse DAG plus noise) stays 10 - 100x under: there two passes would do wherever three are taken
# and three wherever the loop falls back, so the four bands of make_W alone cannot tell a wrong gate
# or a skipped third pass from a right one.  The last two bands are the cells in which the form is
# needed (tests/test_small_cases_cpu.py checks both claims with the series in numpy):
#   wide  : g of the first warm slot ~0.8, just under 1: three passes from it leave ||R||^8 far above
#           rounding, the fall-back at 1e-2 is what saves the slot
#   dense : W0 = small_dense_W, every off-diagonal entry of one magnitude, rho(W o W) as listed; R of
#           the first warm slot is then a near rank-one dense matrix whose norm is ~g = 3e-3, and two
#           passes leave ||R||^4 ~ 1e-10, 300 - 8000x LAPACK's error
#   steep : only at SMALL_STEEP's d, one per DS: max|inv| 550 - 1200 (cond_1 2e4 - 8e4) at an lr so small
#           that g alone says three passes, then two: the max|X0| gate is the only reason for the
#           fall-back, and the series in numpy misses the checker there on some slots (10 - 19x) while
#           passing others (3 - 5x)
SMALL_BANDS = {"near": (0.6, 1e-7), "C": (0.8, 3e-6), "B": (0.6, 3e-4), "far": (0.8, 3e-4), "wide": (0.6, None),
               "dense": (None, None), "steep": (None, None)}
SMALL_STEEP = {16: (0.9, 1.1e-7), 32: (0.8, 6.7e-8), 64: (1.0, 2e-8)}   # d -> (scale, lr)
# lr of the cells whose g lies within the margin of a gate at the band's own lr (g of the first warm
# slot is linear in lr, of the extrapolated ones quadratic)
SMALL_LR = {(32, "near"): 5e-8,
            (16, "C"): 2e-6, (32, "C"): 4e-6, (48, "C"): 2e-6, (64, "C"): 1e-6,
            (5, "B"): 1.5e-4, (16, "B"): 6e-4, (17, "B"): 6e-4, (20, "B"): 6e-4,
            (5, "far"): 1e-3, (16, "far"): 1.5e-4, (48, "far"): 1e-4, (64, "far"): 1.5e-4,
            (5, "wide"): 0.046, (16, "wide"): 0.0054, (17, "wide"): 0.0069, (20, "wide"): 0.0063,
            (32, "wide"): 0.002, (33, "wide"): 0.019, (48, "wide"): 0.0029, (64, "wide"): 0.003,
            (5, "dense"): 7.7e-5, (16, "dense"): 4.6e-5, (17, "dense"): 3.9e-5, (20, "dense"): 3.6e-5,
            (32, "dense"): 1.6e-5, (33, "dense"): 3.9e-5, (48, "dense"): 2.7e-5, (64, "dense"): 1.5e-4}
SMALL_SCALE = {(33, "wide"): 0.3}        # (at scale 0.6 three passes from g = 0.8 still pass at d = 33)
SMALL_DENSE_RHO = {5: 0.9, 16: 0.9, 17: 0.9, 20: 0.9, 32: 0.95, 33: 0.9, 48: 0.9, 64: 0.5}
# the forms iterations 2..5 of every cell must take: '2' / '3' passes, 'G' the Gauss-Jordan fall-back
SMALL_FORMS = {"near": "2222", "C": "3222", "B": "G333", "far": "G333", "wide": "GGGG", "dense": "3222",
               "steep": "GGGG",
               (5, "B"): "3222", (32, "far"): "GGGG", (64, "dense"): "3333",
               # cond_1 3.4e4, max|X0| ~669: g alone would say "G333" (g(3..5) = 4.3e-4); without the
               # max|X0| gate the three-pass slots measured 3.6 / 5.2 / 8.75 of the residual bar 8
               (32, "C"): "GGGG"}
SMALL_SEARCH = (0.8, 0.3)                # the oracle's domain line search halves within 12 steps
SMALL_SEARCH_HALVINGS = {7: 1, 12: 2, 16: 2, 20: 3, 32: 4, 40: 3, 48: 4, 64: 4}


def small_oracle(d):
    return make_oracle(d, n=max(200, 10 * d))


def small_dense_W(d, rho, seed):
    """Every off-diagonal entry +-sqrt(rho / (d - 1)): W o W = rho / (d - 1) (J - I), of spectral radius
    rho, inv(I - W o W) dense and positive."""
    sign = np.where(np.random.default_rng(seed).uniform(size=(d, d)) < 0.5, -1.0, 1.0)
    W = np.sqrt(rho / (d - 1)) * sign
    np.fill_diagonal(W, 0)
    return W


def small_cells(bands=None):
    """(d, band) of every cell of the small-d slot tests."""
    return [(d, band) for ds in SMALL_DS.values() for d in ds for band in SMALL_BANDS
            if (bands is None or band in bands) and (band != "steep" or d in SMALL_STEEP)]


def small_cell(d, band):
    """(W0, lr, forms) of a cell."""
    scale, lr = SMALL_STEEP[d] if band == "steep" else SMALL_BANDS[band]
    W0 = small_dense_W(d, SMALL_DENSE_RHO[d], d) if band == "dense" else make_W(d, SMALL_SCALE.get((d, band), scale), d)
    return W0, SMALL_LR.get((d, band), lr), SMALL_FORMS.get((d, band), SMALL_FORMS[band])


def small_form(g, xmax):
    """The form a warm slot of gate quantity g and max|X0| = xmax takes, or None within SMALL_MARGIN
    of a gate."""
    if xmax >= SMALL_GATE_XMAX * SMALL_XMAX_MARGIN or g >= SMALL_GATE_GJ * SMALL_MARGIN:
        return "G"
    if xmax > SMALL_GATE_XMAX / SMALL_XMAX_MARGIN:
        return None
    if g <= SMALL_GATE_THREE / SMALL_MARGIN:
        return "2"
    if SMALL_GATE_THREE * SMALL_MARGIN <= g <= SMALL_GATE_GJ / SMALL_MARGIN:
        return "3"
    if g >= SMALL_GATE_GJ * SMALL_MARGIN:
        return "G"
    return None


def small_warm_starts(o, W0, lr, n_iter=5, s=1.0):
    """The oracle's first n_iter steps from W0: for iterations k = 2..n_iter the W the slot starts
    from and the kernel's warm start X0 (P(k-1) at k = 2, 2 P(k-1) - P(k-2) after), P LAPACK's
    inverses of the A before; no checkpoint among them."""
    o.checkpoint = 1000
    _, tr = o.minimize(W0.copy(), 1.0, n_iter, s, lr, tol=-1.0, snap_at=tuple(range(1, n_iter)))
    assert tr.iters == n_iter and tr.halvings == 0
    Ws = [W0] + [tr.snaps[k] for k in range(1, n_iter)]
    P = [sla.inv(a_matrix(W, s)) for W in Ws]
    return [(Ws[k - 1], P[k - 2] if k == 2 else 2 * P[k - 2] - P[k - 3]) for k in range(2, n_iter + 1)]


def small_gate(W, X0, s=1.0):
    """g = d max|I - A(W)^T X0^T| (the kernel holds the transposes; max| | is the same)."""
    d = W.shape[0]
    return d * float(np.abs(np.eye(d) - X0 @ a_matrix(W, s)).max())


def product_form_inverse(W, X0, passes, s=1.0):
    """The kernel's series in numpy, on the transposes as the kernel holds them: S = A^T,
    R = I - S X0^T, Y = X0^T (I + R)(I + R^2)[(I + R^4)]; returns Y = Mt."""
    S, Y = a_matrix(W, s).T, X0.T.copy()
    R = np.eye(W.shape[0]) - S @ Y
    for _ in range(passes):
        Y = Y + Y @ R
        R = R @ R
    return Y


def small_slot_gates(o, W0, lr, s, steps=12):
    """The kernel's slot sequence over o.minimize, halvings included (every inverse the oracle takes
    is one slot, in order): for each warm slot (is it the slot after a halving, g, max|X0|), with
    LAPACK's inverses as P and the kernel's rule for the warm count: +1 per slot up to 2, back to 1
    on a slot that halves."""
    Ws, inv = [], o._inv
    o._inv = lambda W, s_: (Ws.append(W.copy()), inv(W, s_))[1]
    o.checkpoint = 1000
    try:
        o.minimize(W0.copy(), 1.0, steps, s, lr, tol=-1.0)
    finally:
        del o._inv
    out, warm, p1, p2, after = [], 0, None, None, False
    for W in Ws:
        P = sla.inv(a_matrix(W, s))
        if warm > 0:
            X0 = 2 * p1 - p2 if warm >= 2 else p1
            out.append((after, small_gate(W, X0, s), float(np.abs(X0).max())))
        p1, p2, warm = P, p1, min(warm + 1, 2)
        after = bool((P + 1e-16 < 0).any())
        if after:
            warm = 1
    return out


def domain_decisions(o, W0, lr, s, steps=12, noise_seed=None):
    """o.minimize over `steps` from W0, recording for every inverse the loop tests the margin of its
    domain decision, |min(M + 1e-16)| / max|M|.  noise_seed: 1e-16 relative noise in every inverse
    (the oracle's inv_hook, as the parity envelopes use it).  Returns (W, trace, margins)."""
    margins = []
    rng = None if noise_seed is None else np.random.default_rng(noise_seed)

    def hook(M):
        if rng is not None:
            M = M * (1.0 + 1e-16 * rng.standard_normal(M.shape))
        margins.append(abs(float((M + 1e-16).min())) / float(np.abs(M).max()))
        return M

    o.checkpoint, o.inv_hook = 1000, hook
    try:
        W, tr = o.minimize(W0.copy(), 1.0, steps, s, lr, tol=-1.0)
    finally:
        o.inv_hook = None
    return W, tr, margins


def warm_start_residuals(o, W0, lr, s=1.0):
    """The oracle's first two steps from W0: (||I - A(W1) M(W0)||_inf, ||I - A(W2)(2 M1 - M0)||_inf),
    the whole-matrix residuals of the first warm slot and of the first extrapolated start."""
    d = W0.shape[0]
    I = np.eye(d)
    W1, _ = o.minimize(W0.copy(), 1.0, 1, s, lr, tol=-1.0)
    W2, _ = o.minimize(W0.copy(), 1.0, 2, s, lr, tol=-1.0)
    M0, M1 = sla.inv(a_matrix(W0, s)), sla.inv(a_matrix(W1, s))
    return inf_norm(I - a_matrix(W1, s) @ M0), inf_norm(I - a_matrix(W2, s) @ (2 * M1 - M0))
