"""Plain-numpy restatement of csrc/corr.hip (no reference, no scipy): the order-preserving keys, the
average-tie ranks by a stable argsort and run bounds, and the correlation matrix by centring, Gram
and normalisation.  Also the rank inputs the CPU and GPU tiers share."""
import numpy as np

CASES = ("k257", "t1025", "m4097")
TESTS = ("pearson", "spearman")
ALPHA = 0.05
MARGIN = 1e-6

RANK_N = (2, 3, 64, 65, 257, 1025, 4097, 70001)
RANK_D = (1, 5, 67)
RANK_KINDS = ("normal", "small_ints", "constant", "zeros_denormals", "huge_range", "scaled_primes", "sorted",
              "reversed", "last_bit")


def keys(x):
    """The 64-bit sort key of every double: -0.0 as +0.0, then all bits of a negative flipped and
    the sign bit of a non-negative flipped, so unsigned key order is numeric order."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64).copy()
    b[(b << np.uint64(1)) == 0] = 0
    neg = (b >> np.uint64(63)).astype(bool)
    return np.where(neg, ~b, b ^ np.uint64(1 << 63))


def column_ranks(X):
    """R[r, c] = (lo + hi + 1) / 2 for the tie run [lo, hi) of X[r, c] in column c's sorted keys."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    R = np.empty((n, d))
    for c in range(d):
        k = keys(X[:, c])
        order = np.argsort(k, kind="stable")
        ks = k[order]
        head = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])  # run starts
        lens = np.diff(np.r_[head, n])
        lo = np.repeat(head, lens)
        hi = lo + np.repeat(lens, lens)
        R[order, c] = (lo + hi + 1) * 0.5
    return R


def correlation(X):
    """(Rho, const): const[c] iff max == min on the raw column; Rho = G_ij / sqrt(G_ii G_jj) of the
    centred columns, clamped to [-1, 1], 1 on the diagonal, NaN for constant columns."""
    X = np.asarray(X, dtype=np.float64)
    const = X.max(axis=0) == X.min(axis=0)
    Xc = X - X.sum(axis=0) / X.shape[0]
    G = Xc.T @ Xc
    g = np.diag(G)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = np.clip(G / np.sqrt(g[:, None] * g[None, :]), -1.0, 1.0)
    np.fill_diagonal(rho, 1.0)
    rho[const, :] = np.nan
    rho[:, const] = np.nan
    return rho, const


def pair_index(d, undirected, exclude_diagonal=True):
    if undirected:
        return [(i, j) for i in range(d) for j in range(i + 1, d)]
    return [(i, j) for i in range(d) for j in range(d) if not (exclude_diagonal and i == j)]


def alpha_effs(d):
    return (ALPHA, ALPHA / (d * (d - 1) // 2), ALPHA / (d * (d - 1)))


def p_bar(r_ref, n):
    """The relative bar on p: 1e-12 on r carried through p's sensitivity n |r| / (1 - r^2), x 10."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return 1e-11 * np.maximum(1.0, n * np.abs(r_ref) / (1.0 - r_ref * r_ref))


def check_against_reference(stat, p, stat_ref, p_ref, n, const, test):
    """The bars of the fixture comparison; returns (max |stat - ref|, max relative p error / bar)
    over the pairs they apply to.  stat, p: d x d."""
    d = stat.shape[0]
    off = ~np.eye(d, dtype=bool)
    bad = const[:, None] | const[None, :]
    live = off & ~bad
    serr = float(np.abs(stat - stat_ref)[live].max())
    assert serr <= 1e-12, serr
    big = live & (p_ref >= 1e-290)
    rel = np.abs(p - p_ref)[big] / p_ref[big]
    ratio = float((rel / p_bar(stat_ref, n)[big]).max()) if big.any() else 0.0
    assert ratio <= 1.0, ratio
    tiny = live & ~(p_ref >= 1e-290)
    assert (p[tiny] <= 1e-280).all()
    # the diagonal by rule, constant columns by the reference's rule
    dg = np.eye(d, dtype=bool) & ~bad
    assert (stat[dg] == 1.0).all() and (p[dg] == 0.0).all()
    if test == "pearson":
        assert np.isnan(stat[bad]).all() and np.isnan(p[bad]).all()
        assert np.isnan(stat_ref[bad]).all() and np.isnan(p_ref[bad]).all()
    else:
        assert (stat[bad] == 0.0).all() and (p[bad] == 1.0).all()
        assert (stat_ref[bad] == 0.0).all() and (p_ref[bad] == 1.0).all()
    return serr, ratio


def rank_input(kind, n, d, seed=0):
    """An n x d rank input of the named kind (module docstring of tests/test_gpu_corr.py)."""
    rng = np.random.default_rng([seed, n, d, RANK_KINDS.index(kind)])
    if kind == "normal":
        return rng.standard_normal((n, d))
    if kind == "small_ints":
        return rng.integers(0, 4, size=(n, d)).astype(np.float64)
    if kind == "constant":
        X = rng.standard_normal((n, d))
        X[:, d // 2] = 0.1
        return X
    if kind == "zeros_denormals":
        pool = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.2250738585072014e-308])
        return pool[rng.integers(0, len(pool), size=(n, d))]
    if kind == "huge_range":
        return rng.choice([-1.0, 1.0], size=(n, d)) * 10.0 ** rng.uniform(-300, 300, size=(n, d))
    if kind == "scaled_primes":
        base = np.array([1.0, 2.0, 3.0, 5.0, 7.0])
        scale = np.array([2.0 ** -40, 1.0, 2.0 ** 40])
        return base[rng.integers(0, 5, size=(n, d))] * scale[rng.integers(0, 3, size=(n, d))]
    if kind == "sorted":
        return np.sort(rng.standard_normal((n, d)), axis=0)
    if kind == "reversed":
        return np.sort(rng.standard_normal((n, d)), axis=0)[::-1].copy()
    if kind == "last_bit":
        b = np.float64(1.5).view(np.uint64) + rng.integers(0, 3, size=(n, d)).astype(np.uint64)
        return b.view(np.float64) * rng.choice([-1.0, 1.0], size=(n, d))
    raise ValueError(kind)
