"""Plain-numpy restatement of HSIC from low-rank factors ("HSIC from low-rank factors"),
written from the formulas and not from csrc/hsic.hip: the pivoted incomplete Cholesky factor of one
column's RBF Gram matrix, its centring, and HSIC(x, y[pi]) = || Fc^T Gc[pi] ||_F^2 / n^2
(tests/test_hsic_cpu.py certifies it against the reference's recorded results;
tests/test_gpu_hsic.py holds the kernels to it)."""
import numpy as np

from tests import indep_numpy as inp

ETA = 1e-13
RANK_CAP = 256


def gram(x, sigma2):
    x = np.asarray(x, dtype=np.float64)
    return np.exp(-(x[:, None] - x[None, :]) ** 2 / (2.0 * sigma2))


def ichol(x, sigma2, eta=ETA, cap=None):
    """(F, resid): K ~ F F^T by pivoted incomplete Cholesky.  A step takes the row with the largest
    residual diagonal entry (the first of equal ones), appends c = (K[:, p] - F F[p]) / sqrt(d_p) and
    lowers d by c^2 (never below 0; the pivot's own to 0).  It stops when max d <= eta, at rank n,
    or at `cap` columns; resid is max d then."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    d = np.ones(n)
    F = np.zeros((n, min(n, cap or n)))
    r = 0
    while True:
        p = int(np.argmax(d))
        if d[p] <= eta or r == F.shape[1]:
            return F[:, :r].copy(), float(d[p])
        c = (np.exp(-(x - x[p]) ** 2 / (2.0 * sigma2)) - F[:, :r] @ F[p, :r]) / np.sqrt(d[p])
        F[:, r] = c
        d = np.maximum(d - c * c, 0.0)
        d[p] = 0.0
        r += 1


def centred(F):
    return F - F.mean(axis=0)


def values(Fc, Gc, perms):
    """(P + 1,): the statistic of the identity and of every permutation."""
    n = Fc.shape[0]
    rows = [np.arange(n)] + [np.asarray(p, dtype=np.int64) for p in perms]
    return np.array([((Fc.T @ Gc[r]) ** 2).sum() / (float(n) * float(n)) for r in rows])


def hsic_null(X, pairs, perms, sigma2=None, eta=ETA):
    """(stat, ge, null, ranks): `mi_tests.hsic_null` for explicit perms (len(pairs), P, n); a pair
    with a zero-range column is (0, P, zeros).  ranks: column -> rank of its factor."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    fac, ranks = {}, {}
    for v in sorted({int(c) for pr in pairs for c in pr}):
        s2 = inp.median_sigma2(X[:, v]) if sigma2 is None else float(sigma2[v])
        F, _ = ichol(X[:, v], s2, eta, RANK_CAP)
        fac[v], ranks[v] = centred(F), F.shape[1]
    P = 0 if perms is None else np.asarray(perms).shape[1]
    stat, ge, null = np.zeros(len(pairs)), np.zeros(len(pairs), dtype=np.int64), np.zeros((len(pairs), P))
    for q, (i, j) in enumerate(pairs):
        i, j = int(i), int(j)
        if np.ptp(X[:, i]) == 0 or np.ptp(X[:, j]) == 0:
            ge[q] = P
            continue
        v = values(fac[i], fac[j], [] if perms is None else perms[q])
        stat[q], null[q], ge[q] = v[0], v[1:], int((v[1:] >= v[0]).sum())
    return stat, ge, null, ranks


def data(n, seed=0):
    """n x 5: gauss, a dependent column, rounded (ties), an independent heavy-ish tail, constant."""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    x, e, z = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    return np.ascontiguousarray(np.column_stack([x, np.sin(2.0 * x) + 0.3 * e, np.round(2.0 * z) / 2.0,
                                                 np.exp(0.7 * e), np.full(n, 1.5)]))


# rank -> sigma^2 that gives column 0 of data(300) that rank at ETA, each with the step before the
# stop above 2 ETA and the residual below ETA / 2 (tests/test_hsic_cpu.py checks the table)
FORCED_RANKS = {1: 1e30, 15: 3.492859048214689, 16: 2.977313784916276, 17: 2.4310576907605155,
                33: 0.29028255722403123, 70: 0.03640718179172758}

ALL_PAIRS_5 =[(i, j) for i in range(5) for j in range(i + 1, 5)]
