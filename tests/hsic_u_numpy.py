"""Plain-numpy restatement of the HSIC chi-square test ("HSIC chi-square test for every
pair"), written from the formulas and not from csrc/hsic.hip.

(a) `cov_u_direct`: the O(n^2) definition.  For a column with RBF Gram matrix K: D = 1 - K off the
    diagonal and 0 on it, U-centred (Szekely and Rizzo), cov_U(x, y) = <A~, B~> / (n (n - 3)).
(b) `cov_u_factors`: the same number from `hsic_numpy.ichol` factors and O(n) vectors a column,
    <A~_x, A~_y> = || Fc_x^T Fc_y ||_F^2 + 2 n v~_x.v~_y + n^2 c_x c_y - a_x.a_y.

The bound: a factor is within eta of K elementwise and U-centring is linear, so
|dA~_ij| <= c_n eta and |A~_ij| <= c_n with c_n = (4 n - 4) / (n - 2): an entry of D moves by at most
eta, a row mean r_i / (n - 2) by (n - 1) / (n - 2) eta, twice, and T / ((n - 1)(n - 2)) by
n / (n - 2) eta; the same with 1 for eta bounds A~ itself.  A product of two such entries moves by at
most c_n^2 eta (2 + eta), summed over n (n - 1) entries and divided by n (n - 3):
|d cov_U| <= B_n(eta) = (n - 1) / (n - 3) c_n^2 eta (2 + eta).
(tests/test_hsic_chi2_cpu.py certifies (b) against (a); tests/test_gpu_hsic_chi2.py holds the
kernels to both.)"""
import itertools

import numpy as np

from tests import hsic_numpy as hn
from tests import indep_numpy as inp

ROUND = 1e-12  # the project's rounding bar (tests/test_gpu_indep.py)


def u_centred(K):
    """A~ of D = 1 - K (diagonal 0)."""
    n = K.shape[0]
    D = 1.0 - K
    np.fill_diagonal(D, 0.0)
    r = D.sum(axis=1)
    A = D - r[:, None] / (n - 2) - r[None, :] / (n - 2) + r.sum() / ((n - 1) * (n - 2))
    np.fill_diagonal(A, 0.0)
    return A


def sigma2_of(X, sigma2=None):
    X = np.asarray(X, dtype=np.float64)
    if sigma2 is not None:
        return np.asarray(sigma2, dtype=np.float64)
    return np.array([inp.median_sigma2(X[:, v]) for v in range(X.shape[1])])


def cov_u_direct(X, sigma2=None):
    """(a): d x d, cov_U of every pair of columns, the variances on the diagonal."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    s2 = sigma2_of(X, sigma2)
    A = [u_centred(hn.gram(X[:, v], s2[v])) for v in range(d)]
    out = np.zeros((d, d))
    for i in range(d):
        for j in range(i, d):
            out[i, j] = out[j, i] = (A[i] * A[j]).sum() / (n * (n - 3.0))
    return out


def column_terms(F):
    """(Fc, v~, a, c) of one column's uncentred factor F."""
    n = F.shape[0]
    m = F.mean(axis=0)
    Fc = F - m
    khat = (F * F).sum(axis=1)
    rho = (n - 1.0) - (F @ F.sum(axis=0) - khat)
    T = rho.sum()
    v = -(Fc @ m) - rho / (n - 2.0)
    g = 1.0 - m @ m + T / ((n - 1.0) * (n - 2.0))
    a = -(Fc * Fc).sum(axis=1) + 2.0 * v + g
    return Fc, v - v.mean(), a, g + 2.0 * v.mean()


def cov_u_factors(X, sigma2=None, eta=hn.ETA):
    """(b): (cov_u, biased, ranks) from incomplete Cholesky factors at eta."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    s2 = sigma2_of(X, sigma2)
    terms, ranks = [], []
    for v in range(d):
        F, _ = hn.ichol(X[:, v], s2[v], eta, hn.RANK_CAP)
        terms.append(column_terms(F))
        ranks.append(F.shape[1])
    cov, bia = np.zeros((d, d)), np.zeros((d, d))
    for i in range(d):
        for j in range(i, d):
            (Fx, vx, ax, cx), (Fy, vy, ay, cy) = terms[i], terms[j]
            sq = ((Fx.T @ Fy) ** 2).sum()
            u = sq + 2.0 * n * (vx @ vy) + float(n) * n * cx * cy - ax @ ay
            cov[i, j] = cov[j, i] = u / (n * (n - 3.0))
            bia[i, j] = bia[j, i] = sq / (float(n) * n)
    return cov, bia, ranks


def bound(n, eta):
    """B_n(eta)."""
    cn = (4.0 * n - 4.0) / (n - 2.0)
    return (n - 1.0) / (n - 3.0) * cn * cn * eta * (2.0 + eta)


def r_u(cov):
    """R_U = cov_U(x, y) / sqrt(cov_U(x, x) cov_U(y, y)), 0 if either variance is <= 0."""
    cov = np.asarray(cov, dtype=np.float64)
    var = np.diag(cov)
    out = np.zeros_like(cov)
    for i in range(cov.shape[0]):
        for j in range(cov.shape[0]):
            if var[i] > 0 and var[j] > 0:
                out[i, j] = cov[i, j] / np.sqrt(var[i] * var[j])
    return out


def pvalues(R, n):
    from scipy import stats
    return stats.chi2.sf(n * np.asarray(R) + 1.0, 1)


def corner_intervals(cov, n, B):
    """(R, dR), d x d each: R_U of `cov` and the largest |R(corner) - R| over the eight corners
    (cov +- B, var_x +- B, var_y +- B).  R is monotone in each argument, so the corners bound the
    R_U of any covariances within B of these."""
    cov = np.asarray(cov, dtype=np.float64)
    d = cov.shape[0]
    R = r_u(cov)
    dR = np.zeros((d, d))
    for i in range(d):
        for j in range(d):
            for sc, sx, sy in itertools.product((-1.0, 1.0), repeat=3):
                c, vx, vy = cov[i, j] + sc * B, cov[i, i] + sx * B, cov[j, j] + sy * B
                rc = c / np.sqrt(vx * vy) if (vx > 0 and vy > 0) else 0.0
                dR[i, j] = max(dR[i, j], abs(rc - R[i, j]))
    return R, dR


def p_interval(R, dR, n):
    """(plo, phi): the p-values at R + (dR + ROUND) and R - (dR + ROUND); p falls as R grows."""
    return pvalues(R + (dR + ROUND), n), pvalues(R - (dR + ROUND), n)


API_N, API_D, API_SEED, API_ALPHA = 1000, 8, 11, 0.05


def api_case():
    """X (1000 x 8) of a gaussian linear SEM on a random ER graph: the public-API case."""
    from midagma_amd import utils
    utils.set_random_seed(API_SEED)
    B = utils.simulate_dag(API_D, API_D, "ER")
    W = utils.simulate_parameter(B)
    return np.ascontiguousarray(utils.simulate_linear_sem(W, API_N, "gauss"))


def pair_set(p, alpha=API_ALPHA):
    """(I, alpha_eff): the pairs i < j with p > alpha / #pairs, in the reference's order."""
    d = p.shape[0]
    i, j = np.triu_indices(d, 1)
    alpha_eff = alpha / len(i)
    keep = p[i, j] > alpha_eff
    return np.stack([i[keep], j[keep]], axis=1).astype(int).reshape(-1, 2), alpha_eff
