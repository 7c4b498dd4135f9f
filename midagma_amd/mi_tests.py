"""Pairwise independence tests that build the trek regularizers' pair set I -- the reference's
`notreks.mi_tests` with the permutation tests on the GPU.

Names, signatures, defaults and pair order are the reference's.  'hsic' and 'dcor' run their
permutation tests in csrc/indep.hip through `midagma_amd.solver.HipIndep`; there is no CPU path for
them (no device: `HipSolverError`).  'pearson' and 'spearman' are analytic: inside
`test_pairwise_independence` and `get_I_from_full_pairwise_tests` they run on the host, scipy once
per pair, exactly as in the reference (bit for bit, and O(pairs) rankings: small problems only).

For all pairs at once there are two functions the reference does not have,
`correlation_tests(X, test="pearson" | "spearman")` and `get_I_from_correlation_tests(X, ...)`:
the column ranks (a batched radix sort) and the correlation matrix (centring and the FP64 MFMA
Gram) are computed on the GPU by csrc/corr.hip from a host or device-resident X, and scipy's
analytic p-values are evaluated on the host for the whole d x d matrix in one vectorised call.
They agree with the per-pair path to rounding in the correlation ("Ranks and
correlations") and return the same I wherever no p-value is within that rounding of alpha_eff.
There is no CPU path for them either.

The 'dcor' test of those functions sums n^2 terms an evaluation and stops at n = 16384.  Beside it,
for any n < 2^31, stand three more functions the reference does not have: `dcor_null`, `dcor_tests`
and `get_I_from_dcor_tests` (csrc/dcor.hip through `midagma_amd.solver.HipDcor`): the same
statistic, exact, from a sort, block sums and cell tables in O(n sqrt(n)) work an evaluation, with
the permutation p-value or the analytic chi-square p-value of the bias-corrected statistic
("dCor without the n^2 sum").  They change nothing of the functions above.

The 'hsic' test of those functions has the same n^2 sum and the same cap.  `hsic_null`, `hsic_tests`
and `get_I_from_hsic_tests` (csrc/hsic.hip through `midagma_amd.solver.HipHsic`) lift it: each
column's RBF Gram matrix is replaced by a pivoted incomplete Cholesky factor with elementwise error
<= tol, and an evaluation becomes a small FP64 MFMA GEMM over gathered factor rows.  The statistic is
the reference's to within 4 tol (1 + tol) plus rounding ("HSIC from low-rank factors"),
the median bandwidths are the reference's bit for bit, at any n < 2^31.  They too change nothing of
the functions above.  `hsic_tests(pvalue="chi2")` tests every pair with one evaluation and no
permutations: the chi-square test of `dcor_tests(pvalue="chi2")` on the U-centred RBF kernel, from
one tiled FP64 MFMA pass over all the factors ("HSIC chi-square test for every pair").

One keyword is added, ``perms``:
  * ``"numpy"`` (default): the host draws ``rng = np.random.default_rng(seed)`` once and calls
    ``rng.permutation(n)`` num_perm times per pair, in pair order -- the reference's stream, so the
    p-values are the reference's.  Generation of the next chunk of pairs overlaps the device work
    of the current one.
  * ``"device"``: the permutations are made on the GPU from Philox4x32-10 ("Independence
    tests").  The p-values are valid permutation p-values but come from another stream than the
    reference's.

The RBF kernels' median-heuristic bandwidths of 'hsic' are computed on the device
(`HipIndep.median_bandwidths`, no O(n^2) host work).  `permutation_null` has a keyword
``bandwidths`` for it: ``"device"`` (default) or ``"host"`` (`median_sigma2`, numpy).  The two give
the same bits, so no result depends on it; `test_pairwise_independence` and
`get_I_from_full_pairwise_tests` keep the reference's parameter lists (plus ``perms``) and use the
default.

X (x and y for the two `_stat` functions) may be a float64 torch CUDA tensor: 'hsic' and 'dcor' then
read it on its device, on torch's current stream, without a host copy and without writing it
(``perms="numpy"`` still draws on the host and uploads the permutations); 'pearson' and 'spearman'
copy it to the host.

Not mirrored: `permutation_pvalue(stat_fn, ...)`, which takes an arbitrary Python callable.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Iterable, List, Literal, Optional, Tuple

import numpy as np

from .solver import HipDcor, HipHsic, HipIndep, _device_x, _host_x, is_device_tensor

__all__ = ["IndepTestResult", "hsic_stat", "dcor_stat", "permutation_null", "test_pairwise_independence",
           "get_I_from_full_pairwise_tests", "summarize_I", "median_sigma2", "correlation_tests",
           "get_I_from_correlation_tests", "dcor_null", "dcor_tests", "get_I_from_dcor_tests", "hsic_null",
           "hsic_tests", "get_I_from_hsic_tests"]

TestName = Literal["hsic", "dcor", "pearson", "spearman"]

# host bytes of numpy permutations generated ahead of the device (two chunks exist at a time)
_HOST_CHUNK_BYTES = 128 << 20


@dataclass(frozen=True)
class IndepTestResult:
    i: int
    j: int
    stat: float
    pvalue: float


def median_sigma2(x: np.ndarray) -> float:
    """The reference's median heuristic (`_rbf_gram`, sigma=None): the median of the off-diagonal
    squared differences, 1.0 when that median is 0.  Host work: n (n - 1) / 2 values."""
    x = np.asarray(x, dtype=np.float64).ravel()
    n = x.shape[0]
    off = np.empty(n * (n - 1) // 2)
    k = 0
    for a in range(n - 1):
        off[k:k + n - 1 - a] = (x[a] - x[a + 1:]) ** 2
        k += n - 1 - a
    med = np.median(off)
    return float(med) if med > 0 else 1.0


def _sigma2(x, sigma) -> float:
    if sigma is None:
        return median_sigma2(x)
    s2 = float(sigma) ** 2
    return s2 if s2 > 0 else 1.0


def _as_data(X, max_n=HipIndep.MAX_N):
    """A C-contiguous float64 copy (the caller's X is never touched), checked; a device tensor is
    checked for dtype and shape and returned with unit column stride (the engine only reads it, and
    checks it for inf and nan on the device)."""
    if is_device_tensor(X):
        return _device_x(X, "X", max_n)
    return _host_x(X, "X", max_n, copy=True)


def _as_pairs(pairs, d: int) -> np.ndarray:
    P = np.asarray(list(pairs), dtype=np.int64).reshape(-1, 2)
    if P.size and (P.min() < 0 or P.max() >= d):
        raise ValueError(f"pair index outside [0, {d})")
    return P


def _host(X) -> np.ndarray:
    return X.detach().cpu().numpy() if is_device_tensor(X) else X


def _two_columns(x, y):
    if is_device_tensor(x) or is_device_tensor(y):
        import torch
        dev = x.device if is_device_tensor(x) else y.device
        x = torch.as_tensor(x, dtype=torch.float64, device=dev).reshape(-1)
        y = torch.as_tensor(y, dtype=torch.float64, device=dev).reshape(-1)
        if x.shape != y.shape:
            raise ValueError("x and y must have the same length")
        return _as_data(torch.stack([x, y], dim=1))
    x = np.asarray(x, dtype=np.float64).ravel()
    y = np.asarray(y, dtype=np.float64).ravel()
    if x.shape != y.shape:
        raise ValueError("x and y must have the same length")
    return _as_data(np.column_stack([x, y]))


def hsic_stat(x: np.ndarray, y: np.ndarray, sigma_x: Optional[float] = None, sigma_y: Optional[float] = None) -> float:
    """Biased HSIC estimator (1/n^2) sum(Kc * Lc) with RBF kernels (median-heuristic bandwidths
    unless given), on the GPU."""
    X = _two_columns(x, y)
    eng = HipIndep(X)
    try:
        given = (sigma_x, sigma_y)
        auto = [v for v in (0, 1) if given[v] is None]
        s2 = eng.median_bandwidths(auto) if auto else np.ones(2)
        for v in (0, 1):
            if given[v] is not None:
                s2[v] = _sigma2(None, given[v])
        if len(auto) < 2:
            eng.set_bandwidths(s2)
        stat, _ = eng.run("hsic", [(0, 1)], 0)
    finally:
        eng.close()
    return float(stat[0])


def dcor_stat(x: np.ndarray, y: np.ndarray) -> float:
    """Distance correlation (from the biased distance covariance), on the GPU."""
    X = _two_columns(x, y)
    eng = HipIndep(X)
    try:
        stat, _ = eng.run("dcor", [(0, 1)], 0)
    finally:
        eng.close()
    return float(stat[0])


def _numpy_perms(rng: np.random.Generator, m: int, P: int, n: int) -> np.ndarray:
    out = np.empty((m, P, n), dtype=np.int32)
    for q in range(m):
        for p in range(P):
            out[q, p] = rng.permutation(n)
    return out


def permutation_null(X, pairs, *, test: str = "hsic", num_perm: int = 200, seed: int = 0, perms: str = "numpy",
                     device: int = 0, budget_bytes: int = 0, return_null: bool = True, bandwidths: str = "device"):
    """(stat, ge, null): per pair the observed statistic, ge = #{p : stat_p >= stat} and (m x
    num_perm, or None) the permuted statistics of the 'hsic' / 'dcor' permutation test.
    budget_bytes: the device's byte budget per pair batch (0: the library's default); results do
    not depend on it.  bandwidths: where the 'hsic' medians are computed ('device' or 'host'; the
    same bits).  A device X makes its device the engine's (`device` is ignored)."""
    if test not in HipIndep.KINDS:
        raise ValueError("test must be 'hsic' or 'dcor'")
    if perms not in ("numpy", "device"):
        raise ValueError("perms must be 'numpy' or 'device'")
    if bandwidths not in ("device", "host"):
        raise ValueError("bandwidths must be 'device' or 'host'")
    X = _as_data(X)
    n, d = X.shape
    pairs = _as_pairs(pairs, d)
    m, P = len(pairs), int(num_perm)
    if P < 0:
        raise ValueError("num_perm must be >= 0")
    eng = HipIndep(X, device)
    try:
        if test == "hsic" and bandwidths == "device":
            eng.median_bandwidths(np.unique(pairs))
        elif test == "hsic":
            s2 = np.ones(d)
            for v in np.unique(pairs):
                s2[v] = median_sigma2(_host(X[:, v]))
            eng.set_bandwidths(s2)
        if perms == "device":
            out = eng.run(test, pairs, P, None, seed, budget_bytes, return_null=return_null)
            return out[0], out[1], (out[2] if return_null else None)
        rng = np.random.default_rng(seed)
        stat = np.zeros(m)
        ge = np.zeros(m, dtype=np.int64)
        null = np.zeros((m, P)) if return_null else None
        chunk = max(1, _HOST_CHUNK_BYTES // max(1, 4 * P * n))

        def consume(q0, q1, pm):
            out = eng.run(test, pairs[q0:q1], P, pm, 0, budget_bytes, return_null=return_null)
            stat[q0:q1], ge[q0:q1] = out[0], out[1]
            if return_null:
                null[q0:q1] = out[2]

        # the worker thread drives the device (the library call releases the GIL) while this
        # thread draws the next chunk's permutations
        with ThreadPoolExecutor(max_workers=1) as pool:
            pending = None
            for q0 in range(0, m, chunk):
                q1 = min(m, q0 + chunk)
                pm = _numpy_perms(rng, q1 - q0, P, n)
                if pending is not None:
                    pending.result()
                pending = pool.submit(consume, q0, q1, pm)
            if pending is not None:
                pending.result()
        return stat, ge, null
    finally:
        eng.close()


def _pearson_stat_pvalue(x, y) -> Tuple[float, float]:
    from scipy import stats
    r, p = stats.pearsonr(np.asarray(x).ravel(), np.asarray(y).ravel())
    return float(abs(r)), float(p)


def _spearman_stat_pvalue(x, y) -> Tuple[float, float]:
    import warnings

    from scipy import stats
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (scipy warns about constant input; the rule below handles it)
        rho, p = stats.spearmanr(np.asarray(x).ravel(), np.asarray(y).ravel())
    if not np.isfinite(rho) or not np.isfinite(p):  # scipy returns nan for constant inputs
        return 0.0, 1.0
    return float(abs(rho)), float(p)


def test_pairwise_independence(X: np.ndarray, pairs: Iterable[Tuple[int, int]], *, test: TestName = "hsic",
                               num_perm: int = 200, seed: int = 0,
                               perms: str = "numpy") -> List[IndepTestResult]:
    """(stat, pvalue) per pair.  hsic, dcor: permutation p-values (ge + 1) / (num_perm + 1) on the
    GPU; pearson, spearman: scipy's analytic p-values (num_perm, seed, perms ignored)."""
    if test not in ("hsic", "dcor", "pearson", "spearman"):
        raise ValueError("test must be one of 'hsic', 'dcor', 'pearson', 'spearman'")
    pairs = [(int(i), int(j)) for (i, j) in pairs]
    if test in ("pearson", "spearman"):
        X = _as_data(_host(X))
        _as_pairs(pairs, X.shape[1])
        fn = _pearson_stat_pvalue if test == "pearson" else _spearman_stat_pvalue
        out = []
        for (i, j) in pairs:
            stat, p = fn(X[:, i], X[:, j])
            out.append(IndepTestResult(i=i, j=j, stat=stat, pvalue=p))
        return out
    stat, ge, _ = permutation_null(X, pairs, test=test, num_perm=num_perm, seed=seed, perms=perms, return_null=False)
    return [IndepTestResult(i=i, j=j, stat=float(stat[q]), pvalue=float((int(ge[q]) + 1) / (int(num_perm) + 1)))
            for q, (i, j) in enumerate(pairs)]


test_pairwise_independence.__test__ = False  # a library function, not a pytest test


def get_I_from_full_pairwise_tests(X: np.ndarray, *, alpha: float = 0.05, test: TestName = "hsic",
                                   num_perm: int = 200, seed: int = 0, bonferroni: bool = True,
                                   undirected: bool = True, exclude_diagonal: bool = True,
                                   perms: str = "numpy") -> np.ndarray:
    """Test all pairs and return I = {(i, j): p > alpha_eff}, the pairs whose independence is not
    rejected (alpha_eff = alpha / #pairs under Bonferroni), in the reference's pair order."""
    if not is_device_tensor(X):
        X = np.asarray(X)
    n, d = X.shape
    pairs: List[Tuple[int, int]] = []
    if undirected:
        for i in range(d):
            for j in range(i + 1, d):
                pairs.append((i, j))
    else:
        for i in range(d):
            for j in range(d):
                if exclude_diagonal and i == j:
                    continue
                pairs.append((i, j))
    results = test_pairwise_independence(X, pairs, test=test, num_perm=num_perm, seed=seed, perms=perms)
    m = len(results)
    alpha_eff = (alpha / m) if (bonferroni and m > 0) else alpha
    I = [(r.i, r.j) for r in results if r.pvalue > alpha_eff]
    return np.asarray(I, dtype=int)


def _pearson_pvalues(r: np.ndarray, n: int) -> np.ndarray:
    """scipy.stats.pearsonr's two-sided p-value at r, elementwise: r is Beta(n/2 - 1, n/2 - 1) on
    [-1, 1] under independence (the distribution object scipy uses; n = 2: p = 1 as in scipy)."""
    from scipy import stats
    r = np.asarray(r, dtype=np.float64)
    if n == 2:
        return np.where(np.isnan(r), np.nan, 1.0)
    ab = n / 2 - 1
    return 2 * stats.beta(ab, ab, loc=-1, scale=2).sf(np.abs(r))


def _spearman_pvalues(r: np.ndarray, n: int) -> np.ndarray:
    """scipy.stats.spearmanr's two-sided p-value at r, elementwise: t = r sqrt(dof / ((r + 1)(1 - r)))
    is Student-t with dof = n - 2 under independence."""
    from scipy import stats
    r = np.asarray(r, dtype=np.float64)
    dof = n - 2
    with np.errstate(divide="ignore", invalid="ignore"):
        t = r * np.sqrt((dof / ((r + 1.0) * (1.0 - r))).clip(0))
        return 2 * stats.t.sf(np.abs(t), dof)


def _stat_pvalue_from_rho(rho: np.ndarray, const: np.ndarray, n: int, test: str):
    """(stat, pvalue), d x d each, from a correlation matrix and its constant-column marks, by
    the reference's rules: stat = |rho|; the diagonal is (1, 0); a pair with a constant column is
    (nan, nan) for 'pearson' (scipy's result, passed on) and (0, 1) for 'spearman' (the
    reference's replacement of scipy's nan)."""
    rho = np.asarray(rho, dtype=np.float64)
    const = np.asarray(const, dtype=bool)
    d = rho.shape[0]
    # the distribution functions are the cost at large d (scipy's beta.sf: 5 us a value), so they
    # run on the entries above the diagonal only and (j, i) takes (i, j)'s values
    iu = np.triu_indices(d, 1)
    r = rho[iu]
    stat, p = np.empty((d, d)), np.empty((d, d))
    stat[iu] = np.abs(r)
    p[iu] = _pearson_pvalues(r, n) if test == "pearson" else _spearman_pvalues(r, n)
    stat.T[iu], p.T[iu] = stat[iu], p[iu]
    np.fill_diagonal(stat, 1.0)
    np.fill_diagonal(p, 0.0)
    bad = const[:, None] | const[None, :]
    if test == "pearson":
        stat[bad], p[bad] = np.nan, np.nan
    else:
        bad |= ~np.isfinite(stat) | ~np.isfinite(p)
        stat[bad], p[bad] = 0.0, 1.0
    return stat, p


def correlation_tests(X, *, test: str = "pearson", device: int = 0, budget_bytes: int = 0):
    """(stat, pvalue), two d x d host arrays: the 'pearson' or 'spearman' test of every ordered
    pair of X's columns at once, with the correlations (and, for 'spearman', the column ranks)
    computed on the GPU (csrc/corr.hip) and scipy's analytic p-values vectorised on the host.
    Entry (i, j) is what `test_pairwise_independence(X, [(i, j)], test=test)` returns, to rounding
    in the correlation; the diagonal is (1, 0) by rule, and (j, i) holds (i, j)'s values (i < j).
    X: a host float64 array (uploaded to
    `device`) or a float64 CUDA tensor, read in place and never written (`device` is ignored).
    ValueError when X holds inf or nan; no GPU: `HipSolverError` (there is no CPU path)."""
    from .solver import _device_matrix, correlation
    if test not in ("pearson", "spearman"):
        raise ValueError("test must be 'pearson' or 'spearman'")
    Xd = _device_matrix(X, "correlation_tests", device)
    n = int(Xd.shape[0])
    rho, const = correlation(Xd, ranks=(test == "spearman"), budget_bytes=budget_bytes)
    return _stat_pvalue_from_rho(rho.cpu().numpy(), const, n, test)


def get_I_from_correlation_tests(X, *, alpha: float = 0.05, test: str = "pearson", bonferroni: bool = True,
                                 undirected: bool = True, exclude_diagonal: bool = True,
                                 device: int = 0) -> np.ndarray:
    """`get_I_from_full_pairwise_tests` for the analytic tests, with every pair tested at once by
    `correlation_tests`: I = {(i, j): p > alpha_eff} in the reference's pair order, alpha_eff =
    alpha / #pairs under Bonferroni; the same dtype and shape, the empty case included."""
    _, p = correlation_tests(X, test=test, device=device)
    d = p.shape[0]
    if undirected:
        i, j = np.triu_indices(d, 1)
    else:
        i, j = np.divmod(np.arange(d * d), d)
        if exclude_diagonal:
            i, j = i[i != j], j[i != j]
    m = len(i)
    alpha_eff = (alpha / m) if (bonferroni and m > 0) else alpha
    keep = p[i, j] > alpha_eff  # (nan compares False: a pearson pair with a constant column never enters I)
    if not keep.any():
        return np.asarray([], dtype=int)
    return np.stack([i[keep], j[keep]], axis=1).astype(int)


def _I_from_pvalues(p: np.ndarray, alpha: float, bonferroni: bool, undirected: bool,
                    exclude_diagonal: bool) -> np.ndarray:
    d = p.shape[0]
    if undirected:
        i, j = np.triu_indices(d, 1)
    else:
        i, j = np.divmod(np.arange(d * d), d)
        if exclude_diagonal:
            i, j = i[i != j], j[i != j]
    m = len(i)
    alpha_eff = (alpha / m) if (bonferroni and m > 0) else alpha
    keep = p[i, j] > alpha_eff
    if not keep.any():
        return np.asarray([], dtype=int)
    return np.stack([i[keep], j[keep]], axis=1).astype(int)


def _engine_null(eng, pairs: np.ndarray, P: int, seed: int, perms, return_null: bool, **kw):
    """(stat, ge, null or None) of `eng.run` (HipDcor, HipHsic; kw: the engine's own arguments) with
    the engine's device permutations, numpy's drawn as `permutation_null` draws them (a host chunk
    of pairs at a time), or the given ones."""
    n, m = eng.n, len(pairs)
    kw["return_null"] = True
    if isinstance(perms, str) and perms == "device":
        stat, ge, null = eng.run(pairs, P, None, seed, **kw)
    elif isinstance(perms, str):
        rng = np.random.default_rng(seed)
        stat, ge, null = np.zeros(m), np.zeros(m, dtype=np.int64), np.zeros((m, P))
        step = max(1, _HOST_CHUNK_BYTES // max(1, 4 * P * n))
        for q0 in range(0, m, step):
            q1 = min(m, q0 + step)
            pm = _numpy_perms(rng, q1 - q0, P, n)
            stat[q0:q1], ge[q0:q1], null[q0:q1] = eng.run(pairs[q0:q1], P, pm, 0, **kw)
    else:
        stat, ge, null = eng.run(pairs, P, perms, 0, **kw)
    return stat, ge, (null if return_null else None)


def _check_perms(perms, arrays: bool = True):
    """A string `perms` names a generator; `arrays`: the entry also takes explicit permutations."""
    if isinstance(perms, str) and perms not in ("numpy", "device"):
        raise ValueError("perms must be 'numpy', 'device' or an int32 array (m, num_perm, n)" if arrays
                         else "perms must be 'numpy' or 'device'")


def _perm_array(perms, m: int, P: int, n: int):
    """`perms` if it names a generator, else the explicit permutations as a checked int32 array."""
    if isinstance(perms, str):
        return perms
    perms = np.ascontiguousarray(perms, dtype=np.int32)
    if perms.shape != (m, P, n):
        raise ValueError(f"perms must be {(m, P, n)}, got {perms.shape}")
    return perms


def _mirrored(d: int, iu, s, pv, diagonal: float):
    """(stat, p), d x d: s and pv of the pairs iu (i < j) at (i, j) and (j, i); the diagonal is
    (`diagonal`, 0) by rule."""
    stat, p = np.full((d, d), float(diagonal)), np.zeros((d, d))
    if len(iu[0]):
        stat[iu], p[iu] = s, pv
        stat.T[iu], p.T[iu] = s, pv
    return stat, p


def dcor_null(X, pairs, *, num_perm: int = 200, seed: int = 0, perms="numpy", unbiased: bool = False,
              device: int = 0, budget_bytes: int = 0, return_null: bool = True, block: int = 0):
    """`permutation_null(test="dcor")` without the n^2 sum and without its cap on n (csrc/dcor.hip:
    a sort, block sums and cell tables, exact in O(n sqrt(n)) work an evaluation): (stat, ge, null)
    with the same conventions, to rounding the same values.
    perms: ``"numpy"`` draws one ``default_rng(seed)`` exactly as `permutation_null` does (pair
    order, num_perm permutations each); ``"device"`` makes them on the GPU by this path's own rule
    (the stable argsort of 64 Philox bits per row, DESIGN.md, so not `permutation_null`'s device
    stream); an int32 array (m, num_perm, n) is taken as given (every row must be a permutation).
    unbiased: the bias-corrected R_U = dcov^2_U / sqrt(dvar_U,x dvar_U,y) (U-centring; needs n >= 4),
    counted by dcov^2_U.  budget_bytes: the device scratch per chunk of evaluations (0: 2 GiB);
    block: the block edge (0: the rule; tests); results do not depend on the budget."""
    _check_perms(perms)
    X = _as_data(X, max_n=None)
    n, d = int(X.shape[0]), int(X.shape[1])
    pairs = _as_pairs(pairs, d)
    P = int(num_perm)
    if P < 0:
        raise ValueError("num_perm must be >= 0")
    if unbiased and n < 4:
        raise ValueError("the bias-corrected statistic needs n >= 4")
    if not (block == 0 or 4 <= int(block) <= 1024):
        raise ValueError("block must be 0 or in [4, 1024]")
    perms = _perm_array(perms, len(pairs), P, n)
    eng = HipDcor(X, device, budget_bytes)
    try:
        return _engine_null(eng, pairs, P, seed, perms, return_null, unbiased=unbiased, block=int(block),
                            budget_bytes=budget_bytes)
    finally:
        eng.close()


def dcor_tests(X, *, pvalue: str = "permutation", num_perm: int = 200, seed: int = 0, perms="device",
               device: int = 0, budget_bytes: int = 0):
    """(stat, p), two d x d host arrays: the dCor test of every pair i < j of X's columns, in the
    reference's pair order, mirrored to (j, i); the diagonal is (1, 0) by rule and a pair with a
    zero-range column is (0, 1).
    pvalue="permutation": stat is the reference's dCor (`dcor_null`), p = (ge + 1) / (num_perm + 1).
    pvalue="chi2": one evaluation a pair, no permutations: stat is the bias-corrected R_U and
    p = chi2.sf(n R_U + 1, 1), the chi-square test of Shen, Panda and Vogelstein, "The chi-square test
    of distance correlation" (valid and slightly conservative at alpha <= 0.05).  It is not in the
    reference, which has only the permutation test.  n < 4 raises ValueError."""
    if pvalue not in ("permutation", "chi2"):
        raise ValueError("pvalue must be 'permutation' or 'chi2'")
    _check_perms(perms, arrays=False)
    X = _as_data(X, max_n=None)
    n, d = int(X.shape[0]), int(X.shape[1])
    if pvalue == "chi2" and n < 4:
        raise ValueError("the chi-square test needs n >= 4")
    P = int(num_perm)
    if P < 0:
        raise ValueError("num_perm must be >= 0")
    iu = np.triu_indices(d, 1)
    pairs = np.stack(iu, axis=1).astype(np.int64)
    s = pv = None
    if len(pairs):
        eng = HipDcor(X, device, budget_bytes)
        try:
            if pvalue == "chi2":
                from scipy import stats
                s, ge, _ = _engine_null(eng, pairs, 0, 0, "device", False, unbiased=True, budget_bytes=budget_bytes)
                zero = _zero_range(X)  # (their R_U is 0 by rule, and the rule's p is 1, not chi2.sf(1))
                pv = np.where(zero[iu[0]] | zero[iu[1]], 1.0, stats.chi2.sf(n * s + 1.0, 1))
            else:
                s, ge, _ = _engine_null(eng, pairs, P, seed, perms, False, budget_bytes=budget_bytes)
                pv = (ge + 1.0) / (P + 1.0)
        finally:
            eng.close()
    return _mirrored(d, iu, s, pv, 1.0)


def _zero_range(X) -> np.ndarray:
    """max == min per column, on the raw values."""
    if is_device_tensor(X):
        return (X.max(dim=0).values == X.min(dim=0).values).cpu().numpy()
    return X.max(axis=0) == X.min(axis=0)


def get_I_from_dcor_tests(X, *, alpha: float = 0.05, pvalue: str = "permutation", num_perm: int = 200,
                          seed: int = 0, perms="device", bonferroni: bool = True, undirected: bool = True,
                          exclude_diagonal: bool = True, device: int = 0) -> np.ndarray:
    """`get_I_from_full_pairwise_tests(test="dcor")` through `dcor_tests`: I = {(i, j): p > alpha_eff}
    in the reference's pair order, built from p exactly as `get_I_from_correlation_tests` builds it
    (alpha_eff = alpha / #pairs under Bonferroni; the same dtype and shape, the empty case included).
    With perms="numpy" and undirected=True the p-values are `permutation_null`'s."""
    _, p = dcor_tests(X, pvalue=pvalue, num_perm=num_perm, seed=seed, perms=perms, device=device)
    return _I_from_pvalues(p, alpha, bonferroni, undirected, exclude_diagonal)


def _hsic_engine(X, device: int, budget_bytes: int, cols, sigma2) -> HipHsic:
    """An engine on X with its bandwidths: the medians of the listed columns (sigma2 None) or the
    given squared bandwidths (d values)."""
    eng = HipHsic(X, device, budget_bytes)
    try:
        if sigma2 is None:
            eng.median_bandwidths(cols)
        else:
            eng.set_bandwidths(sigma2)
    except Exception:
        eng.close()
        raise
    return eng


def _check_hsic_args(perms, num_perm, tol, chunk):
    _check_perms(perms)
    if int(num_perm) < 0:
        raise ValueError("num_perm must be >= 0")
    if not 1e-14 <= float(tol) <= 1e-3:
        raise ValueError("tol must be in [1e-14, 1e-3]")
    if not (chunk == 0 or (16 <= int(chunk) <= 2**20 and int(chunk) % 16 == 0)):
        raise ValueError("chunk must be 0 or a multiple of 16 in [16, 2^20]")


def hsic_null(X, pairs, *, num_perm: int = 200, seed: int = 0, perms="numpy", tol: float = 1e-13, device: int = 0,
              budget_bytes: int = 0, return_null: bool = True, sigma2=None, chunk: int = 0):
    """`permutation_null(test="hsic")` without the n^2 sum and without its cap on n (csrc/hsic.hip:
    low-rank factors of the RBF Gram matrices, an FP64 MFMA GEMM an evaluation): (stat, ge, null)
    with the same conventions; every value is within 4 tol (1 + tol) plus rounding of the n^2 sum's.
    perms: ``"numpy"`` draws one ``default_rng(seed)`` exactly as `permutation_null` does;
    ``"device"`` makes them on the GPU by `dcor_null`'s rule; an int32 array (m, num_perm, n) is taken
    as given (every row must be a permutation).  tol: the largest residual diagonal entry at which a
    column's factorisation stops (1e-14 .. 1e-3); a column that needs a rank above 256 raises
    ValueError.  sigma2: d squared bandwidths instead of the median heuristic.  budget_bytes: the
    device bytes for factors and scratch (0: 2 GiB); chunk: rows per partial product (0: the rule;
    tests); results do not depend on the budget."""
    _check_hsic_args(perms, num_perm, tol, chunk)
    X = _as_data(X, max_n=None)
    n, d = int(X.shape[0]), int(X.shape[1])
    pairs = _as_pairs(pairs, d)
    P = int(num_perm)
    perms = _perm_array(perms, len(pairs), P, n)
    if sigma2 is not None:
        sigma2 = np.ascontiguousarray(sigma2, dtype=np.float64).ravel()
        if sigma2.size != d or not (np.isfinite(sigma2).all() and (sigma2 > 0).all()):
            raise ValueError("sigma2 must hold d finite squared bandwidths > 0")
    eng = _hsic_engine(X, device, budget_bytes, np.unique(pairs), sigma2)
    try:
        return _engine_null(eng, pairs, P, seed, perms, return_null, tol=float(tol), chunk=int(chunk),
                            budget_bytes=budget_bytes)
    finally:
        eng.close()


def hsic_tests(X, *, pvalue: str = "permutation", num_perm: int = 200, seed: int = 0, perms="device",
               tol: float = 1e-13, device: int = 0, budget_bytes: int = 0, sigma2=None):
    """(stat, p), two d x d host arrays: the HSIC test of every pair i < j of X's columns, in the
    reference's pair order, mirrored to (j, i).  A pair with a zero-range column is (0, 1).  The
    diagonal is (nan, 0) by rule: the reference tests no column against itself.
    pvalue="permutation": the permutation test (`hsic_null`), p = (ge + 1) / (num_perm + 1).
    pvalue="chi2": one evaluation a pair, no permutations (`HipHsic.all_pairs`, one tiled pass over
    all the factors): stat is the bias-corrected correlation R_U of the distances D = 1 - K (hyppo's
    Hsic convention) and p = chi2.sf(n R_U + 1, 1), the chi-square test of Shen, Panda and
    Vogelstein that `dcor_tests(pvalue="chi2")` uses, which holds for any characteristic kernel.  It
    is not in the reference, which has only the permutation test.  n < 4 raises ValueError."""
    if pvalue not in ("permutation", "chi2"):
        raise ValueError("pvalue must be 'permutation' or 'chi2'")
    _check_perms(perms, arrays=False)
    _check_hsic_args(perms, num_perm, tol, 0)
    X = _as_data(X, max_n=None)
    n, d = int(X.shape[0]), int(X.shape[1])
    if pvalue == "chi2" and n < 4:
        raise ValueError("the chi-square test needs n >= 4")
    P = int(num_perm)
    iu = np.triu_indices(d, 1)
    pairs = np.stack(iu, axis=1).astype(np.int64)
    s = pv = None
    if len(pairs):
        eng = _hsic_engine(X, device, budget_bytes, None, sigma2)
        try:
            if pvalue == "chi2":
                cov, _ = eng.all_pairs(None, tol=float(tol), budget_bytes=budget_bytes)
            else:
                s, ge, _ = _engine_null(eng, pairs, P, seed, perms, False, tol=float(tol), budget_bytes=budget_bytes)
        finally:
            eng.close()
        if pvalue == "chi2":
            from scipy import stats
            s = _r_u(cov)[iu]
            zero = _zero_range(X)  # (their R_U is 0 by rule, and the rule's p is 1, not chi2.sf(1))
            pv = np.where(zero[iu[0]] | zero[iu[1]], 1.0, stats.chi2.sf(n * s + 1.0, 1))
        else:
            pv = (ge + 1.0) / (P + 1.0)
    return _mirrored(d, iu, s, pv, np.nan)


def _r_u(cov: np.ndarray) -> np.ndarray:
    """R_U = cov_U(x, y) / sqrt(cov_U(x, x) cov_U(y, y)) from the matrix of U-centred covariances;
    0 where either variance is <= 0."""
    var = np.diag(cov)
    den = var[:, None] * var[None, :]
    ok = (var[:, None] > 0) & (var[None, :] > 0)
    return np.where(ok, cov / np.sqrt(np.where(ok, den, 1.0)), 0.0)


def get_I_from_hsic_tests(X, *, alpha: float = 0.05, pvalue: str = "permutation", num_perm: int = 200,
                          seed: int = 0, perms="device", bonferroni: bool = True, undirected: bool = True,
                          exclude_diagonal: bool = True, tol: float = 1e-13, device: int = 0) -> np.ndarray:
    """`get_I_from_full_pairwise_tests(test="hsic")` through `hsic_tests`: I = {(i, j): p > alpha_eff}
    in the reference's pair order (alpha_eff = alpha / #pairs under Bonferroni; the same dtype and
    shape, the empty case included).  With perms="numpy" and undirected=True the p-values are
    `permutation_null`'s wherever no permuted value is within 4 tol (1 + tol) of the observed one.
    pvalue="chi2": the chi-square test's p-values, one evaluation a pair."""
    _, p = hsic_tests(X, pvalue=pvalue, num_perm=num_perm, seed=seed, perms=perms, tol=tol, device=device)
    return _I_from_pvalues(p, alpha, bonferroni, undirected, exclude_diagonal)


def summarize_I(I: np.ndarray, d: int, max_show: int = 10) -> None:
    I = np.asarray(I, dtype=int)
    print(f"I size: {len(I)} pairs (d={d})")
    if len(I) == 0:
        return
    print("first pairs:", I[:max_show].tolist(), ("..." if len(I) > max_show else ""))
