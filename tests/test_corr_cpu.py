"""All-pairs Pearson / Spearman without a GPU: the numpy restatement of csrc/corr.hip
(tests/corr_numpy.py) against scipy and against the fixture tests/golden/corr.npz (made by
tests/golden/make_corr.py from the reference), the host p-value functions against scipy's own
per-pair p-values, the argument checks of the ABI, and the module surface."""
import ctypes as C
import inspect
import warnings

import numpy as np
import pytest
from scipy import stats

from tests import corr_numpy as cn
from midagma_amd import mi_tests as mi
from midagma_amd import solver


@pytest.fixture(scope="module")
def fx(golden):
    return golden("corr.npz")


@pytest.fixture(scope="module")
def fx_indep(golden):
    return golden("indep.npz")


def _restated(X, T):
    Z = cn.column_ranks(X) if T == "spearman" else X
    rho, const = cn.correlation(Z)
    return mi._stat_pvalue_from_rho(rho, const, X.shape[0], T) + (const,)


# ---- ranks ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", cn.RANK_KINDS)
def test_restated_ranks_equal_scipy(kind):
    for n in [n for n in cn.RANK_N if n <= 4097]:
        for d in (1, 5):
            X = cn.rank_input(kind, n, d)
            assert np.array_equal(cn.column_ranks(X), stats.rankdata(X, method="average", axis=0)), (kind, n, d)


def test_keys_order_and_zero():
    x = np.array([-np.inf, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1e300, np.inf])
    k = cn.keys(x)
    assert k[4] == k[5] and (np.diff(k[[0, 1, 2, 3, 4, 6, 7, 8, 9]].astype(object)) > 0).all()


# ---- correlations against the fixtures ------------------------------------------------------------

@pytest.mark.parametrize("T", cn.TESTS)
@pytest.mark.parametrize("case", cn.CASES)
def test_restated_tests_match_the_fixture(fx, case, T):
    X = fx[f"{case}/X"]
    n, d = X.shape
    stat, p, const = _restated(X, T)
    cn.check_against_reference(stat, p, fx[f"{case}/{T}/stat"], fx[f"{case}/{T}/pvalue"], n, const, T)
    for b in (0, 1):
        for u in (0, 1):
            pairs = cn.pair_index(d, bool(u))
            a = cn.ALPHA / len(pairs) if b else cn.ALPHA
            I = np.array([ij for ij in pairs if p[ij] > a], dtype=np.int64).reshape(-1, 2)
            assert np.array_equal(I, fx[f"{case}/{T}/I_b{b}_u{u}"]), (b, u)


@pytest.mark.parametrize("T", cn.TESTS)
def test_restated_tests_match_c97(fx_indep, T):
    X, pairs = fx_indep["c97/X"], fx_indep["c97/pairs"]
    stat, p, const = _restated(X, T)
    i, j = pairs[:, 0], pairs[:, 1]
    d = X.shape[1]
    S, P = np.full((d, d), np.nan), np.full((d, d), np.nan)
    S[i, j], P[i, j] = fx_indep[f"c97/{T}/stat"], fx_indep[f"c97/{T}/pvalue"]
    S[j, i], P[j, i] = S[i, j], P[i, j]
    np.fill_diagonal(S, 1.0), np.fill_diagonal(P, 0.0)
    assert not const.any() and np.isfinite(S).all()
    cn.check_against_reference(stat, p, S, P, X.shape[0], const, T)


@pytest.mark.parametrize("case", cn.CASES)
def test_margin_condition(fx, case):
    d = fx[f"{case}/X"].shape[1]
    for T in cn.TESTS:
        p = fx[f"{case}/{T}/pvalue"][~np.eye(d, dtype=bool)]
        p = p[np.isfinite(p)]
        for a in cn.alpha_effs(d):
            assert (np.abs(p - a) >= cn.MARGIN * a).all(), (T, a)
    if case == "m4097":
        for T in cn.TESTS:
            for b in (0, 1):
                for u in (0, 1):
                    assert 0 < len(fx[f"{case}/{T}/I_b{b}_u{u}"]) < len(cn.pair_index(d, bool(u)))


def test_constant_column_is_decided_on_raw_values(fx):
    X = fx["k257/X"]
    assert (X[:, 3] == 0.1).all()
    assert cn.correlation(X)[1].tolist() == [False, False, False, True, False, False]
    # in a summation order whose mean is not 0.1 the centred column is not zero: constant is max == min
    Y = np.column_stack([np.arange(10.0), np.full(10, 0.1)])
    mean = np.cumsum(Y[:, 1])[-1] / 10
    assert mean != 0.1 and np.abs(Y[:, 1] - mean).max() > 0
    assert cn.correlation(Y)[1].tolist() == [False, True]


# ---- the p-value functions ------------------------------------------------------------------------

def test_pvalue_functions_equal_scipy_bit_for_bit(fx):
    for case in cn.CASES:
        X = fx[f"{case}/X"]
        n, d = X.shape
        for i in range(d):
            for j in range(d):
                if i == j or np.ptp(X[:, i]) == 0 or np.ptp(X[:, j]) == 0:
                    continue
                r, p = stats.pearsonr(X[:, i], X[:, j])
                assert mi._pearson_pvalues(np.array([r]), n)[0] == p
                r, p = stats.spearmanr(X[:, i], X[:, j])
                assert mi._spearman_pvalues(np.array([r]), n)[0] == p


def test_rules_for_the_diagonal_and_constant_columns():
    rho = np.array([[1.0, 0.5, np.nan], [0.5, 1.0, np.nan], [np.nan, np.nan, np.nan]])
    const = np.array([False, False, True])
    s, p = mi._stat_pvalue_from_rho(rho, const, 30, "pearson")
    assert s[0, 0] == 1.0 and p[0, 0] == 0.0 and np.isnan(s[2]).all() and np.isnan(p[:, 2]).all()
    s, p = mi._stat_pvalue_from_rho(rho, const, 30, "spearman")
    assert s[1, 1] == 1.0 and p[1, 1] == 0.0 and (s[2] == 0.0).all() and (p[:, 2] == 1.0).all()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        X = np.random.default_rng(1).standard_normal((30, 2))
        (ref,) = mi.test_pairwise_independence(X, [(0, 1)], test="spearman")
    r = cn.correlation(cn.column_ranks(X))[0]
    s, p = mi._stat_pvalue_from_rho(r, np.zeros(2, bool), 30, "spearman")
    assert abs(s[0, 1] - ref.stat) <= 1e-15 and abs(p[0, 1] - ref.pvalue) <= 1e-12 * ref.pvalue


# ---- ABI ------------------------------------------------------------------------------------------

def test_corr_entry_points_validate_without_a_device():
    from midagma_amd import _lib
    L = _lib.load()
    assert L.midagma_abi_version() == 11  # the entries are additive
    for name in ("midagma_colrank", "midagma_corr", "midagma_corr_workspace"):
        assert name in _lib.EXPORTED
    x = C.c_void_p(4096)  # never dereferenced: every call below fails its argument checks first
    bad_shapes = [(1, 3, 3, 3), (1 << 31, 3, 3, 3), (10, 0, 3, 3), (10, 65536, 65536, 65536), (10, 3, 2, 3),
                  (10, 3, 3, 2)]
    for (n, d, ldx, ldo) in bad_shapes:
        assert L.midagma_colrank(x, n, d, ldx, x, ldo, 0, None) == -3, (n, d, ldx, ldo)
        assert L.midagma_corr(x, n, d, ldx, x, ldo, x, 0, None) == -3, (n, d, ldx, ldo)
    assert L.midagma_colrank(None, 10, 3, 3, x, 3, 0, None) == -3
    assert L.midagma_colrank(x, 10, 3, 3, None, 3, 0, None) == -3
    assert L.midagma_corr(None, 10, 3, 3, x, 3, x, 0, None) == -3
    assert L.midagma_corr(x, 10, 3, 3, None, 3, x, 0, None) == -3
    assert L.midagma_corr(x, 10, 3, 3, x, 3, None, 0, None) == -3
    assert b"null pointer" in L.midagma_last_error(None)
    for (n, d) in ((1, 3), (1 << 31, 3), (10, 0), (10, 65536)):
        assert L.midagma_corr_workspace(n, d, 0) == 0
    w = L.midagma_corr_workspace(1000, 10, 0)
    assert w >= 10 * 1000 * 24 and L.midagma_corr_workspace(1000, 10, 1) < w  # one column a chunk under a tiny budget
    assert L.midagma_corr_workspace(1000, 10, 1) >= 1000 * 24


# ---- module surface and errors --------------------------------------------------------------------

def test_module_surface_and_signatures():
    assert {"correlation_tests", "get_I_from_correlation_tests"} <= set(mi.__all__)
    assert {"column_ranks", "correlation"} <= set(solver.__all__)
    sig = inspect.signature(mi.correlation_tests)
    want = {"test": "pearson", "device": 0, "budget_bytes": 0}
    assert list(sig.parameters) == ["X"] + list(want)
    for k, v in want.items():
        assert sig.parameters[k].default == v and sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(mi.get_I_from_correlation_tests)
    want = {"alpha": 0.05, "test": "pearson", "bonferroni": True, "undirected": True, "exclude_diagonal": True,
            "device": 0}
    assert list(sig.parameters) == ["X"] + list(want)
    for k, v in want.items():
        assert sig.parameters[k].default == v and sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(solver.column_ranks)
    assert list(sig.parameters) == ["X", "budget_bytes"] and sig.parameters["budget_bytes"].default == 0
    sig = inspect.signature(solver.correlation)
    assert list(sig.parameters) == ["X", "ranks", "budget_bytes"]
    assert sig.parameters["ranks"].default is False and sig.parameters["budget_bytes"].default == 0
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("ranks", "budget_bytes"))
    assert "stay on the host" not in mi.__doc__ and "correlation_tests" in mi.__doc__


class _FakeDeviceTensor:
    """Looks like a float32 CUDA tensor to `is_device_tensor`; nothing may touch its memory."""

    class device:
        type = "cuda"
        index = 0

    def __init__(self):
        import torch
        self.dtype, self.shape = torch.float32, (10, 3)

    def data_ptr(self):
        raise AssertionError("the dtype check must come first")

    def dim(self):
        return 2


def test_bad_inputs_raise_value_error_before_any_device():
    X = np.random.default_rng(0).standard_normal((10, 3))
    for v in (np.nan, np.inf, -np.inf):
        bad = X.copy()
        bad[3, 1] = v
        for T in cn.TESTS:
            with pytest.raises(ValueError):
                mi.correlation_tests(bad, test=T)
            with pytest.raises(ValueError):
                mi.get_I_from_correlation_tests(bad, test=T)
        with pytest.raises(ValueError):
            solver.column_ranks(bad)
        with pytest.raises(ValueError):
            solver.correlation(bad)
    for fn in (mi.correlation_tests, mi.get_I_from_correlation_tests, solver.column_ranks, solver.correlation):
        with pytest.raises(ValueError):
            fn(X[:1])
        with pytest.raises(ValueError):
            fn(X.astype(np.float32))
        with pytest.raises(ValueError):
            fn(X[:, 0])
        with pytest.raises(ValueError):
            fn(_FakeDeviceTensor())
    for T in ("hsic", "dcor", "kendall"):
        with pytest.raises(ValueError):
            mi.correlation_tests(X, test=T)
        with pytest.raises(ValueError):
            mi.get_I_from_correlation_tests(X, test=T)


def test_there_is_no_cpu_path():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from midagma_amd._lib import HipSolverError
    X = np.random.default_rng(0).standard_normal((10, 3))
    with pytest.raises(HipSolverError):
        solver.column_ranks(X)
    with pytest.raises(HipSolverError):
        solver.correlation(X)
    for T in cn.TESTS:
        with pytest.raises(HipSolverError):
            mi.correlation_tests(X, test=T)
        with pytest.raises(HipSolverError):
            mi.get_I_from_correlation_tests(X, test=T)
