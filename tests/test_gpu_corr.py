"""csrc/corr.hip on the GPU: the column ranks bit-equal to the numpy restatement
(tests/corr_numpy.py, itself equal to scipy.stats.rankdata in tests/test_corr_cpu.py), and
`mi_tests.correlation_tests` / `get_I_from_correlation_tests` against the reference's recorded
results (tests/golden/corr.npz, and c97 of indep.npz).

Rank inputs (corr_numpy.rank_input), each at n in {2, 3, 64, 65, 257, 1025, 4097, 70001} and d in
{1, 5, 67}, read through a row stride above d, under two scratch budgets:
    normal            the ordinary case
    small_ints        integers 0..3: heavy ties
    constant          one constant column: a tie run of length n, every digit pass skipped
    zeros_denormals   +0.0, -0.0 and +- denormals: the key canonicalisation
    huge_range        1e-300 .. 1e300 with both signs: every digit pass live
    scaled_primes     {1, 2, 3, 5, 7} x 2^k: equal low digits, distinct high ones (an unstable pass)
    sorted, reversed  order-dependent bugs
    last_bit          neighbours that differ in the last mantissa bit: the lowest digit
and n = 1 000 003, d = 2 (one constant column): bucket counts above 2^16, a tie run of length n.

Bars against the reference: stat within 1e-12; p within relative 1e-11 max(1, n |r| / (1 - r^2))
where the reference's p >= 1e-290, and <= 1e-280 where it is 0 or below 1e-290; the diagonal and the
constant columns by rule; every stored I exactly.  Measured maxima: DESIGN.md, "Ranks and
correlations"."""
import numpy as np
import pytest

from tests import corr_numpy as cn
from midagma_amd import mi_tests as mi
from midagma_amd import solver

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


@pytest.fixture(scope="module")
def fx(golden):
    return golden("corr.npz")


@pytest.fixture(scope="module")
def fx_indep(golden):
    return golden("indep.npz")


def _wide(torch, X, pad=3):
    """X as a column slice of a wider device tensor (row stride d + pad), and the wide tensor."""
    n, d = X.shape
    wide = torch.full((n, d + pad), 7.25, dtype=torch.float64, device="cuda")
    wide[:, 1:d + 1] = torch.from_numpy(X).cuda()
    return wide[:, 1:d + 1], wide


# ---- ranks ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", cn.RANK_KINDS)
def test_ranks_equal_the_restatement(torch_, kind):
    for n in cn.RANK_N:
        for d in cn.RANK_D:
            X = cn.rank_input(kind, n, d)
            want = cn.column_ranks(X)
            Xd, wide = _wide(torch_, X)
            before = wide.clone()
            assert Xd.stride(0) == d + 3
            got = solver.column_ranks(Xd)
            small = solver.column_ranks(Xd, budget_bytes=3 * 25 * n)  # two or three columns a chunk
            assert got.shape == (n, d) and got.dtype == torch_.float64 and got.is_cuda
            assert np.array_equal(got.cpu().numpy(), want), (kind, n, d)
            assert torch_.equal(got, small), (kind, n, d)
            assert torch_.equal(wide, before), (kind, n, d)  # X (and its neighbours) unchanged
    assert np.array_equal(solver.column_ranks(X).cpu().numpy(), want)  # a host X is uploaded


def test_ranks_at_a_million_rows(torch_):
    n = 1_000_003
    X = np.random.default_rng(11).standard_normal((n, 2))
    X[:, 0] = -3.5
    Xd = torch_.from_numpy(X).cuda()
    got = solver.column_ranks(Xd)
    again = solver.column_ranks(Xd, budget_bytes=30 * n)  # one column a chunk
    assert (got[:, 0] == (n + 1) / 2).all()
    assert np.array_equal(got.cpu().numpy(), cn.column_ranks(X))
    assert torch_.equal(got, again)
    assert np.array_equal(Xd.cpu().numpy(), X)


# ---- correlations and pair sets -------------------------------------------------------------------

def _reference(fx, fx_indep, case, T):
    """(X, stat_ref, p_ref) as d x d matrices (NaN where c97's pair list has no entry)."""
    if case != "c97":
        return fx[f"{case}/X"], fx[f"{case}/{T}/stat"], fx[f"{case}/{T}/pvalue"]
    X, pairs = fx_indep["c97/X"], fx_indep["c97/pairs"]
    d = X.shape[1]
    i, j = pairs[:, 0], pairs[:, 1]
    S, P = np.full((d, d), np.nan), np.full((d, d), np.nan)
    S[i, j], P[i, j] = fx_indep[f"c97/{T}/stat"], fx_indep[f"c97/{T}/pvalue"]
    S[j, i], P[j, i] = S[i, j], P[i, j]
    np.fill_diagonal(S, 1.0), np.fill_diagonal(P, 0.0)
    assert np.isfinite(S).all() and np.isfinite(P).all()
    return X, S, P


@pytest.mark.parametrize("T", cn.TESTS)
@pytest.mark.parametrize("case", cn.CASES + ("c97",))
def test_correlation_tests_match_the_reference(torch_, fx, fx_indep, case, T):
    X, stat_ref, p_ref = _reference(fx, fx_indep, case, T)
    n, d = X.shape
    X0 = X.copy()
    stat, p = mi.correlation_tests(X, test=T)
    Xd, wide = _wide(torch_, X)
    before = wide.clone()
    stat_d, p_d = mi.correlation_tests(Xd, test=T)
    assert np.array_equal(stat, stat_d, equal_nan=True) and np.array_equal(p, p_d, equal_nan=True)
    assert np.array_equal(X, X0) and torch_.equal(wide, before)
    assert stat.shape == p.shape == (d, d) and stat.dtype == p.dtype == np.float64
    const = X.max(axis=0) == X.min(axis=0)
    _, const_d = solver.correlation(Xd, ranks=(T == "spearman"))
    assert const_d.dtype == bool and np.array_equal(const_d, const)
    serr, ratio = cn.check_against_reference(stat, p, stat_ref, p_ref, n, const, T)
    print(f"\n{case} {T}: max |stat - ref| = {serr:.3e}, max p error / bar = {ratio:.3e}")


@pytest.mark.parametrize("T", cn.TESTS)
@pytest.mark.parametrize("case", cn.CASES)
def test_pair_sets_equal_the_reference(torch_, fx, case, T):
    X = fx[f"{case}/X"]
    Xd = torch_.from_numpy(X).cuda()
    for b in (0, 1):
        for u in (0, 1):
            want = fx[f"{case}/{T}/I_b{b}_u{u}"]
            for src in (X, Xd):
                I = mi.get_I_from_correlation_tests(src, alpha=cn.ALPHA, test=T, bonferroni=bool(b),
                                                    undirected=bool(u))
                assert I.dtype == np.asarray([], dtype=int).dtype
                assert np.array_equal(I.reshape(-1, 2), want), (b, u)


def test_pair_set_shapes(torch_):
    X = np.random.default_rng(3).standard_normal((50, 3))
    X[:, 1] = X[:, 0]
    X[:, 2] = -X[:, 0]
    I = mi.get_I_from_correlation_tests(X)  # every pair rejected: the reference's empty array
    assert I.shape == (0,) and I.dtype == np.asarray([], dtype=int).dtype
    X = np.random.default_rng(4).standard_normal((50, 3))
    I = mi.get_I_from_correlation_tests(X, alpha=1e-9, undirected=False, exclude_diagonal=False)
    assert I.tolist() == [[0, 1], [0, 2], [1, 0], [1, 2], [2, 0], [2, 1]]  # the diagonal has p = 0


# ---- errors ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("v", [np.nan, np.inf, -np.inf])
def test_non_finite_device_x_raises(torch_, v):
    X = np.random.default_rng(0).standard_normal((300, 5))
    X[211, 3] = v
    Xd = torch_.from_numpy(X).cuda()
    with pytest.raises(ValueError):
        solver.column_ranks(Xd)
    with pytest.raises(ValueError):
        solver.correlation(Xd)
    for T in cn.TESTS:
        with pytest.raises(ValueError):
            mi.correlation_tests(Xd, test=T)
        with pytest.raises(ValueError):
            mi.get_I_from_correlation_tests(Xd, test=T)
    assert np.array_equal(Xd.cpu().numpy(), X, equal_nan=True)
