"""csrc/indep.hip on the GPU against the reference's recorded results (tests/golden/indep.npz, made
by tests/golden/make_indep.py; certified on the CPU by tests/test_indep_cpu.py).

The bar on the statistics is 1e-12 absolute: both lie in [0, 1] here and each is a mean of n^2
terms carrying a few ulp each, so the error bound is around 1e-15; the counts and p-values must be
exactly the reference's (the fixture keeps every permuted value at least 1e-6 relative away from
the observed one)."""
import numpy as np
import pytest

from tests import indep_numpy as inp
from midagma_amd import mi_tests as mi
from midagma_amd.solver import HipIndep

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(golden):
    return golden("indep.npz")


def _case(fx, case):
    return fx[f"{case}/X"], fx[f"{case}/pairs"], int(fx[f"{case}/P"]), int(fx[f"{case}/seed"])


def _engine(X, T):
    eng = HipIndep(X)
    if T == "hsic":
        eng.set_bandwidths([mi.median_sigma2(X[:, v]) for v in range(X.shape[1])])
    return eng


@pytest.mark.parametrize("T", inp.STATS)
@pytest.mark.parametrize("case", inp.CASES)
def test_statistics_counts_and_pvalues_match_the_reference(fx, case, T):
    X, pairs, P, seed = _case(fx, case)
    X0 = X.copy()
    stat, ge, null = mi.permutation_null(X, pairs, test=T, num_perm=P, seed=seed)
    dev = max(np.abs(stat - fx[f"{case}/{T}/stat"]).max(), np.abs(null - fx[f"{case}/{T}/null"]).max())
    print(f"{case} {T}: GPU vs reference, max abs deviation {dev:.3e}")
    assert dev <= 1e-12
    assert np.array_equal(ge, fx[f"{case}/{T}/ge"])
    res = mi.test_pairwise_independence(X, [tuple(p) for p in pairs.tolist()], test=T, num_perm=P, seed=seed)
    assert [(r.i, r.j) for r in res] == [tuple(p) for p in pairs.tolist()]
    assert np.array_equal([r.pvalue for r in res], fx[f"{case}/{T}/pvalue"])
    assert np.array_equal([r.stat for r in res], stat)
    assert np.array_equal(X, X0)


@pytest.mark.parametrize("T", inp.STATS)
def test_get_I_matches_the_reference(fx, T):
    X, _, P, seed = _case(fx, "c96")
    sizes = set()
    for b in (0, 1):
        for u in (0, 1):
            I = mi.get_I_from_full_pairwise_tests(X, alpha=0.05, test=T, num_perm=P, seed=seed, bonferroni=bool(b),
                                                  undirected=bool(u))
            want = fx[f"c96/{T}/I_b{b}_u{u}"]
            assert I.dtype == np.asarray([], dtype=int).dtype
            assert I.shape == (len(want), 2) or (len(want) == 0 and I.size == 0)
            assert np.array_equal(I.reshape(-1, 2), want)
            sizes.add(len(want))
    assert len(sizes) > 1  # the flags select different sets here


def test_get_I_empty_result_is_an_empty_int_array(fx):
    X = fx["c96/X"][:, :3]  # x0, sin(3 x0), 0.9 x0: every pair dependent
    I = mi.get_I_from_full_pairwise_tests(X, alpha=0.5, test="dcor", num_perm=19, seed=0, bonferroni=False)
    assert I.size == 0 and I.dtype == np.asarray([], dtype=int).dtype


@pytest.mark.parametrize("T", inp.STATS)
def test_constant_column_gives_stat_0_and_p_1(fx, T):
    X, _, P, seed = _case(fx, "c96")
    res = mi.test_pairwise_independence(X, [(3, 0), (0, 3), (3, 3)], test=T, num_perm=P, seed=seed)
    assert all(r.stat == 0.0 and r.pvalue == 1.0 for r in res)
    stat, ge, null = mi.permutation_null(X, [(3, 1)], test=T, num_perm=P, seed=seed, perms="device")
    assert stat[0] == 0.0 and ge[0] == P and (null == 0.0).all()


def test_single_statistics(fx):
    X = fx["c97/X"]
    q = fx["c97/pairs"].tolist().index([0, 1])
    assert abs(mi.hsic_stat(X[:, 0], X[:, 1]) - fx["c97/hsic/stat"][q]) <= 1e-12
    assert abs(mi.dcor_stat(X[:, 0], X[:, 1]) - fx["c97/dcor/stat"][q]) <= 1e-12
    s0, s1 = np.sqrt(mi.median_sigma2(X[:, 0])), np.sqrt(mi.median_sigma2(X[:, 1]))
    assert abs(mi.hsic_stat(X[:, 0], X[:, 1], s0, s1) - fx["c97/hsic/stat"][q]) <= 1e-12
    # sigma <= 0 means sigma^2 = 1 (the reference's rule)
    assert mi.hsic_stat(X[:, 0], X[:, 1], 0.0, -2.0) == mi.hsic_stat(X[:, 0], X[:, 1], 1.0, 2.0) != 0.0
    assert mi.dcor_stat(X[:, 0], np.full(97, 2.0)) == 0.0 == mi.hsic_stat(np.full(97, 2.0), X[:, 0])


@pytest.mark.parametrize("T", inp.STATS)
def test_runs_and_batch_budgets_are_bit_identical(fx, T):
    X, pairs, P, seed = _case(fx, "c200")
    m, n = len(pairs), X.shape[0]
    perms = inp.numpy_perms(seed, m, P, n).astype(np.int32)
    eng = _engine(X, T)
    try:
        # budgets that force 1, 2 and all pairs per batch
        one = 1
        per_pair = next(b for b in range(1 << 10, 1 << 30, 1 << 10) if eng.batch_pairs(P, b) >= 2) // 2
        two = 2 * per_pair + per_pair // 2
        huge = 1 << 32
        assert eng.batch_pairs(P, one) == 1 and eng.batch_pairs(P, two) == 2 and eng.batch_pairs(P, huge) >= m
        base = eng.run(T, pairs, P, perms, budget_bytes=huge, return_null=True)
        again = eng.run(T, pairs, P, perms, budget_bytes=huge, return_null=True)
        for b in (one, two):
            other = eng.run(T, pairs, P, perms, budget_bytes=b, return_null=True)
            for x, y in zip(base, other):
                assert np.array_equal(x, y)
        for x, y in zip(base, again):
            assert np.array_equal(x, y)
        # a pair's results do not depend on its neighbours in the call
        solo = eng.run(T, pairs[4:5], P, perms[4:5], return_null=True)
        assert solo[0][0] == base[0][4] and solo[1][0] == base[1][4] and np.array_equal(solo[2][0], base[2][4])
        # device permutations: a pair's permutations depend on its index, not on the batch split
        d1 = eng.run(T, pairs, P, None, seed=7, budget_bytes=one, return_null=True, return_perms=True)
        d2 = eng.run(T, pairs, P, None, seed=7, budget_bytes=huge, return_null=True, return_perms=True)
        for x, y in zip(d1, d2):
            assert np.array_equal(x, y)
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["c5", "c97", "c1000"])
def test_device_permutations(fx, case):
    """The device's permutations equal the numpy Philox restatement, and the statistics under
    perms='device' equal a run fed those permutations through the explicit array, bit for bit."""
    X, pairs, P, _ = _case(fx, case)
    seed = (0x9E3779B9 << 32) | 20240607  # both key words in use
    m, n = len(pairs), X.shape[0]
    want = inp.philox_perms(seed, m, P, n)
    for T in inp.STATS:
        eng = _engine(X, T)
        try:
            stat, ge, null, perms = eng.run(T, pairs, P, None, seed=seed, return_null=True, return_perms=True)
            assert perms.dtype == np.int32 and np.array_equal(perms, want)
            stat2, ge2, null2 = eng.run(T, pairs, P, perms, return_null=True)
        finally:
            eng.close()
        assert np.array_equal(stat, stat2) and np.array_equal(ge, ge2) and np.array_equal(null, null2)
        if T == "hsic":  # (dcor counts by dcov^2, before the square roots)
            assert np.array_equal(ge, (null >= stat[:, None]).sum(axis=1))
        # the observed statistic does not depend on the permutation source
        assert np.abs(stat - fx[f"{case}/{T}/stat"]).max() <= 1e-12
        s3, g3, n3 = mi.permutation_null(X, pairs, test=T, num_perm=P, seed=seed, perms="device")
        assert np.array_equal(s3, stat) and np.array_equal(g3, ge) and np.array_equal(n3, null)


def test_error_paths():
    X = np.random.default_rng(0).standard_normal((10, 3))
    bad = X.copy()
    bad[2, 2] = np.inf
    for T in inp.STATS:
        with pytest.raises(ValueError):
            mi.test_pairwise_independence(bad, [(0, 1)], test=T)
        with pytest.raises(ValueError):
            mi.test_pairwise_independence(X[:1], [(0, 1)], test=T)
        with pytest.raises(ValueError):
            mi.test_pairwise_independence(X, [(0, 3)], test=T)
        with pytest.raises(ValueError):
            mi.test_pairwise_independence(X, [(-1, 0)], test=T)
        with pytest.raises(ValueError):
            mi.test_pairwise_independence(np.zeros((16385, 2)), [(0, 1)], test=T)
    # the library's own checks, behind the Python ones
    eng = HipIndep(X)
    try:
        with pytest.raises(ValueError):
            eng.run("hsic", [(0, 1)], 2, seed=0)  # no bandwidths yet
        with pytest.raises(ValueError):
            eng.set_bandwidths([1.0, 0.0, 1.0])
        with pytest.raises(ValueError):
            eng.run("dcor", [(0, 3)], 2, seed=0)
        with pytest.raises(ValueError):
            eng.run("dcor", [(0, 1)], 1, np.full((1, 1, 10), 10, dtype=np.int32))  # index outside [0, n)
        stat, ge = eng.run("dcor", [(0, 1)], 0)
        assert ge[0] == 0 and 0.0 < stat[0] < 1.0
    finally:
        eng.close()
