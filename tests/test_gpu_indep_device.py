"""The independence tests on a device-resident X and the device medians for the RBF bandwidths
(csrc/indep.hip: midagma_indep_set_data_dev, midagma_indep_median_bandwidths).

The medians must equal `mi_tests.median_sigma2` (numpy's np.median of the squared differences)
exactly; a device X must give the results of the host X bit for bit, and both stay within the bars
of tests/test_gpu_indep.py against the reference's recorded values (1e-12 on the statistics, counts
and p-values exact)."""
import numpy as np
import pytest

from tests import indep_median_numpy as imn
from tests import indep_numpy as inp
from midagma_amd import mi_tests as mi
from midagma_amd.solver import HipIndep

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("indep.npz")


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


def _case(fx, case):
    return fx[f"{case}/X"], fx[f"{case}/pairs"], int(fx[f"{case}/P"]), int(fx[f"{case}/seed"])


def _host_sigma2(X):
    return np.array([mi.median_sigma2(X[:, v]) for v in range(X.shape[1])])


@pytest.fixture(scope="module")
def host_null(fx):
    """(case, T) -> permutation_null on the host X, computed once."""
    cache = {}

    def get(case, T):
        if (case, T) not in cache:
            X, pairs, P, seed = _case(fx, case)
            cache[case, T] = mi.permutation_null(X, pairs, test=T, num_perm=P, seed=seed)
        return cache[case, T]

    return get


# ---- medians ------------------------------------------------------------------------------------

def _check_medians(X):
    want = _host_sigma2(X)
    d = X.shape[1]
    eng = HipIndep(X)
    try:
        got = eng.median_bandwidths()
        assert got.dtype == np.float64 and np.array_equal(got, want)
        assert np.array_equal(eng.median_bandwidths(), got)  # a second call: the same bits
        for cols in ([d - 1], list(range(0, d, 2)), [0, 0, d - 1]):
            sub = eng.median_bandwidths(cols)
            exp = np.ones(d)
            exp[cols] = want[cols]
            assert np.array_equal(sub, exp)
        assert np.array_equal(eng.median_bandwidths([]), np.ones(d))
    finally:
        eng.close()
    return want


@pytest.mark.parametrize("case", inp.CASES)
def test_medians_equal_numpy_on_the_fixtures(fx, case):
    _check_medians(fx[f"{case}/X"])


@pytest.mark.parametrize("n", SIZES)
def test_medians_equal_numpy_on_generated_columns(n):
    cols = imn.columns(n)
    X = np.column_stack([cols[k] for k in sorted(cols)])
    want = _check_medians(X)
    names = sorted(cols)
    assert want[names.index("constant")] == 1.0 and want[names.index("signed_zero")] == 1.0


def _median_from_counts(values, counts):
    """np.median of the multiset {values[k]^2 with multiplicity counts[k]}, values ascending."""
    cum = np.cumsum(counts)
    M = int(cum[-1])
    at = lambda k: float(values[np.searchsorted(cum, k + 1)]) ** 2  # element k, from 0
    return at(M // 2) if M & 1 else (at(M // 2 - 1) + at(M // 2)) / 2.0


def test_medians_at_the_cap_equal_the_exact_count_based_median():
    """n = 16384 (the whole 128 KiB of LDS) without the 1 GB host array: for integer columns the
    multiset of differences follows from counts."""
    n = HipIndep.MAX_N
    rng = np.random.default_rng(5)
    a = rng.permutation(n).astype(np.float64)             # |difference| k occurs n - k times
    b = rng.integers(0, 64, size=n).astype(np.float64)    # a 64-bin histogram's correlation
    k = np.arange(1, n)
    want_a = _median_from_counts(k, n - k)
    h = np.bincount(b.astype(np.int64), minlength=64).astype(np.int64)
    cnt = np.array([(h * (h - 1) // 2).sum()] + [(h[:-s] * h[s:]).sum() for s in range(1, 64)])
    assert cnt.sum() == n * (n - 1) // 2
    want_b = _median_from_counts(np.arange(64), cnt)
    eng = HipIndep(np.column_stack([a, b]))
    try:
        got = eng.median_bandwidths()
        assert np.array_equal(got, [want_a, want_b])
        assert np.array_equal(eng.median_bandwidths([1]), [1.0, want_b])
    finally:
        eng.close()


# ---- device X equals host X ---------------------------------------------------------------------

@pytest.mark.parametrize("T", inp.STATS)
@pytest.mark.parametrize("case", inp.CASES)
def test_device_x_equals_host_x_and_the_reference(fx, torch_, host_null, case, T):
    X, pairs, P, seed = _case(fx, case)
    Xd = torch_.as_tensor(X).cuda()
    keep = Xd.clone()
    stat, ge, null = mi.permutation_null(Xd, pairs, test=T, num_perm=P, seed=seed)
    hs, hg, hn = host_null(case, T)
    assert np.array_equal(stat, hs) and np.array_equal(ge, hg) and np.array_equal(null, hn)
    dev = max(np.abs(stat - fx[f"{case}/{T}/stat"]).max(), np.abs(null - fx[f"{case}/{T}/null"]).max())
    print(f"{case} {T}: device X vs reference, max abs deviation {dev:.3e}")
    assert dev <= 1e-12
    assert np.array_equal(ge, fx[f"{case}/{T}/ge"])
    res = mi.test_pairwise_independence(Xd, [tuple(p) for p in pairs.tolist()], test=T, num_perm=P, seed=seed)
    assert np.array_equal([r.pvalue for r in res], fx[f"{case}/{T}/pvalue"])
    assert np.array_equal([r.stat for r in res], stat)
    assert torch_.equal(Xd, keep)


@pytest.mark.parametrize("T", inp.STATS)
def test_get_I_on_a_device_x_matches_the_reference(fx, torch_, T):
    X, _, P, seed = _case(fx, "c96")
    Xd = torch_.as_tensor(X).cuda()
    for b in (0, 1):
        for u in (0, 1):
            I = mi.get_I_from_full_pairwise_tests(Xd, alpha=0.05, test=T, num_perm=P, seed=seed, bonferroni=bool(b),
                                                  undirected=bool(u))
            assert np.array_equal(I.reshape(-1, 2), fx[f"c96/{T}/I_b{b}_u{u}"])


@pytest.mark.parametrize("T", inp.STATS)
def test_strided_view_bandwidth_modes_and_device_permutations(fx, torch_, T):
    X, pairs, P, seed = _case(fx, "c97")
    n, d = X.shape
    Xd = torch_.as_tensor(X).cuda()
    big = torch_.full((n, d + 3), 7.0, dtype=torch_.float64, device="cuda")
    big[:, :d] = Xd
    view = big[:, :d]
    assert view.stride() == (d + 3, 1)
    keep = big.clone()
    base = mi.permutation_null(Xd, pairs, test=T, num_perm=P, seed=seed)
    for other in (mi.permutation_null(view, pairs, test=T, num_perm=P, seed=seed),
                  mi.permutation_null(Xd.t().contiguous().t(), pairs, test=T, num_perm=P, seed=seed),  # column-major
                  mi.permutation_null(Xd, pairs, test=T, num_perm=P, seed=seed, bandwidths="host"),
                  mi.permutation_null(X, pairs, test=T, num_perm=P, seed=seed, bandwidths="host")):
        for x, y in zip(base, other):
            assert np.array_equal(x, y)
    assert torch_.equal(big, keep)
    dd = mi.permutation_null(Xd, pairs, test=T, num_perm=P, seed=seed, perms="device")
    dh = mi.permutation_null(X, pairs, test=T, num_perm=P, seed=seed, perms="device")
    for x, y in zip(dd, dh):
        assert np.array_equal(x, y)
    # the engine itself: the medians of the view are the host's
    eng = HipIndep(view)
    try:
        assert (eng.n, eng.d) == (n, d)
        assert np.array_equal(eng.median_bandwidths(), _host_sigma2(X))
    finally:
        eng.close()


def test_single_statistics_on_device_columns(fx, torch_):
    X = fx["c97/X"]
    x, y = torch_.as_tensor(X[:, 0]).cuda(), torch_.as_tensor(X[:, 1]).cuda()
    assert mi.hsic_stat(x, y) == mi.hsic_stat(X[:, 0], X[:, 1])
    assert mi.dcor_stat(x, y) == mi.dcor_stat(X[:, 0], X[:, 1])
    s0 = np.sqrt(mi.median_sigma2(X[:, 0]))
    assert mi.hsic_stat(x, y, s0, None) == mi.hsic_stat(X[:, 0], X[:, 1], s0, None)
    assert mi.hsic_stat(x, X[:, 1]) == mi.hsic_stat(X[:, 0], X[:, 1])
    q = fx["c97/pairs"].tolist().index([0, 1])
    assert abs(mi.hsic_stat(x, y) - fx["c97/hsic/stat"][q]) <= 1e-12
    # pearson and spearman take the host copy
    res_d = mi.test_pairwise_independence(torch_.as_tensor(X).cuda(), [(0, 1), (1, 2)], test="spearman")
    assert res_d == mi.test_pairwise_independence(X, [(0, 1), (1, 2)], test="spearman")


# ---- ordering -----------------------------------------------------------------------------------

def test_x_produced_on_a_side_stream_needs_no_synchronise(torch_):
    from midagma_amd import utils
    d, n = 8, 4096
    W = np.triu(np.random.default_rng(2).uniform(0.5, 1.5, (d, d)), k=1)
    pairs = [(0, 1), (2, 7), (5, 3)]
    side = torch_.cuda.Stream()
    with torch_.cuda.stream(side):
        Xd = utils.simulate_linear_sem_gpu(W, n, "gauss", seed=11)
        eng = HipIndep(Xd)  # no synchronise: the library orders itself behind the producer
    try:
        s2 = eng.median_bandwidths()
        hs = eng.run("hsic", pairs, 8, None, seed=3, return_null=True)
        dc = eng.run("dcor", pairs, 8, None, seed=3, return_null=True)
    finally:
        eng.close()
    torch_.cuda.synchronize()
    eng = HipIndep(Xd)
    try:
        assert np.array_equal(eng.median_bandwidths(), s2)
        for T, first in (("hsic", hs), ("dcor", dc)):
            for x, y in zip(first, eng.run(T, pairs, 8, None, seed=3, return_null=True)):
                assert np.array_equal(x, y)
    finally:
        eng.close()
    Xh = Xd.cpu().numpy()
    assert np.array_equal(s2[:2], [mi.median_sigma2(Xh[:, 0]), mi.median_sigma2(Xh[:, 1])])


# ---- errors -------------------------------------------------------------------------------------

def test_error_paths(torch_):
    X = np.random.default_rng(0).standard_normal((10, 3))
    Xd = torch_.as_tensor(X).cuda()
    for bad_value in (float("nan"), float("inf"), float("-inf")):
        bad = Xd.clone()
        bad[7, 2] = bad_value
        with pytest.raises(ValueError):
            HipIndep(bad)
        for T in inp.STATS:
            with pytest.raises(ValueError):
                mi.permutation_null(bad, [(0, 1)], test=T, num_perm=2)
        eng = HipIndep(Xd)
        try:
            want = eng.run("dcor", [(0, 1)], 3, None, seed=1)
            with pytest.raises(ValueError):
                eng.set_data(bad)
            # the engine holds no data now: every entry refuses, nothing runs on the rejected X
            with pytest.raises(ValueError):
                eng.run("dcor", [(0, 1)], 3, None, seed=1)
            with pytest.raises(ValueError):
                eng.median_bandwidths()
            with pytest.raises(ValueError):
                eng.set_bandwidths([1.0, 1.0, 1.0])
            eng.set_data(Xd)
            for x, y in zip(want, eng.run("dcor", [(0, 1)], 3, None, seed=1)):
                assert np.array_equal(x, y)
        finally:
            eng.close()
    with pytest.raises(ValueError):
        HipIndep(Xd.float())
    with pytest.raises(ValueError):
        HipIndep(Xd.reshape(5, 2, 3))
    with pytest.raises(ValueError):
        HipIndep(Xd[:1])
    with pytest.raises(ValueError):
        HipIndep(torch_.zeros((16385, 2), dtype=torch_.float64, device="cuda"))
    for T in inp.STATS:
        with pytest.raises(ValueError):
            mi.test_pairwise_independence(Xd.float(), [(0, 1)], test=T)
        with pytest.raises(ValueError):
            mi.test_pairwise_independence(Xd[:1], [(0, 1)], test=T)
        with pytest.raises(ValueError):
            mi.test_pairwise_independence(Xd, [(0, 3)], test=T)
    with pytest.raises(ValueError):
        mi.permutation_null(X, [(0, 1)], bandwidths="gpu")
    with pytest.raises(ValueError):
        mi.permutation_null(Xd, [(0, 1)], bandwidths="numpy")
    eng = HipIndep(X)
    try:
        with pytest.raises(ValueError):
            eng.median_bandwidths([3])
        with pytest.raises(ValueError):
            eng.median_bandwidths([-1])
        assert np.array_equal(eng.median_bandwidths(), _host_sigma2(X))
    finally:
        eng.close()
