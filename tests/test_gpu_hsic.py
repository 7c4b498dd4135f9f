"""csrc/hsic.hip on the GPU: HSIC from low-rank factors against the reference's recorded results
(tests/golden/indep.npz), against tests/hsic_numpy.py (certified on the CPU by
tests/test_hsic_cpu.py), against the n^2 kernel of csrc/indep.hip, and the median bandwidths against
that kernel's and the counting restatement of tests/indep_median_numpy.py.

The bar on a statistic is 1e-12 + 4 eta absolute: tests/test_gpu_indep.py's rounding bar plus the
bound |HSIC_factored - HSIC| <= 4 eta (1 + eta) ("HSIC from low-rank factors").  Two
factorisations (the kernels' and the restatement's) are each within 4 eta of the n^2 sum, so they are
within 2 (4 eta) + 1e-12 of each other.  The recorded fixtures' smallest non-zero |null - stat| is
5.3e-8, so no count is excused."""
import ctypes as C

import numpy as np
import pytest

from midagma_amd import _lib
from midagma_amd import mi_tests as mi
from midagma_amd.solver import HipHsic, HipIndep
from tests import dcor_numpy as dn
from tests import hsic_numpy as hn
from tests import indep_median_numpy as imn
from tests import indep_numpy as inp

pytestmark = pytest.mark.gpu

ETA = 1e-13
BAR = 1e-12 + 4 * ETA
BAR2 = 1e-12 + 2 * (4 * ETA)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("indep.npz")


@pytest.mark.parametrize("case", inp.CASES)
def test_statistics_counts_and_pvalues_match_the_reference(fx, case):
    X, pairs, P, seed = fx[f"{case}/X"], fx[f"{case}/pairs"], int(fx[f"{case}/P"]), int(fx[f"{case}/seed"])
    X0 = X.copy()
    stat, ge, null = mi.hsic_null(X, pairs, num_perm=P, seed=seed, perms="numpy")
    dev = max(np.abs(stat - fx[f"{case}/hsic/stat"]).max(), np.abs(null - fx[f"{case}/hsic/null"]).max())
    print(f"{case}: GPU vs reference, max abs deviation {dev:.3e}")
    assert dev <= BAR
    assert np.array_equal(ge, fx[f"{case}/hsic/ge"])
    assert np.array_equal((ge + 1) / (P + 1), fx[f"{case}/hsic/pvalue"])
    assert np.array_equal(X, X0)


def test_get_I_matches_the_reference(fx):
    """The undirected sets are the reference's, and b1_u0 (tests/test_hsic_cpu.py); with
    undirected=False and no Bonferroni the reference's fresh permutations for (j, i) decide one pair
    differently, so the mirrored set is checked against the undirected one instead."""
    X, P, seed = fx["c96/X"], int(fx["c96/P"]), int(fx["c96/seed"])
    got = {}
    for b in (0, 1):
        for u in (0, 1):
            I = mi.get_I_from_hsic_tests(X, alpha=0.05, num_perm=P, seed=seed, perms="numpy", bonferroni=bool(b),
                                         undirected=bool(u))
            assert I.dtype == np.asarray([], dtype=int).dtype
            got[b, u] = I.reshape(-1, 2)
    for b, u in ((0, 1), (1, 1), (1, 0)):
        assert np.array_equal(got[b, u], fx[f"c96/hsic/I_b{b}_u{u}"]), (b, u)
    both = sorted(map(tuple, np.concatenate([got[0, 1], got[0, 1][:, ::-1]]).tolist()))
    assert sorted(map(tuple, got[0, 0].tolist())) == both
    assert len({len(v) for v in got.values()}) > 1  # the flags select different sets here
    I = mi.get_I_from_hsic_tests(fx["c96/X"][:, :3], alpha=0.5, num_perm=19, seed=0, perms="numpy", bonferroni=False)
    assert I.size == 0 and I.dtype == np.asarray([], dtype=int).dtype


# (n, chunk): 0 the rule; 64 puts n at chunk - 1, chunk and chunk + 1; 16 at n = 257 makes 17 chunks
@pytest.mark.parametrize("n,chunk", [(2, 0), (3, 0), (5, 16), (63, 64), (64, 64), (65, 64), (257, 16), (257, 0),
                                     (4097, 0), (4097, 1024)])
def test_shapes_match_the_restatement(n, chunk):
    P = 5  # (the identity and 5 permutations: a full group of 4 and a ragged one)
    X = hn.data(n)
    X0 = X.copy()
    rng = np.random.default_rng(n)
    perms = np.array([[rng.permutation(n) for _ in range(P)] for _ in hn.ALL_PAIRS_5], dtype=np.int32)
    ws, wg, wn, ranks = hn.hsic_null(X, hn.ALL_PAIRS_5, perms)
    stat, ge, null = mi.hsic_null(X, hn.ALL_PAIRS_5, num_perm=P, perms=perms, chunk=chunk)
    dev = max(np.abs(stat - ws).max(), np.abs(null - wn).max())
    print(f"n={n} chunk={chunk}: GPU vs restatement, max abs deviation {dev:.3e}, ranks {sorted(ranks.values())}")
    assert dev <= BAR2
    for q, (i, j) in enumerate(hn.ALL_PAIRS_5):
        if j == 4:  # the constant column
            assert stat[q] == 0.0 and ge[q] == P and not null[q].any()
    assert np.array_equal(X, X0)


def _factor_checks(eng, X, sigma2, cols, eta=ETA):
    rank, resid = eng.factor(cols, eta)
    assert (resid <= eta).all() and (rank <= 256).all() and (rank >= 1).all()
    worst = 0.0
    if eng.n <= 257:
        for k, v in enumerate(cols):
            Fc, mean = eng.get_factor(v, rank[k])
            assert not Fc[:, rank[k]:].any() and not mean[rank[k]:].any()
            F = Fc + mean
            worst = max(worst, np.abs(hn.gram(X[:, v], sigma2[v]) - F @ F.T).max())
        assert worst <= eta + 1e-14
    return rank, resid, worst


@pytest.mark.parametrize("n", [5, 97, 257])
def test_factors_reproduce_the_gram_matrix(n):
    X = hn.data(n)
    eng = HipHsic(X)
    try:
        s2 = eng.median_bandwidths()
        rank, resid, worst = _factor_checks(eng, X, s2, np.arange(5))
        print(f"n={n}: ranks {rank.tolist()}, max|K - F F^T| {worst:.3e}, largest residual {resid.max():.3e}")
        Fc, _ = eng.get_factor(4, rank[4])  # the zero-range column
        assert rank[4] == 1 and not Fc.any()
        for eta in (1e-14, 1e-6, 1e-3):
            _factor_checks(eng, X, s2, np.arange(5), eta)
    finally:
        eng.close()


def test_forced_ranks():
    X = np.ascontiguousarray(np.tile(hn.data(300)[:, :1], (1, len(hn.FORCED_RANKS))))
    want = np.array(list(hn.FORCED_RANKS))
    s2 = np.array([hn.FORCED_RANKS[r] for r in want])
    assert sorted(want.tolist()) == [1, 15, 16, 17, 33, 70]  # r_pad 16, 16, 16, 32, 48 and 80: every tile edge
    d = len(want)
    pairs = [(i, j) for i in range(d) for j in range(d) if i != j]  # both orders: rank r_x != r_y both ways
    P = 2
    rng = np.random.default_rng(3)
    perms = np.array([[rng.permutation(300) for _ in range(P)] for _ in pairs], dtype=np.int32)
    eng = HipHsic(X[:257])
    try:
        eng.set_bandwidths(s2)
        _factor_checks(eng, X[:257], s2, np.arange(d))
        eng.set_data(X)
        eng.set_bandwidths(s2)
        rank, resid = eng.factor(np.arange(d))
        assert np.array_equal(rank, want) and (resid <= ETA).all()
        stat, ge, null = eng.run(pairs, P, perms, return_null=True)
    finally:
        eng.close()
    ws, wg, wn, _ = hn.hsic_null(X, pairs, perms, sigma2=s2)
    dev = max(np.abs(stat - ws).max(), np.abs(null - wn).max())
    print(f"forced ranks {rank.tolist()}: GPU vs restatement, max abs deviation {dev:.3e}")
    assert dev <= BAR2
    assert np.array_equal(ge, wg)


def test_full_rank_and_the_rank_cap():
    x = np.random.default_rng(5).standard_normal(300)
    X = np.ascontiguousarray(np.column_stack([x, x]))
    eng = HipHsic(X[:97])
    try:
        eng.set_bandwidths([1e-12, 1.0])  # K of column 0 is the identity to rounding
        rank, resid = eng.factor([0, 1])
        assert rank[0] == 97 and resid[0] <= ETA and rank[1] < 40
        stat, _ = eng.run([(0, 1), (0, 0)], 0)
        want, _, _, _ = hn.hsic_null(X[:97], [(0, 1), (0, 0)], None, sigma2=[1e-12, 1.0])
        assert np.abs(stat - want).max() <= BAR2
        eng.set_data(X)
        eng.set_bandwidths([1.0, 1e-12])
        with pytest.raises(ValueError, match=r"column 1 needs a rank above 256 .*rank 256, residual"):
            eng.run([(0, 1)], 0)
        with pytest.raises(ValueError, match="column 1 "):
            eng.factor([1])
        rank, _ = eng.factor([0])  # the other column is as before
        assert 1 < rank[0] < 40
    finally:
        eng.close()


@pytest.mark.parametrize("n", [5, 97, 1000, 16384])
def test_median_bandwidths_are_the_n2_engines_bits(n):
    cols = imn.columns(n)
    X = np.ascontiguousarray(np.column_stack(list(cols.values())))
    old = HipIndep(X)
    eng = HipHsic(X)
    try:
        want = old.median_bandwidths()
        got = eng.median_bandwidths()
        assert np.array_equal(got, want), list(zip(cols, got, want))
        assert got[list(cols).index("constant")] == 1.0
        some = eng.median_bandwidths([5, 1, 1])  # a list: the others are 1.0
        assert np.array_equal(some[[1, 5]], want[[1, 5]]) and (some[[0, 2, 3, 4, 6]] == 1.0).all()
    finally:
        old.close()
        eng.close()


def test_median_bandwidths_beyond_the_n2_cap():
    n = 70001
    cols = imn.columns(n)
    names = ("normal", "tied", "constant", "two_valued")
    X = np.ascontiguousarray(np.column_stack([cols[k] for k in names]))
    eng = HipHsic(X)
    try:
        got = eng.median_bandwidths()
    finally:
        eng.close()
    want = np.array([imn.select_sigma2(cols[k]) for k in names])
    assert np.array_equal(got, want), (got, want)


def test_n16384_matches_the_n2_kernel():
    X, perms = dn.big_case()
    P = 8
    rng = np.random.default_rng(dn.BIG_SEED + 1)
    perms = np.array([[rng.permutation(dn.BIG_N) for _ in range(P)] for _ in dn.BIG_PAIRS], dtype=np.int32)
    stat, ge, null = mi.hsic_null(X, dn.BIG_PAIRS, num_perm=P, perms=perms)
    eng = HipIndep(X)
    try:
        eng.median_bandwidths()
        s2, g2, n2 = eng.run("hsic", dn.BIG_PAIRS, P, perms, return_null=True)
    finally:
        eng.close()
    dev = max(np.abs(stat - s2).max(), np.abs(null - n2).max())
    gap = np.abs(n2 - s2[:, None]).min()
    print(f"n=16384: factored vs n^2 kernel, max abs deviation {dev:.3e}; smallest |null - stat| {gap:.3e}")
    assert dev <= BAR
    assert gap > 1e3 * BAR and np.array_equal(ge, g2)


def test_a_hundred_thousand_rows_with_device_permutations():
    n, P, seed = 100_000, 20, 0x1234567890
    rng = np.random.default_rng(8)
    x = rng.standard_normal(n)
    X = np.ascontiguousarray(np.column_stack([x, np.sin(2.0 * x) + rng.standard_normal(n), rng.standard_normal(n),
                                              np.full(n, 2.5)]))
    pairs = [(0, 1), (0, 2), (0, 3)]
    eng = HipHsic(X)
    try:
        s2 = eng.median_bandwidths()
        perms = np.stack([eng.device_perms(q, P, seed) for q in range(len(pairs))])
        stat, ge, null = eng.run(pairs, P, None, seed, return_null=True)
        rank, _ = eng.factor([0, 1, 2, 3])
    finally:
        eng.close()
    assert np.array_equal(perms, np.stack([dn.philox_perms(seed, q, P, n) for q in range(len(pairs))]))
    ws, wg, wn, ranks = hn.hsic_null(X, pairs, perms, sigma2=s2)
    dev = max(np.abs(stat - ws).max(), np.abs(null - wn).max())
    print(f"n={n}: GPU vs restatement on the device's permutations, max abs deviation {dev:.3e}; ranks {rank.tolist()}")
    assert dev <= BAR2
    assert (rank <= 64).all() and max(ranks.values()) <= 64
    assert ge[0] == 0 and np.array_equal(ge, wg)  # the dependent pair: p = 1 / 21
    assert stat[2] == 0.0 and ge[2] == P and not null[2].any()
    s, p = mi.hsic_tests(X[:, [0, 1, 3]], num_perm=P, seed=seed, perms="device")
    assert s[0, 1] == stat[0] and p[0, 1] == 1.0 / (P + 1) and s[1, 0] == s[0, 1] and p[1, 0] == p[0, 1]
    assert s[0, 2] == 0.0 and s[1, 2] == 0.0 and p[0, 2] == 1.0 and p[1, 2] == 1.0
    assert np.isnan(np.diag(s)).all() and not np.diag(p).any()


def test_budgets_and_runs_give_identical_bits():
    X = hn.data(1000)
    outs = []
    for budget in (0, 1, 0, 1):  # 1: a pair a column group (every column refactored), a group of 4 evaluations a batch
        outs.append(mi.hsic_null(X, hn.ALL_PAIRS_5, num_perm=6, seed=9, perms="device", budget_bytes=budget))
    outs.append(mi.hsic_null(X, hn.ALL_PAIRS_5, num_perm=6, seed=9, perms="device", budget_bytes=300_000))
    for o in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(o, outs[0]))
    assert outs[0][2].std() > 0
    rng = np.random.default_rng(1)  # host permutations take the same batches
    perms = np.array([[rng.permutation(1000) for _ in range(6)] for _ in hn.ALL_PAIRS_5], dtype=np.int32)
    a = mi.hsic_null(X, hn.ALL_PAIRS_5, num_perm=6, perms=perms)
    b = mi.hsic_null(X, hn.ALL_PAIRS_5, num_perm=6, perms=perms, budget_bytes=1)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_host_and_device_X_give_identical_bits_and_X_is_not_written():
    import torch
    X = hn.data(1000, seed=4)
    host = mi.hsic_null(X, hn.ALL_PAIRS_5, num_perm=4, seed=1, perms="device")
    Xd = torch.from_numpy(X).cuda()
    wide = torch.zeros((1000, 7), dtype=torch.float64, device="cuda")
    wide[:, :5] = Xd
    for T in (Xd, wide[:, :5]):  # contiguous, and a row stride above d
        keep = T.clone()
        dev = mi.hsic_null(T, hn.ALL_PAIRS_5, num_perm=4, seed=1, perms="device")
        assert all(np.array_equal(a, b) for a, b in zip(host, dev))
        assert torch.equal(T, keep)
    s_host, p_host = mi.hsic_tests(X, num_perm=4, seed=1)
    s_dev, p_dev = mi.hsic_tests(Xd, num_perm=4, seed=1)
    assert np.array_equal(s_host, s_dev, equal_nan=True) and np.array_equal(p_host, p_dev)


def test_X_from_a_side_stream_needs_no_synchronise():
    import torch
    X = hn.data(4097, seed=6)
    want = mi.hsic_null(X, hn.ALL_PAIRS_5, num_perm=2, seed=1, perms="device")
    base = torch.from_numpy(X).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Y = base
        for _ in range(50):  # X's producer: a chain of kernels that ends in X itself
            Y = (Y * 2.0) * 0.5
        got = mi.hsic_null(Y, hn.ALL_PAIRS_5, num_perm=2, seed=1, perms="device")
    assert all(np.array_equal(a, b) for a, b in zip(want, got))


def test_error_paths():
    import torch
    X = hn.data(97)
    bad = np.zeros((1, 1, 97), dtype=np.int32)  # in range, not a bijection
    with pytest.raises(ValueError, match="not a permutation"):
        mi.hsic_null(X, [(0, 1)], num_perm=1, perms=bad)
    bad[0, 0] = np.arange(97)
    bad[0, 0, 5] = 97
    with pytest.raises(ValueError, match="outside"):
        mi.hsic_null(X, [(0, 1)], num_perm=1, perms=bad)
    bad[0, 0, 5] = -1
    with pytest.raises(ValueError, match="outside"):
        mi.hsic_null(X, [(0, 1)], num_perm=1, perms=bad)
    Xd = torch.from_numpy(X).cuda()
    Xd[3, 1] = float("inf")
    with pytest.raises(ValueError, match="infs or NaNs"):
        mi.hsic_null(Xd, [(0, 1)], num_perm=1)
    eng = HipHsic(X)
    try:
        with pytest.raises(ValueError, match="set the bandwidths first"):
            eng.run([(0, 1)], 0)
        eng.median_bandwidths()
        with pytest.raises(ValueError, match="tol must be in"):
            eng.run([(0, 1)], 0, tol=1e-2)
        with pytest.raises(ValueError, match="tol must be in"):
            eng.factor([0], 1e-15)
        with pytest.raises(ValueError, match=r"pair index outside \[0, d\)"):
            eng.run([(0, 5)], 0)
        with pytest.raises(ValueError, match=r"column index outside \[0, d\)"):
            eng.factor([5])
        with pytest.raises(ValueError, match="finite and > 0"):
            eng.set_bandwidths([1.0, 0.0, 1.0, 1.0, 1.0])
        stat, ge = eng.run([(0, 1)], 0)  # the bandwidths of before still stand
        assert stat[0] > 0 and ge[0] == 0
    finally:
        eng.close()


def test_live_bytes_return_to_the_baseline_after_close():
    L = _lib.lib()
    base = L.midagma_debug_live_bytes()
    eng = HipHsic(hn.data(1000))
    eng.median_bandwidths()
    eng.run(hn.ALL_PAIRS_5, 3, None, 1)
    assert L.midagma_debug_live_bytes() > base
    eng.close()
    assert L.midagma_debug_live_bytes() == base
    h = C.c_void_p()
    assert L.midagma_hsic_create(C.byref(h), 10**6) == _lib.OK  # no such device: found by set_data
    x = np.zeros((4, 2))
    assert L.midagma_hsic_set_data(h, _lib.dptr(x), 4, 2, 0) == _lib.E_ARG
    L.midagma_hsic_destroy(h)
    assert L.midagma_debug_live_bytes() == base
