"""csrc/dcor.hip on the GPU: the dCor tests without the n^2 sum against the reference's recorded
results (tests/golden/indep.npz), against tests/dcor_numpy.py (certified on the CPU by
tests/test_dcor_cpu.py) and against the n^2 kernel of csrc/indep.hip.

The bar on the statistics is 1e-12 absolute on stat^2 (R^2 for the reference's form, R_U for the
bias-corrected one), tests/test_gpu_indep.py's bar; counts and p-values are exact wherever the data
keeps the permuted values away from the observed one (the fixture's perm_guard, the seeds checked
in tests/test_dcor_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from midagma_amd import _lib
from midagma_amd import mi_tests as mi
from midagma_amd.solver import HipDcor, HipIndep, column_argsort
from tests import dcor_numpy as dn
from tests import indep_numpy as inp

pytestmark = pytest.mark.gpu

BAR = 1e-12


@pytest.fixture(scope="module")
def fx(golden):
    return golden("indep.npz")


@pytest.mark.parametrize("case", inp.CASES)
def test_statistics_counts_and_pvalues_match_the_reference(fx, case):
    X, pairs, P, seed = fx[f"{case}/X"], fx[f"{case}/pairs"], int(fx[f"{case}/P"]), int(fx[f"{case}/seed"])
    X0 = X.copy()
    stat, ge, null = mi.dcor_null(X, pairs, num_perm=P, seed=seed, perms="numpy")
    dev = max(np.abs(stat - fx[f"{case}/dcor/stat"]).max(), np.abs(null - fx[f"{case}/dcor/null"]).max())
    print(f"{case}: GPU vs reference, max abs deviation {dev:.3e}")
    assert dev <= BAR
    assert np.array_equal(ge, fx[f"{case}/dcor/ge"])
    assert np.array_equal((ge + 1) / (P + 1), fx[f"{case}/dcor/pvalue"])
    assert np.array_equal(X, X0)


def test_get_I_matches_the_reference(fx):
    """The undirected sets are the reference's.  With undirected=False the reference draws fresh
    permutations for (j, i) while `dcor_tests` mirrors (i, j)'s p-value, so that set is the
    reference's only where no mirrored decision differs: under Bonferroni here (b1_u0); for b0_u0
    the two differ by construction (24 pairs against the fixture's 22), and the mirrored set is
    checked against the undirected one instead."""
    X, P, seed = fx["c96/X"], int(fx["c96/P"]), int(fx["c96/seed"])
    got = {}
    for b in (0, 1):
        for u in (0, 1):
            I = mi.get_I_from_dcor_tests(X, alpha=0.05, num_perm=P, seed=seed, perms="numpy", bonferroni=bool(b),
                                         undirected=bool(u))
            assert I.dtype == np.asarray([], dtype=int).dtype
            got[b, u] = I.reshape(-1, 2)
    for b, u in ((0, 1), (1, 1), (1, 0)):
        assert np.array_equal(got[b, u], fx[f"c96/dcor/I_b{b}_u{u}"]), (b, u)
    both = sorted(map(tuple, np.concatenate([got[0, 1], got[0, 1][:, ::-1]]).tolist()))
    assert sorted(map(tuple, got[0, 0].tolist())) == both
    assert len({len(v) for v in got.values()}) > 1  # the flags select different sets here
    X3 = fx["c96/X"][:, :3]  # x0, sin(3 x0), 0.9 x0: every pair dependent
    I = mi.get_I_from_dcor_tests(X3, alpha=0.5, num_perm=19, seed=0, perms="numpy", bonferroni=False)
    assert I.size == 0 and I.dtype == np.asarray([], dtype=int).dtype


def _second_edge(n, block):
    return {0: 4 if n < 64 else 32, 4: 0, 16: 64, 64: 8}[block]


@pytest.mark.parametrize("n,block", [(2, 0), (3, 0), (5, 4), (96, 16), (97, 16), (257, 64), (1000, 0), (4097, 0)])
def test_data_kinds_match_the_restatement(n, block):
    P = 3
    rng = np.random.default_rng(n)
    perms = np.array([[rng.permutation(n) for _ in range(P)] for _ in dn.ALL_PAIRS_5], dtype=np.int32)
    worst = 0.0
    for X in dn.kind_matrices(n, seed=n):
        X0 = X.copy()
        for unbiased in ((False, True) if n >= 4 else (False,)):
            _, _, _, vals = dn.dcor_null(X, dn.ALL_PAIRS_5, perms, block, unbiased)
            prep = {v: dn.column_prep(X[:, v]) for v in range(5)}
            want = np.array([[dn.r2_of(v, prep[i], prep[j], unbiased) for v in vals[q]]
                             for q, (i, j) in enumerate(dn.ALL_PAIRS_5)])
            out = []
            for edge in (block, _second_edge(n, block)):
                stat, _, null = mi.dcor_null(X, dn.ALL_PAIRS_5, num_perm=P, perms=perms, unbiased=unbiased, block=edge)
                got = np.column_stack([stat, null])
                out.append(got if unbiased else got**2)
            worst = max(worst, np.abs(out[0] - want).max(), np.abs(out[1] - out[0]).max())
            assert np.abs(out[0] - want).max() <= BAR
            assert np.abs(out[1] - out[0]).max() <= BAR  # two block edges agree
        assert np.array_equal(X, X0)
    print(f"n={n} block={block}: GPU vs restatement, worst |stat^2 deviation| {worst:.3e}")


def test_n16384_matches_the_n2_kernel():
    X, perms = dn.big_case()
    stat, ge, null = mi.dcor_null(X, dn.BIG_PAIRS, num_perm=dn.BIG_P, perms=perms)
    eng = HipIndep(X)
    try:
        s2, g2, n2 = eng.run("dcor", dn.BIG_PAIRS, dn.BIG_P, perms, return_null=True)
    finally:
        eng.close()
    dev = max(np.abs(stat - s2).max(), np.abs(null - n2).max())
    print(f"n=16384: block path vs n^2 kernel, max abs deviation {dev:.3e}")
    assert dev <= BAR
    assert np.array_equal(ge, g2)


@pytest.mark.parametrize("n", [5, 97, 70001])
def test_device_permutations_match_the_restatement(n):
    X = dn.kind_matrices(n, seed=1)[1][:, [0, 4, 3]].copy()
    P, seed, pairs = 2, 0x1234567890, [(0, 1), (0, 2)]
    eng = HipDcor(X)
    try:
        perms = np.stack([eng.device_perms(q, P, seed) for q in range(len(pairs))])
        p1, inv = eng.device_perms(1, P, seed, inverse=True)
        stat, ge, null = eng.run(pairs, P, None, seed, block=256 if n > 1024 else 0, return_null=True)
    finally:
        eng.close()
    want = np.stack([dn.philox_perms(seed, q, P, n) for q in range(len(pairs))])
    assert np.array_equal(perms, want)
    assert np.array_equal(p1, want[1]) and np.array_equal(np.take_along_axis(inv, p1, 1), np.tile(np.arange(n), (P, 1)))
    ws, wg, wn, _ = dn.dcor_null(X, pairs, want, 256 if n > 1024 else 0)
    dev = max(np.abs(stat**2 - ws**2).max(), np.abs(null**2 - wn**2).max())
    print(f"n={n}: device permutations, GPU vs restatement |stat^2 deviation| {dev:.3e}")
    assert dev <= BAR
    if n > 5:
        assert np.array_equal(ge, wg)


def test_a_million_rows():
    n = 1_000_003
    rng = np.random.default_rng(0)
    x = rng.standard_normal(n)
    X = np.ascontiguousarray(np.column_stack([x, 3.0 - 2.0 * x, np.full(n, 2.5)]))
    stat, p = mi.dcor_tests(X, num_perm=1, seed=3, perms="device")
    assert abs(stat[0, 1] - 1.0) <= 1e-9 and stat[1, 0] == stat[0, 1]
    assert stat[0, 2] == 0.0 and stat[1, 2] == 0.0 and p[0, 2] == 1.0 and p[1, 2] == 1.0
    assert p[0, 1] == 0.5 and np.array_equal(np.diag(stat), np.ones(3)) and np.array_equal(np.diag(p), np.zeros(3))
    # ties do not unbalance the blocks: a 0/1 column of that length
    B = np.ascontiguousarray(np.column_stack([x, (x + rng.standard_normal(n) > 0).astype(float)]))
    s, ge, _ = mi.dcor_null(B, [(0, 1)], num_perm=0, return_null=False)
    assert 0.3 < s[0] < 0.9 and ge[0] == 0


def test_budgets_and_runs_give_identical_bits():
    X = dn.kind_matrices(1000, seed=2)[0]
    outs = []
    for budget in (0, 1, 0, 1):  # 1: every chunk holds one evaluation
        stat, ge, null = mi.dcor_null(X, dn.ALL_PAIRS_5, num_perm=5, seed=9, perms="device", budget_bytes=budget)
        outs.append((stat, ge, null))
    for o in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(o, outs[0]))
    assert outs[0][2].std() > 0


def test_host_and_device_X_give_identical_bits_and_X_is_not_written():
    import torch
    X = dn.kind_matrices(1000, seed=4)[1]
    host = mi.dcor_null(X, dn.ALL_PAIRS_5, num_perm=4, seed=1, perms="device")
    Xd = torch.from_numpy(X).cuda()
    wide = torch.zeros((1000, 7), dtype=torch.float64, device="cuda")
    wide[:, :5] = Xd
    for T in (Xd, wide[:, :5]):  # contiguous, and a row stride above d
        keep = T.clone()
        dev = mi.dcor_null(T, dn.ALL_PAIRS_5, num_perm=4, seed=1, perms="device")
        assert all(np.array_equal(a, b) for a, b in zip(host, dev))
        assert torch.equal(T, keep)
    s_host, p_host = mi.dcor_tests(X, num_perm=4, seed=1)
    s_dev, p_dev = mi.dcor_tests(Xd, num_perm=4, seed=1)
    assert np.array_equal(s_host, s_dev) and np.array_equal(p_host, p_dev)


def test_X_from_a_side_stream_needs_no_synchronise():
    import torch
    X = dn.kind_matrices(4097, seed=6)[1]
    want = mi.dcor_null(X, dn.ALL_PAIRS_5, num_perm=2, seed=1, perms="device")
    base = torch.from_numpy(X).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Y = base
        for _ in range(50):  # X's producer: a chain of kernels that ends in X itself
            Y = (Y * 2.0) * 0.5
        got = mi.dcor_null(Y, dn.ALL_PAIRS_5, num_perm=2, seed=1, perms="device")
    assert all(np.array_equal(a, b) for a, b in zip(want, got))


@pytest.mark.parametrize("seed", dn.CHI2_SEEDS)
def test_chi2(seed):
    X = dn.chi2_case(seed)
    n = dn.CHI2_N
    stat, p = mi.dcor_tests(X, pvalue="chi2")
    want, _, _, _ = dn.dcor_null(X, [(0, 1), (0, 2), (1, 2)], None, 0, True)
    got = np.array([stat[0, 1], stat[0, 2], stat[1, 2]])
    assert np.abs(n * got - n * want).max() <= n * BAR
    assert np.array_equal(p[np.triu_indices(3, 1)], dn.chi2_pvalue(n, got))
    assert p[0, 1] > 0.05 and p[0, 2] < 1e-6
    assert np.array_equal(p, p.T) and np.array_equal(np.diag(p), np.zeros(3))
    C3 = np.column_stack([X[:, 0], np.full(n, 1.0)])
    s, pv = mi.dcor_tests(C3, pvalue="chi2")
    assert s[0, 1] == 0.0 and pv[0, 1] == 1.0
    with pytest.raises(ValueError):
        mi.dcor_tests(X[:3], pvalue="chi2")
    eng = HipDcor(X[:3])
    try:
        with pytest.raises(ValueError, match="n >= 4"):
            eng.run([(0, 1)], 0, unbiased=True)
    finally:
        eng.close()


def test_colargsort_is_numpys_stable_argsort():
    import torch
    for n, d in ((2, 1), (97, 3), (4097, 5), (70001, 2)):
        X = np.round(np.random.default_rng(n).standard_normal((n, d)) * 4) / 4  # many ties
        X[::7, 0] = -0.0
        X[1::7, 0] = 0.0
        order = column_argsort(torch.from_numpy(X).cuda(), budget_bytes=1 if n == 97 else 0).cpu().numpy()
        want = np.argsort(X + 0.0, axis=0, kind="stable").T
        assert np.array_equal(order, want)
    with pytest.raises(ValueError, match="infs or NaNs"):
        column_argsort(torch.tensor([[1.0], [float("nan")]], dtype=torch.float64, device="cuda"))


def test_bad_permutations_and_nonfinite_device_X_are_rejected():
    import torch
    X = dn.kind_matrices(97, seed=0)[0]
    bad = np.zeros((1, 1, 97), dtype=np.int32)  # in range, not a bijection
    with pytest.raises(ValueError, match="not a permutation"):
        mi.dcor_null(X, [(0, 1)], num_perm=1, perms=bad)
    bad[0, 0] = np.arange(97)
    bad[0, 0, 5] = 97
    with pytest.raises(ValueError, match="outside"):
        mi.dcor_null(X, [(0, 1)], num_perm=1, perms=bad)
    Xd = torch.from_numpy(X).cuda()
    Xd[3, 1] = float("inf")
    with pytest.raises(ValueError, match="infs or NaNs"):
        mi.dcor_null(Xd, [(0, 1)], num_perm=1)


def test_live_bytes_return_to_the_baseline_after_close():
    L = _lib.lib()
    base = L.midagma_debug_live_bytes()
    eng = HipDcor(dn.kind_matrices(1000, seed=0)[0])
    eng.run(dn.ALL_PAIRS_5, 3, None, 1)
    assert L.midagma_debug_live_bytes() > base
    eng.close()
    assert L.midagma_debug_live_bytes() == base
    h = C.c_void_p()
    assert L.midagma_dcor_create(C.byref(h), 10**6) == _lib.OK  # no such device: found by set_data
    x = np.zeros((4, 2))
    assert L.midagma_dcor_set_data(h, _lib.dptr(x), 4, 2, 0) == _lib.E_ARG
    L.midagma_dcor_destroy(h)
    assert L.midagma_debug_live_bytes() == base
    # ... and destroying it left no stale HIP error behind for the thread's next launch check
    stat, _, _ = mi.dcor_null(dn.kind_matrices(97, seed=0)[0], [(0, 1)], num_perm=1, perms="device")
    assert 0.0 < stat[0] <= 1.0
