"""midagma_amd.mi_tests without a GPU: the module surface, the host-side tests, the argument checks
of the ABI, and a plain-numpy restatement of the two identities csrc/indep.hip evaluates, which
certifies tests/golden/indep.npz (made by tests/golden/make_indep.py from the reference) and the
formulation without the reference."""
import ctypes as C
import inspect

import numpy as np
import pytest

from tests import indep_numpy as inp
from midagma_amd import mi_tests as mi


@pytest.fixture(scope="module")
def fx(golden):
    return golden("indep.npz")


@pytest.fixture(scope="module")
def restated(fx):
    """{(case, stat): (P + 1 values per pair, m x (P + 1))} by the numpy restatement, and the stream."""
    out = {}
    for case in inp.CASES:
        X, pairs, P, seed = fx[f"{case}/X"], fx[f"{case}/pairs"], int(fx[f"{case}/P"]), int(fx[f"{case}/seed"])
        perms = inp.numpy_perms(seed, len(pairs), P, X.shape[0])
        out[case, "perms"] = perms
        for T in inp.STATS:
            out[case, T] = np.array([inp.pair_values(T, X[:, i], X[:, j], perms[q])
                                     for q, (i, j) in enumerate(pairs)])
    return out


def test_module_surface_and_signatures():
    for name in ("IndepTestResult", "hsic_stat", "dcor_stat", "test_pairwise_independence",
                 "get_I_from_full_pairwise_tests", "summarize_I"):
        assert hasattr(mi, name), name
    assert [f for f in mi.IndepTestResult.__dataclass_fields__] == ["i", "j", "stat", "pvalue"]
    assert list(inspect.signature(mi.hsic_stat).parameters) == ["x", "y", "sigma_x", "sigma_y"]
    assert list(inspect.signature(mi.dcor_stat).parameters) == ["x", "y"]
    sig = inspect.signature(mi.test_pairwise_independence)
    assert list(sig.parameters) == ["X", "pairs", "test", "num_perm", "seed", "perms"]
    assert [sig.parameters[k].default for k in ("test", "num_perm", "seed", "perms")] == ["hsic", 200, 0, "numpy"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("test", "num_perm", "seed", "perms"))
    sig = inspect.signature(mi.get_I_from_full_pairwise_tests)
    want = {"alpha": 0.05, "test": "hsic", "num_perm": 200, "seed": 0, "bonferroni": True, "undirected": True,
            "exclude_diagonal": True, "perms": "numpy"}
    assert list(sig.parameters) == ["X"] + list(want)
    for k, v in want.items():
        assert sig.parameters[k].default == v and sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY
    assert mi.test_pairwise_independence.__test__ is False
    assert not hasattr(mi, "permutation_pvalue")  # arbitrary stat_fn callables are not mirrored


@pytest.mark.parametrize("T", ["pearson", "spearman"])
def test_analytic_tests_equal_the_fixture(fx, T):
    X, pairs = fx["c97/X"], fx["c97/pairs"]
    X0 = X.copy()
    res = mi.test_pairwise_independence(X, [tuple(p) for p in pairs], test=T)
    assert [(r.i, r.j) for r in res] == [tuple(p) for p in pairs.tolist()]
    assert np.array_equal([r.stat for r in res], fx[f"c97/{T}/stat"])
    assert np.array_equal([r.pvalue for r in res], fx[f"c97/{T}/pvalue"])
    assert np.array_equal(X, X0)


def test_spearman_constant_column_rule():
    X = np.random.default_rng(1).standard_normal((30, 2))
    X[:, 1] = 2.0
    (r,) = mi.test_pairwise_independence(X, [(0, 1)], test="spearman")
    assert (r.stat, r.pvalue) == (0.0, 1.0)


def test_summarize_I_prints(capsys):
    mi.summarize_I(np.array([[0, 1], [1, 2]]), 3)
    assert "I size: 2 pairs (d=3)" in capsys.readouterr().out
    mi.summarize_I(np.zeros((0, 2), dtype=int), 3)
    assert "I size: 0 pairs" in capsys.readouterr().out


def test_bad_inputs_raise_value_error_before_any_device():
    X = np.random.default_rng(0).standard_normal((10, 3))
    bad = X.copy()
    bad[3, 1] = np.nan
    for T in ("hsic", "dcor", "pearson"):
        with pytest.raises(ValueError):
            mi.test_pairwise_independence(bad, [(0, 1)], test=T)
        with pytest.raises(ValueError):
            mi.test_pairwise_independence(X[:1], [(0, 1)], test=T)
        with pytest.raises(ValueError):
            mi.test_pairwise_independence(X, [(0, 3)], test=T)
    with pytest.raises(ValueError):
        mi.test_pairwise_independence(np.zeros((16385, 2)), [(0, 1)], test="hsic")
    with pytest.raises(ValueError):
        mi.test_pairwise_independence(X, [(0, 1)], test="mi")
    with pytest.raises(ValueError):
        mi.test_pairwise_independence(X, [(0, 1)], test="hsic", perms="torch")


def test_permutation_tests_have_no_cpu_path():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from midagma_amd._lib import HipSolverError
    X = np.random.default_rng(0).standard_normal((10, 3))
    for T in ("hsic", "dcor"):
        with pytest.raises(HipSolverError):
            mi.test_pairwise_independence(X, [(0, 1)], test=T, num_perm=3)
        with pytest.raises(HipSolverError):
            mi.get_I_from_full_pairwise_tests(X, test=T, num_perm=3)
    with pytest.raises(HipSolverError):
        mi.hsic_stat(X[:, 0], X[:, 1])
    with pytest.raises(HipSolverError):
        mi.dcor_stat(X[:, 0], X[:, 1])


def test_indep_entry_points_validate_without_a_device():
    from midagma_amd import _lib
    L = _lib.load()
    assert L.midagma_abi_version() == 11  # the entries are additive
    out = C.c_void_p()
    assert L.midagma_indep_create(None, 0) == -3
    assert L.midagma_indep_create(C.byref(out), -1) == -3
    assert b"bad arguments" in L.midagma_indep_last_error(None)
    x = np.zeros(4)
    assert L.midagma_indep_set_data(None, _lib.dptr(x), 2, 2) == -3
    assert L.midagma_indep_set_bandwidths(None, _lib.dptr(x), 2) == -3
    assert L.midagma_indep_batch_pairs(None, 10, 0) == 0
    assert L.midagma_indep_run(None, 0, None, 0, 0, None, 0, 0, None, None, None, None) == -3
    L.midagma_indep_destroy(None)


@pytest.mark.parametrize("case", inp.CASES)
def test_fixture_guards_and_tie_condition(fx, restated, case):
    """The numpy permutation stream is the one the fixture was recorded with, and no permuted
    value of a non-constant pair lies within 1e-6 (relative) of the observed one."""
    assert np.array_equal(inp.perm_guard(restated[case, "perms"]), fx[f"{case}/perm_guard"])
    X, pairs, P = fx[f"{case}/X"], fx[f"{case}/pairs"], int(fx[f"{case}/P"])
    pl = pairs.tolist()
    assert any(i == j for i, j in pl) and any([j, i] in pl for i, j in pl if i != j)
    for T in inp.STATS:
        stat, null = fx[f"{case}/{T}/stat"], fx[f"{case}/{T}/null"]
        assert null.shape == (len(pairs), P)
        for q, (i, j) in enumerate(pairs):
            if np.ptp(X[:, i]) == 0 or np.ptp(X[:, j]) == 0:
                assert stat[q] == 0 and (null[q] == 0).all() and fx[f"{case}/{T}/ge"][q] == P
                assert fx[f"{case}/{T}/pvalue"][q] == 1.0
            else:
                assert np.abs(null[q] - stat[q]).min() >= 1e-6 * abs(stat[q])


@pytest.mark.parametrize("T", inp.STATS)
@pytest.mark.parametrize("case", inp.CASES)
def test_identities_reproduce_the_reference(fx, restated, case, T):
    """(1/n^2) sum Kc[a,b] L[pi_a, pi_b] (HSIC) and (1/n^2) sum Ax[a,b] |y[pi_a] - y[pi_b]| (dCor),
    with nothing re-centred per permutation, give the reference's observed and permuted statistics
    to 1e-13 and every count exactly."""
    vals = restated[case, T]
    P = int(fx[f"{case}/P"])
    dev = max(np.abs(vals[:, 0] - fx[f"{case}/{T}/stat"]).max(), np.abs(vals[:, 1:] - fx[f"{case}/{T}/null"]).max())
    print(f"{case} {T}: numpy restatement vs reference, max abs deviation {dev:.3e}")
    assert dev <= 1e-13
    ge = (vals[:, 1:] >= vals[:, :1]).sum(axis=1)
    assert np.array_equal(ge, fx[f"{case}/{T}/ge"])
    assert np.array_equal((ge + 1) / (P + 1), fx[f"{case}/{T}/pvalue"])


def test_median_bandwidth_is_the_reference_rule():
    rng = np.random.default_rng(5)
    for n in (2, 5, 64, 97):
        x = rng.standard_normal(n)
        assert mi.median_sigma2(x) == inp.median_sigma2(x)
    assert mi.median_sigma2(np.full(7, 3.0)) == 1.0


@pytest.mark.parametrize("n", [5, 97, 1000])
def test_host_philox_permutations_are_valid(n):
    perms = inp.philox_perms(12345678901234567, 3, 4, n)
    assert perms.shape == (3, 4, n)
    assert np.array_equal(np.sort(perms, axis=2), np.broadcast_to(np.arange(n), perms.shape))
    flat = perms.reshape(-1, n)
    if n > 5:
        assert len({r.tobytes() for r in flat}) == len(flat)  # (q, p) enter the counter
    assert not np.array_equal(perms, inp.philox_perms(1, 3, 4, n))


def test_philox_known_answer():
    """Random123's known-answer vectors for Philox4x32-10."""
    z = np.zeros(1, dtype=np.uint64)
    assert [int(v[0]) for v in inp.philox4x32_10(z, z, z, z, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = np.full(1, 0xFFFFFFFF, dtype=np.uint64)
    assert [int(v[0]) for v in inp.philox4x32_10(f, f, f, f, 0xFFFFFFFF, 0xFFFFFFFF)] == [
        0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
