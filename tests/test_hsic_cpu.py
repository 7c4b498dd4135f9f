"""HSIC from low-rank factors, on the CPU: tests/hsic_numpy.py (the restatement the GPU tests hold
csrc/hsic.hip to) against the reference's recorded results and against the Gram matrix itself, the
bandwidths the GPU tests use to force ranks, and the argument checks of the C entries and the Python
functions (no device is opened by any of them).

The factored statistic differs from the n^2 sum by at most 4 eta (1 + eta) ("HSIC from
low-rank factors"); at eta = 1e-13 the restatement is within 1e-15 of every recorded value."""
import ctypes as C

import numpy as np
import pytest

from midagma_amd import _lib
from midagma_amd import mi_tests as mi
from tests import hsic_numpy as hn
from tests import indep_numpy as inp


@pytest.fixture(scope="module")
def fx(golden):
    return golden("indep.npz")


@pytest.mark.parametrize("case", inp.CASES)
def test_restatement_matches_the_recorded_reference(fx, case):
    X, pairs, P, seed = fx[f"{case}/X"], fx[f"{case}/pairs"], int(fx[f"{case}/P"]), int(fx[f"{case}/seed"])
    perms = inp.numpy_perms(seed, len(pairs), P, X.shape[0])
    stat, ge, null, ranks = hn.hsic_null(X, pairs, perms)
    dev = max(np.abs(stat - fx[f"{case}/hsic/stat"]).max(), np.abs(null - fx[f"{case}/hsic/null"]).max())
    print(f"{case}: restatement vs reference, max abs deviation {dev:.3e}, largest rank {max(ranks.values())}")
    assert dev <= 1e-12
    assert np.array_equal(ge, fx[f"{case}/hsic/ge"])
    assert np.array_equal((ge + 1) / (P + 1), fx[f"{case}/hsic/pvalue"])
    assert max(ranks.values()) <= 64


@pytest.mark.parametrize("n", [5, 97, 257])
def test_elementwise_residual_is_within_eta(n):
    X = hn.data(n)
    for v in range(X.shape[1]):
        s2 = inp.median_sigma2(X[:, v])
        F, resid = hn.ichol(X[:, v], s2)
        err = np.abs(hn.gram(X[:, v], s2) - F @ F.T).max()
        print(f"n={n} column {v}: rank {F.shape[1]}, max|K - F F^T| {err:.3e}, resid {resid:.3e}")
        assert resid <= hn.ETA and err <= hn.ETA
    F, _ = hn.ichol(X[:, 4], 1.0)  # the zero-range column: rank 1 and a centred factor that is exactly 0
    assert F.shape[1] == 1 and not hn.centred(F).any()


def test_forced_rank_bandwidths_give_their_ranks():
    x = hn.data(300)[:, 0]
    for rank, s2 in hn.FORCED_RANKS.items():
        F, resid = hn.ichol(x, s2)
        assert F.shape[1] == rank and resid <= hn.ETA, (rank, F.shape[1])


def test_c96_mirrored_I_sets(fx):
    """`get_I_from_hsic_tests` mirrors (i, j)'s p-value to (j, i) where the reference draws fresh
    permutations: the recorded sets it must reproduce are the undirected ones and b1_u0."""
    X, P, seed = fx["c96/X"], int(fx["c96/P"]), int(fx["c96/seed"])
    d = X.shape[1]
    iu = np.triu_indices(d, 1)
    pairs = np.stack(iu, axis=1)
    _, ge, _, _ = hn.hsic_null(X, pairs, inp.numpy_perms(seed, len(pairs), P, X.shape[0]))
    p = np.zeros((d, d))
    p[iu] = p.T[iu] = (ge + 1.0) / (P + 1.0)
    for b, u in ((0, 1), (1, 1), (1, 0)):
        assert np.array_equal(mi._I_from_pvalues(p, 0.05, bool(b), bool(u), True), fx[f"c96/hsic/I_b{b}_u{u}"])


def test_no_device_is_an_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.HipSolverError):
        mi.hsic_null(hn.data(8), [(0, 1)])


# --- argument checks: every one is answered before a device is touched -----------------------------
def _err(h=None):
    m = _lib.lib().midagma_hsic_last_error(h)
    return m.decode() if m else ""


def test_c_entries_check_their_arguments_without_a_device():
    L = _lib.lib()
    buf = np.zeros(16)
    X = C.c_void_p(buf.ctypes.data)
    assert L.midagma_hsic_create(None, 0) == _lib.E_ARG and _err() == "hsic_create: bad arguments"
    h = C.c_void_p()
    assert L.midagma_hsic_create(C.byref(h), -1) == _lib.E_ARG
    assert L.midagma_hsic_set_data(None, _lib.dptr(buf), 4, 2, 0) == _lib.E_ARG
    assert L.midagma_hsic_run(None, None, 0, 0, None, 0, 1e-13, 0, 0, None, None, None) == _lib.E_ARG
    assert L.midagma_hsic_factor(None, None, 0, 1e-13, None, None) == _lib.E_ARG
    assert L.midagma_hsic_profile(None, None) == _lib.E_ARG
    assert L.midagma_hsic_create(C.byref(h), 0) == _lib.OK and h.value
    try:
        for n, d in ((1, 2), (2**31, 2), (4, 0), (4, 65536)):
            assert L.midagma_hsic_set_data(h, _lib.dptr(buf), n, d, 0) == _lib.E_ARG, (n, d)
        assert L.midagma_hsic_set_data(h, None, 4, 2, 0) == _lib.E_ARG
        for n, d, ld in ((1, 2, 2), (2**31, 2, 2), (4, 0, 2), (4, 65536, 65536), (4, 2, 1)):
            assert L.midagma_hsic_set_data_dev(h, X, n, d, ld, 0, None) == _lib.E_ARG, (n, d, ld)
        assert "leading dimension" in _err(h)
        pairs = np.array([[0, 1]], dtype=np.int64)
        stat, ge = np.zeros(1), np.zeros(1, dtype=np.int64)
        PP, G = C.c_void_p(pairs.ctypes.data), C.c_void_p(ge.ctypes.data)

        def run(pp=PP, m=1, P=0, tol=1e-13, chunk=0, st=_lib.dptr(stat), g=G):
            return L.midagma_hsic_run(h, pp, m, P, None, 0, tol, chunk, 0, st, g, None)

        assert run(pp=None) == _lib.E_ARG and run(st=None) == _lib.E_ARG and run(g=None) == _lib.E_ARG
        assert run(P=-1) == _lib.E_ARG and run(P=65536) == _lib.E_ARG and run(m=-1) == _lib.E_ARG
        for tol in (0.0, 9e-15, 2e-3, float("nan")):
            assert run(tol=tol) == _lib.E_ARG and "tol" in _err(h)
            assert L.midagma_hsic_factor(h, PP, 1, tol, None, None) == _lib.E_ARG and "tol" in _err(h)
        for chunk in (8, 17, -16, 2**20 + 16):
            assert run(chunk=chunk) == _lib.E_ARG and "chunk" in _err(h)
        assert run() == _lib.E_ARG and "set the data first" in _err(h)
        assert L.midagma_hsic_set_bandwidths(h, _lib.dptr(buf), 2) == _lib.E_ARG and "set the data first" in _err(h)
        assert L.midagma_hsic_median_bandwidths(h, None, 0, None) == _lib.E_ARG
        assert L.midagma_hsic_factor(h, PP, 1, 1e-13, None, None) == _lib.E_ARG and "set the data first" in _err(h)
        assert L.midagma_hsic_get_factor(h, 0, _lib.dptr(buf), None) == _lib.E_ARG
        assert L.midagma_hsic_perms(h, 0, 1, 0, PP) == _lib.E_ARG
        ms = np.full(4, -1.0)
        assert L.midagma_hsic_profile(h, _lib.dptr(ms)) == _lib.OK and not ms.any()
    finally:
        L.midagma_hsic_destroy(h)
    L.midagma_hsic_destroy(None)


def test_python_functions_check_their_arguments_without_a_device():
    X = np.random.default_rng(0).standard_normal((8, 3))
    with pytest.raises(ValueError, match="perms"):
        mi.hsic_null(X, [(0, 1)], perms="host")
    with pytest.raises(ValueError, match="num_perm"):
        mi.hsic_null(X, [(0, 1)], num_perm=-1)
    with pytest.raises(ValueError, match="pair index"):
        mi.hsic_null(X, [(0, 3)])
    for tol in (0.0, 1e-15, 1e-2):
        with pytest.raises(ValueError, match="tol"):
            mi.hsic_null(X, [(0, 1)], tol=tol)
        with pytest.raises(ValueError, match="tol"):
            mi.hsic_tests(X, tol=tol)
    with pytest.raises(ValueError, match="chunk"):
        mi.hsic_null(X, [(0, 1)], chunk=24)
    with pytest.raises(ValueError, match="perms must be"):
        mi.hsic_null(X, [(0, 1)], num_perm=2, perms=np.zeros((1, 2, 7), dtype=np.int32))
    with pytest.raises(ValueError, match="sigma2"):
        mi.hsic_null(X, [(0, 1)], sigma2=[1.0, 0.0, 1.0])
    with pytest.raises(ValueError, match="sigma2"):
        mi.hsic_null(X, [(0, 1)], sigma2=[1.0, 1.0])
    with pytest.raises(ValueError, match="inf or nan"):
        mi.hsic_null(np.where(X > 2, np.nan, np.inf), [(0, 1)])
    with pytest.raises(ValueError, match="2-d"):
        mi.hsic_null(X[:, 0], [(0, 1)])
    with pytest.raises(ValueError, match="at least 2"):
        mi.hsic_tests(X[:1])
    with pytest.raises(ValueError, match="perms"):
        mi.get_I_from_hsic_tests(X, perms="host")
    for name in ("hsic_null", "hsic_tests", "get_I_from_hsic_tests"):
        assert name in mi.__all__ and name in mi.__doc__
