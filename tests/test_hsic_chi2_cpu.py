"""The HSIC chi-square test without a GPU: tests/hsic_u_numpy.py's factor identity (b) against the
O(n^2) definition (a) within the derived bound, the calibration and the power of the test on the
definition alone, the public-API case's margins, and the argument checks of the new entries."""
import ctypes as C

import numpy as np
import pytest

from midagma_amd import _lib
from midagma_amd import mi_tests as mi
from tests import hsic_numpy as hn
from tests import hsic_u_numpy as hu


@pytest.mark.parametrize("eta", [1e-13, 1e-6])
@pytest.mark.parametrize("n", [4, 5, 97, 500])
def test_factor_identity_matches_the_definition(n, eta):
    X = hn.data(n)
    want = hu.cov_u_direct(X)
    cov, bia, ranks = hu.cov_u_factors(X, eta=eta)
    dev = np.abs(cov - want).max()
    print(f"n={n} eta={eta:g}: identity vs definition, max abs deviation {dev:.3e} (bound {hu.bound(n, eta):.3e}), "
          f"ranks {ranks}")
    assert dev <= hu.ROUND + hu.bound(n, eta)
    assert not cov[4].any() and not cov[:, 4].any()  # the constant column: D = 0
    assert (np.diag(cov)[:4] > 0).all() and np.array_equal(cov, cov.T)
    # the identity's first term is hsic_numpy's statistic (the constant column's factor is exactly 0)
    stat, _, _, _ = hn.hsic_null(X, hn.ALL_PAIRS_5, None, eta=eta)
    assert np.array_equal(stat, np.array([bia[i, j] for i, j in hn.ALL_PAIRS_5]))


def test_the_centred_form_is_exact_on_a_full_rank_factor():
    """With eta = 0 the factor reproduces K to rounding, so (b) is (a) to rounding."""
    X = hn.data(97)[:, :4]
    want = hu.cov_u_direct(X)
    cov, _, _ = hu.cov_u_factors(X, eta=1e-300)
    assert np.abs(cov - want).max() <= hu.ROUND


def test_calibration_on_independent_columns():
    below = total = 0
    for seed in range(40):
        X = np.random.default_rng(500 + seed).standard_normal((200, 5))
        p = hu.pvalues(hu.r_u(hu.cov_u_direct(X)), 200)[np.triu_indices(5, 1)]
        below += int((p < 0.05).sum())
        total += p.size
    print(f"calibration: {below} of {total} independent pairs have p < 0.05")
    assert total == 400 and below / total <= 0.10


def test_a_dependent_pair_is_rejected():
    X = hn.data(500)[:, :2]  # y = sin 2x + noise
    cov = hu.cov_u_direct(X)
    p = hu.pvalues(hu.r_u(cov), 500)[0, 1]
    print(f"dependent pair at n=500: R_U {hu.r_u(cov)[0, 1]:.4f}, p {p:.3e}")
    assert p < 1e-6


def test_the_api_case_excuses_no_pair():
    """No oracle p-value of the public-API case (tests/test_gpu_hsic_chi2.py) has alpha_eff inside its
    corner interval, so the GPU's pair set must equal the oracle's with no pair excused."""
    X = hu.api_case()
    cov = hu.cov_u_direct(X)
    R, dR = hu.corner_intervals(cov, hu.API_N, hu.bound(hu.API_N, 1e-13))
    plo, phi = hu.p_interval(R, dR, hu.API_N)
    I, alpha_eff = hu.pair_set(hu.pvalues(R, hu.API_N))
    iu = np.triu_indices(hu.API_D, 1)
    excused = int(((plo[iu] <= alpha_eff) & (alpha_eff <= phi[iu])).sum())
    print(f"api case: |I| = {len(I)} of {len(iu[0])} pairs, alpha_eff {alpha_eff:.3e}, excused {excused}")
    assert excused == 0 and 0 < len(I) < len(iu[0])


def _err(h=None):
    m = _lib.lib().midagma_hsic_last_error(h)
    return m.decode() if m else ""


def test_c_entries_check_their_arguments_without_a_device():
    L = _lib.lib()
    out = np.zeros(4)
    assert L.midagma_hsic_all_pairs(None, None, 0, 1e-13, 0, 0, _lib.dptr(out), None) == _lib.E_ARG
    assert _err() == "hsic_all_pairs: null handle"
    assert L.midagma_hsic_all_pairs_profile(None, None) == _lib.E_ARG
    h = C.c_void_p()
    assert L.midagma_hsic_create(C.byref(h), 0) == _lib.OK
    try:
        cols = np.array([0, 1], dtype=np.int64)
        CP = C.c_void_p(cols.ctypes.data)

        def run(cp=CP, k=2, tol=1e-13, chunk=0, o=_lib.dptr(out)):
            return L.midagma_hsic_all_pairs(h, cp, k, tol, chunk, 0, o, None)

        assert run(o=None) == _lib.E_ARG and "null pointer" in _err(h)
        assert run(k=-1) == _lib.E_ARG and "ncols" in _err(h)
        for tol in (0.0, 9e-15, 2e-3, float("nan")):
            assert run(tol=tol) == _lib.E_ARG and "tol" in _err(h)
        for chunk in (8, 17, -16, 2**20 + 16):
            assert run(chunk=chunk) == _lib.E_ARG and "chunk" in _err(h)
        assert run() == _lib.E_ARG and "set the data first" in _err(h)
        ms = np.full(3, -1.0)
        assert L.midagma_hsic_all_pairs_profile(h, _lib.dptr(ms)) == _lib.OK and not ms.any()
        assert L.midagma_abi_version() == 11
    finally:
        L.midagma_hsic_destroy(h)


def test_python_functions_check_their_arguments_without_a_device():
    X = np.random.default_rng(0).standard_normal((8, 3))
    with pytest.raises(ValueError, match="pvalue"):
        mi.hsic_tests(X, pvalue="gamma")
    with pytest.raises(ValueError, match="pvalue"):
        mi.get_I_from_hsic_tests(X, pvalue="gamma")
    with pytest.raises(ValueError, match="n >= 4"):
        mi.hsic_tests(X[:3], pvalue="chi2")
    with pytest.raises(ValueError, match="tol"):
        mi.hsic_tests(X, pvalue="chi2", tol=1e-2)
