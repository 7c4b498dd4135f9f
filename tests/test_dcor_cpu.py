"""The dCor path without the n^2 sum, on the CPU: tests/dcor_numpy.py (the restatement of
csrc/dcor.hip) against the reference's formulas written out by brute force and against the
reference's recorded results, the seeds the GPU tests rely on, the permutation rule, and the
argument checks of the C entries and the Python functions (no device is opened by any of them).

The bar on the statistics is 1e-12 absolute on stat^2 (R^2 = dcov^2 / sqrt(dvar_x^2 dvar_y^2), R_U
for the bias-corrected form), tests/test_gpu_indep.py's bar for these statistics.  The worst
deviation measured here is 8.5e-15 against the brute-force formulas (n <= 1000) and 2.2e-14
against the recorded reference."""
import ctypes as C

import numpy as np
import pytest

from midagma_amd import _lib
from midagma_amd import mi_tests as mi
from tests import dcor_numpy as dn
from tests import indep_numpy as inp

SIZES = (2, 3, 4, 5, 64, 65, 97, 257, 1000)
EDGES = (4, 16, 64, 0)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("indep.npz")


@pytest.mark.parametrize("n", SIZES)
def test_restatement_matches_the_reference_formula_by_brute_force(n):
    worst = 0.0
    for kind in dn.KINDS:
        x, y = dn.make_columns(kind, n, seed=n)
        cx, cy = dn.column_prep(x), dn.column_prep(y)
        zero = np.ptp(x) == 0 or np.ptp(y) == 0
        d2, vx, vy = dn.brute_values(x, y)  # mi_tests.py:68-101: the centred n x n matrices
        want = 0.0 if (zero or vx <= 0 or vy <= 0) else d2 / np.sqrt(vx * vy)
        if n >= 4:
            u, ux, uy = dn.brute_values_u(x, y)
            want_u = 0.0 if (zero or ux <= 0 or uy <= 0) else u / np.sqrt(ux * uy)
        for m in EDGES:
            got = dn.r2_of(dn.dcov2(cx, cy, None, m), cx, cy)
            worst = max(worst, abs(got - want))
            assert abs(got - want) <= 1e-12, (kind, m, got, want)
            if n >= 4:
                got_u = dn.r2_of(dn.dcov2(cx, cy, None, m, True), cx, cy, True)
                worst = max(worst, abs(got_u - want_u))
                assert abs(got_u - want_u) <= 1e-12, (kind, m, got_u, want_u)
    print(f"n={n}: restatement vs brute force, worst |stat^2 deviation| {worst:.3e}")


def test_restatement_under_a_permutation_matches_brute_force():
    rng = np.random.default_rng(5)
    for n, m in ((97, 16), (130, 4), (257, 0)):
        x, y = dn.make_columns("rounded", n, seed=n)
        cx, cy = dn.column_prep(x), dn.column_prep(y)
        pi = rng.permutation(n)
        d2, vx, vy = dn.brute_values(x, y[pi])
        for unbiased in (False, True):
            if unbiased:
                d2, vx, vy = dn.brute_values_u(x, y[pi])
            got = dn.r2_of(dn.dcov2(cx, cy, pi, m, unbiased), cx, cy, unbiased)
            assert abs(got - d2 / np.sqrt(vx * vy)) <= 1e-12


@pytest.mark.parametrize("case", inp.CASES)
def test_restatement_matches_the_recorded_reference(fx, case):
    X, pairs, P, seed = fx[f"{case}/X"], fx[f"{case}/pairs"], int(fx[f"{case}/P"]), int(fx[f"{case}/seed"])
    perms = inp.numpy_perms(seed, len(pairs), P, X.shape[0])
    stat, ge, null, _ = dn.dcor_null(X, pairs, perms)
    dev = max(np.abs(stat - fx[f"{case}/dcor/stat"]).max(), np.abs(null - fx[f"{case}/dcor/null"]).max())
    print(f"{case}: restatement vs reference, max abs deviation {dev:.3e}")
    assert dev <= 1e-12
    assert np.array_equal(ge, fx[f"{case}/dcor/ge"])
    assert np.array_equal((ge + 1) / (P + 1), fx[f"{case}/dcor/pvalue"])


def test_row_sums_match_the_distance_matrix():
    for kind in dn.KINDS:
        x, _ = dn.make_columns(kind, 97, seed=3)
        c = dn.column_prep(x)
        a = np.abs(x[:, None] - x[None, :])
        assert np.abs(c["rs"] - a.sum(1)).max() <= 1e-10 * max(1.0, a.sum(1).max())
        assert sorted(c["order"].tolist()) == list(range(97)) and np.all(np.diff(x[c["order"]]) >= 0)


def test_permutation_rule_gives_distinct_bijections():
    n, P = 97, 5
    perms = np.stack([dn.philox_perms(7, q, P, n) for q in range(3)])
    assert perms.shape == (3, P, n)
    assert (np.sort(perms, axis=-1) == np.arange(n)).all()
    flat = {tuple(r) for r in perms.reshape(-1, n).tolist()}
    assert len(flat) == 3 * P  # different (q, p) differ
    assert not np.array_equal(dn.philox_perms(8, 0, P, n), perms[0])  # and so do seeds
    # no packing of a into the key: n beyond indep's 2^14 is a bijection too
    big = dn.philox_perms(7, 1, 1, 70001)[0]
    assert np.array_equal(np.sort(big), np.arange(70001))


def test_big_case_keeps_permuted_values_away_from_the_observed():
    """tests/test_gpu_dcor.py compares ge at n = 16384 with the n^2 kernel: the seed must keep every
    permuted dcov^2 at least 1e-6 relative from the observed one (the fixture's perm_guard)."""
    X, perms = dn.big_case()
    _, _, _, vals = dn.dcor_null(X, dn.BIG_PAIRS, perms)
    gap = np.abs(vals[:, 1:] - vals[:, :1]) / np.abs(vals[:, :1])
    assert gap.min() >= 1e-6, gap.min()


def test_chi2_seeds_are_decisive():
    for seed in dn.CHI2_SEEDS:
        r, _, _, _ = dn.dcor_null(dn.chi2_case(seed), [(0, 1), (0, 2)], None, 0, True)
        p = dn.chi2_pvalue(dn.CHI2_N, r)
        assert p[0] > 0.05 and p[1] < 1e-6, (seed, p)


def test_block_edge_rule():
    L = _lib.lib()
    for n in (1, 2, 64, 4096, 4097, 16384, 16385, 70001, 10**6, 2**31 - 1):
        assert L.midagma_dcor_block(n) == dn.block_edge(n)
    assert (dn.block_edge(4096), dn.block_edge(4097), dn.block_edge(16384), dn.block_edge(10**6)) == (64, 128, 128, 1024)


# --- argument checks: every one is answered before a device is touched -----------------------------
def _err(h=None):
    m = _lib.lib().midagma_dcor_last_error(h)
    return m.decode() if m else ""


def test_c_entries_check_their_arguments_without_a_device():
    L = _lib.lib()
    buf = np.zeros(16)
    out = np.zeros(16, dtype=np.int32)
    X, O = C.c_void_p(buf.ctypes.data), C.c_void_p(out.ctypes.data)
    for args in ((None, 4, 2, 2, O), (X, 4, 2, 2, None), (X, 1, 2, 2, O), (X, 2**31, 2, 2, O), (X, 4, 0, 2, O),
                 (X, 4, 65536, 65536, O), (X, 4, 2, 1, O)):
        assert L.midagma_colargsort(args[0], args[1], args[2], args[3], args[4], 0, None) == _lib.E_ARG
    assert "colargsort" in _lib.last_error(None)

    assert L.midagma_dcor_create(None, 0) == _lib.E_ARG
    h = C.c_void_p()
    assert L.midagma_dcor_create(C.byref(h), -1) == _lib.E_ARG
    assert L.midagma_dcor_set_data(None, _lib.dptr(buf), 4, 2, 0) == _lib.E_ARG
    assert L.midagma_dcor_run(None, None, 0, 0, None, 0, 0, 0, 0, None, None, None) == _lib.E_ARG
    assert L.midagma_dcor_create(C.byref(h), 0) == _lib.OK and h.value
    try:
        for n, d in ((1, 2), (2**31, 2), (4, 0), (4, 65536)):
            assert L.midagma_dcor_set_data(h, _lib.dptr(buf), n, d, 0) == _lib.E_ARG, (n, d)
        assert L.midagma_dcor_set_data(h, None, 4, 2, 0) == _lib.E_ARG
        for n, d, ld in ((1, 2, 2), (2**31, 2, 2), (4, 0, 2), (4, 65536, 65536), (4, 2, 1)):
            assert L.midagma_dcor_set_data_dev(h, X, n, d, ld, 0, None) == _lib.E_ARG, (n, d, ld)
        assert "leading dimension" in _err(h)
        assert L.midagma_dcor_set_data_dev(h, None, 4, 2, 2, 0, None) == _lib.E_ARG
        pairs = np.array([[0, 1]], dtype=np.int64)
        stat, ge = np.zeros(1), np.zeros(1, dtype=np.int64)
        PP, G = C.c_void_p(pairs.ctypes.data), C.c_void_p(ge.ctypes.data)

        def run(pp=PP, m=1, P=0, block=0, st=_lib.dptr(stat), g=G):
            return L.midagma_dcor_run(h, pp, m, P, None, 0, 0, block, 0, st, g, None)

        assert run(pp=None) == _lib.E_ARG and run(st=None) == _lib.E_ARG and run(g=None) == _lib.E_ARG
        assert run(P=-1) == _lib.E_ARG and run(P=65536) == _lib.E_ARG and run(m=-1) == _lib.E_ARG
        for block in (1, 3, -4, 1025):
            assert run(block=block) == _lib.E_ARG and "block" in _err(h)
        assert run() == _lib.E_ARG and "set the data first" in _err(h)
        assert L.midagma_dcor_perms(h, 0, 1, 0, O, None) == _lib.E_ARG
    finally:
        L.midagma_dcor_destroy(h)
    L.midagma_dcor_destroy(None)


def test_python_functions_check_their_arguments_without_a_device():
    X = np.random.default_rng(0).standard_normal((8, 3))
    with pytest.raises(ValueError, match="perms"):
        mi.dcor_null(X, [(0, 1)], perms="host")
    with pytest.raises(ValueError, match="num_perm"):
        mi.dcor_null(X, [(0, 1)], num_perm=-1)
    with pytest.raises(ValueError, match="pair index"):
        mi.dcor_null(X, [(0, 3)])
    with pytest.raises(ValueError, match="block"):
        mi.dcor_null(X, [(0, 1)], block=3)
    with pytest.raises(ValueError, match="block"):
        mi.dcor_null(X, [(0, 1)], block=2048)
    with pytest.raises(ValueError, match="n >= 4"):
        mi.dcor_null(X[:3], [(0, 1)], unbiased=True)
    with pytest.raises(ValueError, match="perms must be"):
        mi.dcor_null(X, [(0, 1)], num_perm=2, perms=np.zeros((1, 2, 7), dtype=np.int32))
    with pytest.raises(ValueError, match="inf or nan"):
        mi.dcor_null(np.where(X > 2, np.nan, np.inf), [(0, 1)])
    with pytest.raises(ValueError, match="2-d"):
        mi.dcor_null(X[:, 0], [(0, 1)])
    with pytest.raises(ValueError, match="at least 2"):
        mi.dcor_tests(X[:1])
    with pytest.raises(ValueError, match="pvalue"):
        mi.dcor_tests(X, pvalue="exact")
    with pytest.raises(ValueError, match="n >= 4"):
        mi.dcor_tests(X[:3], pvalue="chi2")
    with pytest.raises(ValueError, match="perms"):
        mi.get_I_from_dcor_tests(X, perms="host")
    with pytest.raises(ValueError, match="pvalue"):
        mi.get_I_from_dcor_tests(X, pvalue="exact")


def test_I_from_pvalues_follows_the_correlation_builder():
    p = np.array([[0.0, 0.2, 0.001], [0.2, 0.0, 0.04], [0.001, 0.04, 0.0]])
    assert mi._I_from_pvalues(p, 0.05, False, True, True).tolist() == [[0, 1]]
    assert mi._I_from_pvalues(p, 0.05, True, True, True).tolist() == [[0, 1], [1, 2]]
    assert mi._I_from_pvalues(p, 0.05, False, False, True).tolist() == [[0, 1], [1, 0]]
    assert len(mi._I_from_pvalues(p, 0.05, False, False, False)) == 2  # the diagonal's p is 0
    empty = mi._I_from_pvalues(p, 0.5, False, True, True)
    assert empty.size == 0 and empty.dtype == np.asarray([], dtype=int).dtype
