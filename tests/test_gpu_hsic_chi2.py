"""csrc/hsic.hip's pass over every pair on the GPU (`HipHsic.all_pairs`, `hsic_tests(pvalue="chi2")`)
against tests/hsic_u_numpy.py: (a) the O(n^2) definition and (b) the factor identity on numpy factors
(certified against (a) by tests/test_hsic_chi2_cpu.py).

The bars are derived (tests/hsic_u_numpy.py; DESIGN.md, "HSIC chi-square test for every pair"):
cov_U against (a): 1e-12 + B_n(eta), B_n(eta) = (n - 1) / (n - 3) c_n^2 eta (2 + eta), c_n = (4 n - 4) /
(n - 2); against (b), which has its own factorisation: 1e-12 + 2 B_n(eta); R_U: the largest
|R(corner) - R| over the eight corners (cov +- B, var_x +- B, var_y +- B) of (a)'s values, plus 1e-12; p
through the same corners; the biased statistic: test_gpu_hsic.py's 1e-12 + 2 (4 eta)."""
import ctypes as C
import functools

import numpy as np
import pytest

from midagma_amd import _lib
from midagma_amd import mi_tests as mi
from midagma_amd.solver import HipHsic
from tests import hsic_numpy as hn
from tests import hsic_u_numpy as hu

pytestmark = pytest.mark.gpu

ETA = 1e-13
BAR_BIASED = 1e-12 + 2 * (4 * ETA)


@functools.lru_cache(maxsize=None)
def _oracle(n):
    """(X, (a), (b)'s cov_u, (b)'s biased) of hn.data(n); computed once, never written."""
    X = hn.data(n)
    a = hu.cov_u_direct(X)
    b, bia, _ = hu.cov_u_factors(X)
    for arr in (X, a, b, bia):
        arr.setflags(write=False)
    return X, a, b, bia


def _check_against_the_oracles(tag, n, cov, bia, want_a, want_b=None, want_bia=None, eta=ETA):
    B = hu.bound(n, eta)
    dev_a = np.abs(cov - want_a).max()
    print(f"{tag}: cov_U vs the definition, max abs deviation {dev_a:.3e} (bar {hu.ROUND + B:.3e})")
    assert np.array_equal(cov, cov.T) and np.array_equal(bia, bia.T)
    assert dev_a <= hu.ROUND + B
    if want_b is not None:
        dev_b, dev_s = np.abs(cov - want_b).max(), np.abs(bia - want_bia).max()
        print(f"{tag}: vs the identity on numpy factors {dev_b:.3e}; biased {dev_s:.3e}")
        assert dev_b <= hu.ROUND + 2 * B and dev_s <= BAR_BIASED
    R, dR = hu.corner_intervals(want_a, n, B)
    plo, phi = hu.p_interval(R, dR, n)
    got_R = hu.r_u(cov)
    got_p = hu.pvalues(got_R, n)
    print(f"{tag}: R_U max abs deviation {np.abs(got_R - R).max():.3e}")
    assert (np.abs(got_R - R) <= dR + hu.ROUND).all()
    assert ((plo <= got_p) & (got_p <= phi)).all()


# (n, chunk): 0 the rule; 64 puts n at chunk - 1, chunk and chunk + 1; 16 at n = 257 makes 17 chunks
@pytest.mark.parametrize("n,chunk", [(4, 0), (5, 16), (63, 64), (64, 64), (65, 64), (257, 16), (257, 0), (4097, 0),
                                     (4097, 1024)])
def test_shapes_match_the_oracles(n, chunk):
    X, want_a, want_b, want_bia = _oracle(n)
    eng = HipHsic(X)
    try:
        eng.median_bandwidths()
        cov, bia = eng.all_pairs(chunk=chunk)
        cov0, _ = eng.all_pairs()  # (the rule's chunk: what hsic_tests runs)
    finally:
        eng.close()
    _check_against_the_oracles(f"n={n} chunk={chunk}", n, cov, bia, want_a, want_b, want_bia)
    assert not cov[4].any() and not bia[4].any()  # the constant column
    stat, p = mi.hsic_tests(X, pvalue="chi2")
    assert (stat[4, :4] == 0.0).all() and (p[4, :4] == 1.0).all() and (stat[:4, 4] == 0.0).all() and (p[:4, 4] == 1.0).all()
    assert np.isnan(np.diag(stat)).all() and not np.diag(p).any()
    iu = np.triu_indices(5, 1)
    assert np.array_equal(stat[iu], mi._r_u(cov0)[iu]) and np.array_equal(stat, stat.T, equal_nan=True)


# (column of hn.data(257), sigma^2): ranks 15, 22, 55, 151, 47, ., 143, 1, 1 (constant), 195, 31, 27 in numpy
TILE_EDGE_COLUMNS = [(0, 3.0), (1, 0.29), (3, 0.036), (0, 0.004), (1, 0.036), (2, 1.0), (3, 0.002), (0, 1e30), (4, 1.0),
                     (1, 0.001), (0, 0.29), (3, 0.29)]


def test_tile_edges():
    n = 257
    base = hn.data(n)
    X = np.ascontiguousarray(np.column_stack([base[:, c] for c, _ in TILE_EDGE_COLUMNS]))
    s2 = np.array([s for _, s in TILE_EDGE_COLUMNS])
    eng = HipHsic(X)
    try:
        eng.set_bandwidths(s2)
        rank, resid = eng.factor(np.arange(12))
        cov, bia = eng.all_pairs()
        cov16, bia16 = eng.all_pairs(chunk=16)
    finally:
        eng.close()
    rpad = (rank + 15) // 16 * 16
    ends = np.cumsum(rpad)
    starts = ends - rpad
    print(f"tile edges: ranks {rank.tolist()}, R = {ends[-1]}")
    assert {16, 32, 48} <= set(rpad.tolist()) and rpad.max() > 128 and (resid <= ETA).all()
    assert ends[-1] > 2 * 128 and ends[-1] % 128 != 0  # two tile boundaries crossed, a ragged last tile
    assert any(s // 128 != (e - 1) // 128 for s, e in zip(starts, ends))  # a column straddles a boundary
    want_a = hu.cov_u_direct(X, s2)
    want_b, want_bia, _ = hu.cov_u_factors(X, s2)
    _check_against_the_oracles("tile edges", n, cov, bia, want_a, want_b, want_bia)
    _check_against_the_oracles("tile edges, chunk 16", n, cov16, bia16, want_a, want_b, want_bia)


def test_more_columns_than_a_tile_of_vectors():
    """d = 70: the vector panel is 144 wide (two tiles of the vector Grams) and Phi has many tiles."""
    n, d = 97, 70
    X = np.random.default_rng(70).standard_normal((n, d))
    X[:, 1::2] += np.sin(2.0 * X[:, 0::2])
    eng = HipHsic(X)
    try:
        s2 = eng.median_bandwidths()
        cov, bia = eng.all_pairs(chunk=32)
    finally:
        eng.close()
    _check_against_the_oracles("d=70", n, cov, bia, hu.cov_u_direct(X, s2))


@pytest.mark.parametrize("n,d", [(4097, 5), (16384, 6)])
def test_biased_agrees_with_the_shipped_path(n, d):
    X = hn.data(n)
    if d == 6:
        X = np.ascontiguousarray(np.column_stack([X, np.random.default_rng(n).standard_normal(n) + 0.5 * X[:, 0] ** 2]))
    pairs = [(i, j) for i in range(d) for j in range(i + 1, d)]
    stat, _, _ = mi.hsic_null(X, pairs, num_perm=0)
    eng = HipHsic(X)
    try:
        eng.median_bandwidths()
        _, bia = eng.all_pairs()
    finally:
        eng.close()
    got = np.array([bia[i, j] for i, j in pairs])
    print(f"n={n} d={d}: biased vs hsic_null(num_perm=0), max abs deviation {np.abs(got - stat).max():.3e}")
    assert np.abs(got - stat).max() <= 2 * 1e-12
    assert stat.max() > 1e-3  # (the dependent pair: the agreement is not 0 = 0)


def test_runs_budgets_and_column_lists_give_identical_bits():
    X = hn.data(1000)
    eng = HipHsic(X)
    try:
        eng.median_bandwidths()
        first = eng.all_pairs()
        again = eng.all_pairs()
        # a factor and its vectors are about 272 kB (r_pad 32): at 1 and 1.2 MB every column is a group of
        # its own (15 group pairs, every column refactored as it returns), at 2 MB a group is one or two
        small = [eng.all_pairs(budget_bytes=b) for b in (1, 1_200_000, 2_000_000)]
        back = eng.all_pairs()
        sub = [3, 0, 1]
        part = eng.all_pairs(sub)
        part_small = eng.all_pairs(sub, budget_bytes=1)
        dup = eng.all_pairs([1, 1, 3])
    finally:
        eng.close()
    for o in [again, back] + small:
        assert all(np.array_equal(a, b) for a, b in zip(o, first))
    eng = HipHsic(X)  # groups on an engine that knows no rank yet: the columns are factored once to size them
    try:
        eng.median_bandwidths()
        fresh = eng.all_pairs(budget_bytes=1_200_000)
    finally:
        eng.close()
    assert all(np.array_equal(a, b) for a, b in zip(fresh, first))
    for a, b in zip(part, first):
        assert np.array_equal(a, b[np.ix_(sub, sub)])
    assert all(np.array_equal(a, b) for a, b in zip(part, part_small))
    for a, b in zip(dup, first):
        assert np.array_equal(a, b[np.ix_([1, 1, 3], [1, 1, 3])])
    assert first[0][0, 1] > 0 and first[1][0, 1] > 0


def test_host_and_device_X_give_identical_bits_and_X_is_not_written():
    import torch
    X = hn.data(1000, seed=4)
    X0 = X.copy()
    s_host, p_host = mi.hsic_tests(X, pvalue="chi2")
    assert np.array_equal(X, X0)
    Xd = torch.from_numpy(X).cuda()
    wide = torch.zeros((1000, 7), dtype=torch.float64, device="cuda")
    wide[:, :5] = Xd
    for T in (Xd, wide[:, :5]):  # contiguous, and a row stride above d
        keep = T.clone()
        s_dev, p_dev = mi.hsic_tests(T, pvalue="chi2")
        assert np.array_equal(s_host, s_dev, equal_nan=True) and np.array_equal(p_host, p_dev)
        assert torch.equal(T, keep)


def test_public_api_matches_the_definition():
    X = hu.api_case()
    n, d = X.shape
    want = hu.cov_u_direct(X)
    R, dR = hu.corner_intervals(want, n, hu.bound(n, ETA))
    plo, phi = hu.p_interval(R, dR, n)
    stat, p = mi.hsic_tests(X, pvalue="chi2")
    iu = np.triu_indices(d, 1)
    print(f"api: R_U max abs deviation {np.abs(stat[iu] - R[iu]).max():.3e}")
    assert (np.abs(stat[iu] - R[iu]) <= dR[iu] + hu.ROUND).all()
    assert ((plo[iu] <= p[iu]) & (p[iu] <= phi[iu])).all()
    assert np.array_equal(stat, stat.T, equal_nan=True) and np.array_equal(p, p.T)
    assert np.isnan(np.diag(stat)).all() and not np.diag(p).any()
    want_I, alpha_eff = hu.pair_set(hu.pvalues(R, n))
    excused = (plo[iu] <= alpha_eff) & (alpha_eff <= phi[iu])
    assert excused.sum() <= 1
    I = mi.get_I_from_hsic_tests(X, alpha=hu.API_ALPHA, pvalue="chi2")
    assert I.dtype == np.asarray([], dtype=int).dtype
    firm = {(int(i), int(j)) for (i, j), e in zip(zip(*iu), excused) if not e}
    assert {tuple(r) for r in I.tolist()} & firm == {tuple(r) for r in want_I.tolist()} & firm
    assert np.array_equal(I, hu.pair_set(p)[0])  # (the reference's pair order)


def test_the_permutation_route_is_unchanged():
    X = hn.data(257)
    a = mi.hsic_tests(X, num_perm=6, seed=3)
    b = mi.hsic_tests(X, pvalue="permutation", num_perm=6, seed=3)
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])
    stat, ge, _ = mi.hsic_null(X, hn.ALL_PAIRS_5, num_perm=6, seed=3, perms="device")
    iu = np.triu_indices(5, 1)
    assert np.array_equal(a[0][iu], stat) and np.array_equal(a[1][iu], (ge + 1.0) / 7.0)
    Ia = mi.get_I_from_hsic_tests(X, num_perm=6, seed=3)
    Ib = mi.get_I_from_hsic_tests(X, pvalue="permutation", num_perm=6, seed=3)
    assert np.array_equal(Ia, Ib)


def test_error_paths():
    X = hn.data(97)
    with pytest.raises(ValueError, match="n >= 4"):
        mi.hsic_tests(X[:3], pvalue="chi2")
    with pytest.raises(ValueError, match="pvalue"):
        mi.hsic_tests(X, pvalue="gamma")
    eng = HipHsic(X[:3])
    try:
        eng.median_bandwidths()
        with pytest.raises(ValueError, match="needs n >= 4"):
            eng.all_pairs()
        eng.set_data(X)
        with pytest.raises(ValueError, match="set the bandwidths first"):
            eng.all_pairs()
        eng.median_bandwidths()
        with pytest.raises(ValueError, match=r"column index outside \[0, d\)"):
            eng.all_pairs([0, 5])
        with pytest.raises(ValueError, match=r"column index outside \[0, d\)"):
            eng.all_pairs([-1])
        with pytest.raises(ValueError, match="tol must be in"):
            eng.all_pairs(tol=1e-2)
        with pytest.raises(ValueError, match="chunk"):
            eng.all_pairs(chunk=24)
        L = _lib.lib()
        cols = np.array([0, 1], dtype=np.int64)
        rc = L.midagma_hsic_all_pairs(eng.h, C.c_void_p(cols.ctypes.data), 2, 1e-13, 0, 0, None, None)
        assert rc == _lib.E_ARG and b"null pointer" in L.midagma_hsic_last_error(eng.h)
        cov, bia = eng.all_pairs([0, 1])  # the engine still works, and biased_out may be NULL
        only = np.zeros((2, 2))
        assert L.midagma_hsic_all_pairs(eng.h, C.c_void_p(cols.ctypes.data), 2, 1e-13, 0, 0, _lib.dptr(only), None) == _lib.OK
        assert np.array_equal(only, cov) and cov[0, 1] > 0
        e0, e1 = eng.all_pairs([])
        assert e0.shape == (0, 0) and e1.shape == (0, 0)
        prof = eng.all_pairs_profile()
        assert set(prof) == {"factor_ms", "tile_ms", "vector_ms"}
    finally:
        eng.close()


def test_live_bytes_return_to_the_baseline_after_close():
    L = _lib.lib()
    base = L.midagma_debug_live_bytes()
    eng = HipHsic(hn.data(1000))
    eng.median_bandwidths()
    eng.all_pairs()
    eng.all_pairs(budget_bytes=1)
    assert L.midagma_debug_live_bytes() > base
    eng.close()
    assert L.midagma_debug_live_bytes() == base
