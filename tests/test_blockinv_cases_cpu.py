"""The premises of tests/test_gpu_blockinv.py, checked without a GPU: the matrix family of
tests/blockinv_cases.py is as ill-conditioned as its table says and still an M-matrix, the checker
passes LAPACK against itself at ratio 1 and the reference algorithm (unpivoted block Gauss-Jordan)
within 2x, the "fast" bands' warm starts lie far under the series' 0.25 gate, the "far" band's
above it, and the line-search band makes the oracle halve."""
import numpy as np
import pytest
import scipy.linalg as sla

from tests import blockinv_cases as bc

DS = (100, 300)
SCALES = (0.3, 0.6, 0.8)


@pytest.fixture(scope="module")
def oracles():
    return {d: bc.make_oracle(d) for d in DS}


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("scale", SCALES)
def test_family_is_ill_conditioned_and_in_domain(d, scale):
    W = bc.make_W(d, scale, d)
    assert np.all(np.diag(W) == 0)
    A = bc.a_matrix(W)
    rho = float(np.abs(np.linalg.eigvals(W * W)).max())
    M = sla.inv(A)
    cond1 = float(np.abs(A).sum(0).max() * np.abs(M).sum(0).max())
    rho_t, cond_t = bc.TABLE[scale][d]
    print(f"d={d} scale={scale}: rho={rho:.3f} cond1={cond1:.3g} min M={M.min():.3g}")
    assert rho_t / 2 <= rho <= min(2 * rho_t, 1.0) and rho < 1.0
    assert cond_t / 2 <= cond1 <= 2 * cond_t
    assert M.min() > 0


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("scale", SCALES)
def test_checker_on_lapack_and_block_gauss_jordan(d, scale):
    W = bc.make_W(d, scale, d)
    A = bc.a_matrix(W)
    # LAPACK against itself: ratio 1; the forward one is below 1 where the 2^-50 max|X| floor is the
    # larger term of its denominator (d = 100: LAPACK's own error is 0.4 - 0.7 of the floor)
    res, fwd = bc.check_inverse(W, sla.inv(A).T.copy())
    assert res == 1.0 and 0.1 <= fwd <= 1.0, (res, fwd)
    res, fwd = bc.check_inverse(W, bc.block_gj_inverse(A).T.copy())
    print(f"d={d} scale={scale}: block GJ residual ratio {res:.2f}, forward ratio {fwd:.2f}")
    assert res <= 2.0 and fwd <= 2.0


def test_checker_rejects_a_1e7_block_column_error():
    """What the GPU tests are for: a 1e-7 relative error in one 32-wide block column fails both
    checks by orders of magnitude."""
    d = 100
    W = bc.make_W(d, 0.6, d)
    Mt = sla.inv(bc.a_matrix(W)).T.copy()
    Mt[32:64, :] *= 1 + 1e-7
    with pytest.raises(AssertionError):
        bc.check_inverse(W, Mt)
    with pytest.raises(AssertionError):
        bc.check_inverse(W, Mt, forward=False)


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("scale,lr", bc.FAST_BANDS)
def test_fast_bands_warm_start_under_the_gate(oracles, d, scale, lr):
    r1, r2 = bc.warm_start_residuals(oracles[d], bc.make_W(d, scale, d), lr)
    print(f"d={d} scale={scale} lr={lr}: first warm slot {r1:.3g}, extrapolated {r2:.3g}")
    assert r1 <= 0.1 and r2 <= 0.1


@pytest.mark.parametrize("d", DS)
def test_near_band_warm_start_converges_in_two_passes(oracles, d):
    """Two passes finish a block from a residual <= 1e-4 (its square is the 1e-8 bar); the near
    band stays 4x under that."""
    scale, lr = bc.NEAR_BAND
    r1, r2 = bc.warm_start_residuals(oracles[d], bc.make_W(d, scale, d), lr)
    print(f"d={d}: first warm slot {r1:.3g}, extrapolated {r2:.3g}")
    assert r1 <= 2.5e-5 and r2 <= 2.5e-5


def test_far_band_warm_start_over_the_gate(oracles):
    """At d = 300, the smaller of the two sizes the far-warm-start GPU test runs (1.77 here, 1.80 at
    d = 1000).  The residual grows with d: at d = 100 it is 0.19, under the gate, which is why that
    test does not run there."""
    scale, lr = bc.FAR_BAND
    r1, _ = bc.warm_start_residuals(oracles[300], bc.make_W(300, scale, 300), lr)
    print(f"d=300: first warm slot residual {r1:.3g}")
    assert r1 >= 1.0


@pytest.mark.parametrize("d", DS)
def test_line_search_band_halves(oracles, d):
    scale, lr = bc.SEARCH_BAND
    _, tr = oracles[d].minimize(bc.make_W(d, scale, d), 1.0, 12, 1.0, lr, tol=-1.0)
    print(f"d={d}: halvings {tr.halvings}, iters {tr.iters}, lr {tr.lr_final}")
    assert tr.halvings >= 1
