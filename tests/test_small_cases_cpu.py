"""The premises of tests/test_gpu_small_inverse.py, checked without a GPU, from the oracle's own steps.

The one-workgroup loop (csrc/small.hip) picks a warm slot's inverse from g = d max|I - A^T X0|:
two series passes (g <= 1e-4), three (g <= 1e-2) or the Gauss-Jordan fall-back, which it also
takes when max|X0| > 512.  For every cell of blockinv_cases.small_cells() this file computes g and
max|X0| of iterations 2..5 with LAPACK's inverses as the warm starts, and asserts the form
blockinv_cases lists for each slot with a factor 3 to both gates on g, every form at every DS.  It then
shows that the forms are needed where the GPU file relies on it: the series in numpy with one pass
too few fails check_inverse in the dense band (three -> two passes, at every d) and in the wide
band (fall-back -> three passes), and the ungated series fails it on some slot of every steep cell
(max|X0| 550 - 1200 with g far under 1e-2).  In the four bands of the make_W family the shorter
form passes as well, which is why those bands exist.

The slot after a halving (warm = 1, X0 the inverse of the out-of-domain W) is always a fall-back:
see test_slots_after_a_halving_always_fall_back.

Line search: the halving counts of the search band, the out-of-domain failure at s = 0.9, and that
no domain decision of any run the GPU file compares with the oracle hangs on rounding (margin of
min(inv + 1e-16) against max|inv|, and the same decisions and end point under 1e-16 relative noise
in every inverse)."""
import numpy as np
import pytest

from tests import blockinv_cases as bc

ALL_D = sorted(d for ds in bc.SMALL_DS.values() for d in ds)
SEARCH_GPU_D = (7, 16, 20, 32, 48, 64)

_ORACLES = {}


def _oracle(d):
    if d not in _ORACLES:
        _ORACLES[d] = bc.small_oracle(d)
    return _ORACLES[d]


_STARTS = {}


def _starts(d, band):
    """(W_k, X0_k) of iterations 2..5 and their g."""
    if (d, band) not in _STARTS:
        W0, lr, _ = bc.small_cell(d, band)
        ws = bc.small_warm_starts(_oracle(d), W0, lr)
        _STARTS[d, band] = ws, [(bc.small_gate(W, X0), float(np.abs(X0).max())) for W, X0 in ws]
    return _STARTS[d, band]


@pytest.mark.parametrize("d", (5, 7, 16, 17, 20, 32, 33, 48, 64))
def test_family_is_in_domain_at_small_d(d):
    rhos, conds = [], []
    for scale in (0.3, 0.6, 0.8):
        W = bc.make_W(d, scale, d)
        M = np.linalg.inv(bc.a_matrix(W))
        h = -np.linalg.slogdet(bc.a_matrix(W))[1]
        rhos.append(float(np.abs(np.linalg.eigvals(W * W)).max()))
        conds.append(float(np.abs(bc.a_matrix(W)).sum(0).max() * np.abs(M).sum(0).max()))
        print(f"d={d} scale={scale}: rho={rhos[-1]:.3f} cond1={conds[-1]:.3g} h={h:.3g} min M={M.min():.3g}")
        assert M.min() > 0 and rhos[-1] < 1.0
    assert 0.1 <= rhos[0] and rhos[-1] <= 0.98 and 2.0 <= conds[0] and conds[-1] <= 5e4


@pytest.mark.parametrize("d", ALL_D)
def test_dense_start_is_in_domain(d):
    rho = bc.SMALL_DENSE_RHO[d]
    W = bc.small_dense_W(d, rho, d)
    assert np.all(np.diag(W) == 0) and np.ptp(np.abs(W[~np.eye(d, dtype=bool)])) == 0
    assert abs(float(np.abs(np.linalg.eigvals(W * W)).max()) - rho) <= 1e-12
    assert np.linalg.inv(bc.a_matrix(W)).min() > 0


@pytest.mark.parametrize("d,band", bc.small_cells())
def test_every_slot_takes_the_listed_form(d, band):
    _, g = _starts(d, band)
    forms = bc.small_cell(d, band)[2]
    got = [bc.small_form(x, xmax) for x, xmax in g]
    print(f"d={d} {band}: g(2..5) = " + " ".join(f"{x:.2e}" for x, _ in g) + f", max|X0| {max(x for _, x in g):.3g} -> {got}")
    assert None not in got, f"within a factor {bc.SMALL_MARGIN} of a gate: {g}"
    assert "".join(got) == forms


@pytest.mark.parametrize("ds", sorted(bc.SMALL_DS))
def test_every_form_occurs_at_every_ds(ds):
    """Both as the first warm slot (X0 = P(k-1), warm = 1) and as an extrapolated one."""
    first, later = set(), set()
    for d, band in bc.small_cells():
        if d in bc.SMALL_DS[ds]:
            forms = bc.small_cell(d, band)[2]
            first.add(forms[0])
            later |= set(forms[1:])
    assert first == later == {"2", "3", "G"}


def _passes(W, Mt):
    try:
        bc.check_inverse(W, Mt)
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("d", ALL_D)
def test_dense_band_needs_its_third_pass(d):
    """Iteration 2 of the dense band: g ~ 3e-3, three passes pass the checker, two do not."""
    (W, X0), (g, xmax) = _starts(d, "dense")[0][0], _starts(d, "dense")[1][0]
    assert bc.small_form(g, xmax) == "3"
    assert _passes(W, bc.product_form_inverse(W, X0, 3))
    assert not _passes(W, bc.product_form_inverse(W, X0, 2))


@pytest.mark.parametrize("d", ALL_D)
def test_wide_band_needs_its_fall_back(d):
    """Iteration 2 of the wide band: 3e-2 <= g < 1, so a 1e-2 gate moved to 1 would let the slot
    through, and three passes from it fail the checker."""
    (W, X0), (g, xmax) = _starts(d, "wide")[0][0], _starts(d, "wide")[1][0]
    assert bc.small_form(g, 0.0) == "G" and g <= 0.95 and xmax <= 100.0
    assert not _passes(W, bc.product_form_inverse(W, X0, 3))


@pytest.mark.parametrize("d", sorted(bc.SMALL_STEEP))
def test_steep_band_needs_the_xmax_gate(d):
    """g alone says three passes, then two (a factor 3 under its gates), max|X0| is over 512, and
    the series of that form misses the checker on at least one of the four slots."""
    ws, gx = _starts(d, "steep")
    assert [bc.small_form(g, 0.0) for g, _ in gx] == ["3", "2", "2", "2"]
    assert all(x >= bc.SMALL_GATE_XMAX * bc.SMALL_XMAX_MARGIN for _, x in gx)
    ok = [_passes(W, bc.product_form_inverse(W, X0, 3 if k == 0 else 2)) for k, (W, X0) in enumerate(ws)]
    print(f"d={d} steep: max|X0| {gx[0][1]:.0f}, ungated series passes the checker on slots 2..5: {ok}")
    assert not all(ok)


@pytest.mark.parametrize("d", SEARCH_GPU_D)
def test_slots_after_a_halving_always_fall_back(d):
    """The issue expected the slot after a halving to be a warm = 1 product-form slot.  It cannot be.
    The slot that halves inverted an A_bad = sI - W_bad∘W_bad outside the domain (rho(W∘W) > s, so
    A_bad has a negative real eigenvalue); the next slot's W lies half the step back towards the last
    W inside it.  If that W is inside, det(A) > 0 > det(A_bad) when one eigenvalue has crossed, so
    I - R = A inv(A_bad) has a negative real eigenvalue and rho(R) > 1.  If it is still outside (the
    next halving), rho(W∘W) - s has at least halved to first order, and R has an eigenvalue near
    1 - (rho - s) / (rho_bad - s) >= 1/2.  g = d max|R| >= ||R||_inf >= rho(R), so every such slot is
    at least 50x over the 1e-2 gate, and the slot after it (2 P(k-1) - P(k-2) with P(k-2) from
    outside the domain) is no nearer.  Here: every warm slot of every line-search run the GPU file
    makes has g >= 0.5, the slots after a halving g >= 5.  `warm = 1` after ACT_HALVE therefore
    selects between two warm starts that are both refused; no output depends on it."""
    scale, lr = bc.SMALL_SEARCH
    slots = bc.small_slot_gates(_oracle(d), bc.make_W(d, scale, d), lr, 1.0)
    after = [g for a, g, _ in slots if a]
    print(f"d={d}: {len(slots)} warm slots, min g {min(g for _, g, _ in slots):.3g}; after a halving: "
          + " ".join(f"{g:.3g}" for g in after))
    assert after and min(after) >= 0.5
    assert min(g for _, g, _ in slots) >= bc.SMALL_GATE_GJ * bc.SMALL_MARGIN


@pytest.mark.parametrize("d,band", [c for c in bc.small_cells() if c[1] not in ("dense", "wide", "steep")][::3])
def test_listed_form_passes_the_checker_in_numpy(d, band):
    """The series as the kernel runs it, in numpy: every product-form slot of the listed form passes."""
    ws, _ = _starts(d, band)
    for (W, X0), f in zip(ws, bc.small_cell(d, band)[2]):
        if f != "G":
            bc.check_inverse(W, bc.product_form_inverse(W, X0, int(f)))


def _decisions_hold(d, W0, lr, s, want=None):
    o = _oracle(d)
    W, tr, margins = bc.domain_decisions(o, W0, lr, s)
    key = (tr.iters, tr.success, tr.halvings, tr.lr_final)
    print(f"d={d} lr={lr} s={s}: iters {tr.iters} halvings {tr.halvings} success {tr.success}, "
          f"smallest margin {min(margins):.2e} over {len(margins)} decisions")
    if want is not None:
        assert key[:3] == want, key
    assert min(margins) >= 1e-10
    Wn, trn, _ = bc.domain_decisions(o, W0, lr, s, noise_seed=1)
    assert (trn.iters, trn.success, trn.halvings, trn.lr_final) == key
    assert np.abs(W - Wn).max() <= 1e-10
    return tr


@pytest.mark.parametrize("d", sorted(bc.SMALL_SEARCH_HALVINGS))
def test_search_band_halvings_and_failure(d):
    scale, lr = bc.SMALL_SEARCH
    _decisions_hold(d, bc.make_W(d, scale, d), lr, 1.0, want=(12, True, bc.SMALL_SEARCH_HALVINGS[d]))
    _decisions_hold(d, bc.make_W(d, scale, d), lr, 0.9, want=(0 if d == 32 else 1, False, 0))


@pytest.mark.parametrize("d,band", bc.small_cells())
def test_trajectory_cells_do_not_hang_on_rounding(d, band):
    """The 12 steps the GPU file compares with the oracle at 1e-9: no halving, and 1e-16 relative
    noise in every inverse moves the end point by less than 1e-10."""
    W0, lr, _ = bc.small_cell(d, band)
    _decisions_hold(d, W0, lr, 1.0, want=(12, True, 0))


@pytest.mark.parametrize("d", (16, 20, 48))
def test_batch_starts_are_in_domain(d):
    """The batch test's problems 0..2 (scales 0.3 / 0.6 / 0.8 at lr 3e-4): 12 steps without a halving."""
    for scale in (0.3, 0.6, 0.8):
        _decisions_hold(d, bc.make_W(d, scale, d), 3e-4, 1.0, want=(12, True, 0))
