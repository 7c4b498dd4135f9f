"""The one-workgroup small-d loop (csrc/small.hip, d <= 64) at ill-conditioned W: every inverse form
at every resource regime (DS = 16 one wave, 32 four waves, 64 sixteen waves with single-buffered
images), across launch boundaries, through the line search and in the batch.

Every other test of this kernel starts at W = 0 with lr = 3e-4, where A = sI - W∘W ≈ I: every warm
start converges in two passes, the h-gradient is 1e-3 of the step and h itself ~1e-3, so a wrong
third pass, gate constant, barrier or pivot moves nothing a test looks at.  Here W0 comes from
tests/blockinv_cases.py (small_cells: four bands of the make_W family, rho(W∘W) up to 0.97, cond_1
up to 3.4e4, h 0.5 .. 8, and the wide, dense and steep bands, in which the form taken is the only
one that passes), and every slot's inverse is read back with the read-only hook
midagma_debug_slot_matrices (the image the kernel stores for the next launch's warm start) and
checked by blockinv_cases.check_inverse: two-sided residual <= 8x LAPACK's and forward error <= 8x
LAPACK's against a longdouble-refined inverse.  Which form each slot takes (two or three series
passes, or the Gauss-Jordan fall-back, from g = d max|R| and max|X0|) is pinned on the CPU, from the
oracle's steps, with a factor 3 to both gates on g, by tests/test_small_cases_cpu.py; it shows there
too, with the series in numpy, that one pass fewer fails this checker in the dense band, three
passes in place of the fall-back in the wide band, and the ungated series in the steep band.

Largest ratios measured on an MI355X (residual / forward, of the bar 8), per DS and form, over all
cells and the five slots of test_every_slot_inverse:

    form                      DS 16 (d 5, 16)   DS 32 (d 17, 20, 32)   DS 64 (d 33, 48, 64)
    cold Gauss-Jordan         1.33 / 0.89       2.00 / 1.07            3.00 / 1.31
    Gauss-Jordan fall-back    5.23 / 1.78       2.52 / 1.04            2.24 / 1.42
    three passes              3.90 / 0.95       5.96 / 1.34            3.58 / 2.53
    two passes                3.85 / 1.07       4.98 / 1.11            4.69 / 2.13

The finding: without the max|X0| gate, d = 32 band C (scale 0.8, cond_1 3.4e4, max|inv| 669) measured
3.62 / 5.24 / 8.75 on its three-pass slots 3 / 4 / 5, and the steep cells 11.14 (d = 16, max|inv|
546), 13.28 (d = 32) and 8.05 (d = 64, 1213) on their worst slot, with forward ratios under 1.  The
series is one-sided: A Y - I is its own residual, Y A - I is the rounding of R amplified by
|inv(A)||A|.  small.hip now falls back to Gauss-Jordan when max|X0| > 512, and those cells' warm
slots measure <= 2.3.  The first gate tried, 128, made a default fit at d = 32 take 23 % longer
(2000 of its 40000 slots have max|inv| above 128); at 512 default fits at d = 20 / 32 / 48 / 64 take
the parent's time and give its W bit for bit.
Trajectories: W within 1.5e-16 of the oracle (bar 1e-9), h and the objective within 6.3e-14
relative (bar 1e-10).  Line search: 1 / 2 / 3 / 4 / 4 / 4 halvings at d = 7 / 16 / 20 / 32 / 48 / 64,
equal to the oracle's, W within 1.5e-13 (bar 1e-8).  The file runs in 3.5 s.

Mutations (scratch builds of small.hip, not committed), this file on each:
    `three` forced false       : the 8 dense cells of test_every_slot_inverse fail (every d)
    the 1e-2 gate raised to 1  : the 8 wide cells of test_every_slot_inverse fail (every d)
    the max|X0| gate removed   : the 3 steep cells and d = 32 band C fail (ratios above)
    `warm = 1` after ACT_HALVE removed : everything passes, and must: the slot after a halving
        starts from the inverse of an out-of-domain W and always falls back, whichever warm start
        it is offered (tests/test_small_cases_cpu.py::test_slots_after_a_halving_always_fall_back),
        so no output of the kernel depends on that line
Without the dense and wide bands the first two mutations left the file green: d max|R| bounds
||R||_inf but lies 10 - 100x above it on the make_W family, so the shorter form converges there too.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import blockinv_cases as bc  # noqa: E402
from tests.test_gpu_batch import _same  # noqa: E402
from tests.test_gpu_small import REC_FIELDS, _check_records  # noqa: E402

SEARCH_D = (7, 16, 20, 32, 48, 64)
DS_OF = {d: ds for ds, dd in bc.SMALL_DS.items() for d in dd}
FORM_NAME = {"2": "two passes", "3": "three passes", "G": "fall-back", "c": "cold Gauss-Jordan"}

_ORACLES = {}


def _oracle(d, checkpoint=None):
    """The shared covariance of a size (make_dataset(d, max(200, 10 d), seed=d)); never modified but
    for the checkpoint interval, which every caller of its minimize sets."""
    if d not in _ORACLES:
        _ORACLES[d] = bc.small_oracle(d)
    if checkpoint is not None:
        _ORACLES[d].checkpoint = checkpoint
    return _ORACLES[d]


def _solver(d):
    from midagma_amd.solver import HipSolver
    s = HipSolver(d, "l2", "cov", device=0)
    s.set_cov(_oracle(d).cov)
    return s


def _cell_id(d, band):
    return f"DS{DS_OF[d]}-d{d}-{band}"


CELLS = [pytest.param(d, band, id=_cell_id(d, band)) for d, band in bc.small_cells()]


# ------------------------------------------------------------------ a. every slot's inverse
@pytest.mark.parametrize("d,band", CELLS)
def test_every_slot_inverse(d, band):
    """begin at W0, 5 iterations of one run_slots(1) each: slot 1 is the cold Gauss-Jordan, slot 2
    warm-starts from P(1) alone, slots 3.. from 2 P(k-1) - P(k-2), in the form the CPU file pins.
    After each, the stored inverse against the W the slot started from."""
    W0, lr, forms = bc.small_cell(d, band)
    sol = _solver(d)
    try:
        sol.begin(W0, 1.0, 1000, 1.0, lr, tol=-1.0, checkpoint=1000)
        W_in = W0
        for it, form in zip(range(1, 6), "c" + forms):
            sol.run_slots(1)
            sol.sync()
            r = sol.poll()
            assert (r.iters, r.status, r.halvings) == (it, 0, 0), (it, r.iters, r.status, r.halvings)
            W_next, Mt = sol.debug_slot_matrices()
            res, fwd = bc.check_inverse(W_in, Mt, 1.0)
            print(f"SMALLINV DS{DS_OF[d]} d={d} {band} slot {it} ({FORM_NAME[form]}): residual ratio {res:.2f}, "
                  f"forward ratio {fwd:.2f}")
            W_in = W_next
    finally:
        sol.close()


def test_hook_needs_a_slot():
    """The read-back stays -1 (an error in Python) before the first slot of a call."""
    from midagma_amd import _lib
    d = 20
    sol = _solver(d)
    try:
        W0, lr, _ = bc.small_cell(d, "B")
        sol.begin(W0, 1.0, 1000, 1.0, lr, tol=-1.0)
        with pytest.raises(_lib.HipSolverError):
            sol.debug_slot_matrices()
        sol.run_slots(1)
        W1, Mt = sol.debug_slot_matrices()
        assert not np.array_equal(W1, W0)
        bc.check_inverse(W0, Mt, 1.0)
    finally:
        sol.close()


# ------------------------------------------------------------------ b. trajectory and records
def _check_h_obj(res, tr, label):
    worst = 0.0
    for c, r in zip(res.checkpoints, tr.records):
        eh = abs(c.h - r["reg_dag_value"]) / abs(r["reg_dag_value"])
        eo = abs(c.obj - r["obj_total"]) / abs(r["obj_total"])
        worst = max(worst, eh, eo)
        assert eh <= 1e-10, (c.iter, c.h, r["reg_dag_value"])
        assert eo <= 1e-10, (c.iter, c.obj, r["obj_total"])
    print(f"SMALLINV records {label}: h and obj within {worst:.1e} relative, h = {res.checkpoints[-1].h:.3g}")


@pytest.mark.parametrize("checkpoint", [3, 5])
@pytest.mark.parametrize("d,band", CELLS)
def test_trajectory_and_records(d, band, checkpoint):
    """12 steps against o.minimize from the same W0.  checkpoint = 3: records at 3, 6, 9, 12, a
    pivot-taking Gauss-Jordan slot after every third warm slot; checkpoint = 5: 5, 10 and the last
    record at the non-multiple 12.  W within 1e-9, all 13 record fields by test_gpu_small's rule,
    h (O(1) here) and the objective within 1e-10 relative."""
    W0, lr, _ = bc.small_cell(d, band)
    Wr, tr = _oracle(d, checkpoint).minimize(W0.copy(), 1.0, 12, 1.0, lr, tol=-1.0)
    sol = _solver(d)
    try:
        W = W0.copy()
        res = sol.minimize(W, 1.0, 12, 1.0, lr, tol=-1.0, checkpoint=checkpoint, want_checkpoints=True)
    finally:
        sol.close()
    assert res.success and res.iters == tr.iters == 12 and res.halvings == tr.halvings == 0
    dw = float(np.abs(W - Wr).max())
    print(f"SMALLINV trajectory {_cell_id(d, band)} checkpoint {checkpoint}: max|dW| {dw:.2e}")
    assert dw <= 1e-9
    assert [c.iter for c in res.checkpoints] == ([3, 6, 9, 12] if checkpoint == 3 else [5, 10, 12])
    _check_records(res, tr)
    _check_h_obj(res, tr, _cell_id(d, band))


# ------------------------------------------------------------------ c. launch boundaries
def _boundary_cases():
    for d, band in ((16, "far"), (5, "dense"), (20, "B"), (32, "dense"), (48, "far"), (64, "dense")):
        W0, lr, _ = bc.small_cell(d, band)
        yield pytest.param(d, W0, lr, id=_cell_id(d, band))
    for d in (16, 20, 64):
        yield pytest.param(d, bc.make_W(d, bc.SMALL_SEARCH[0], d), bc.SMALL_SEARCH[1], id=f"d{d}-search")


@pytest.mark.parametrize("d,W0,lr", list(_boundary_cases()))
def test_launch_boundaries_bit_identical(d, W0, lr):
    """One run_slots(1) per slot against a single minimize call of the same 12 steps (checkpoint 3):
    the last two inverses and the warm count cross every launch boundary at inverses that are not
    ≈ I, and the product-form slots of the band cells consume them.  In the search cases they cross
    too, but every warm slot there falls back (the CPU file's
    test_slots_after_a_halving_always_fall_back says why), so those cases cover the controller's
    state, the pending norms and the halving itself across launches, not the stored inverses.
    W and every record field bit-identical."""
    a = _solver(d)
    b = _solver(d)
    try:
        Wa = W0.copy()
        ra = a.minimize(Wa, 1.0, 12, 1.0, lr, tol=-1.0, checkpoint=3, want_checkpoints=True)
        b.begin(W0, 1.0, 12, 1.0, lr, tol=-1.0, checkpoint=3)
        for _ in range(ra.slots + 2):
            b.run_slots(1)
        Wb = np.zeros((d, d))
        rb = b.end(Wb)
        cb = b.checkpoints()
    finally:
        a.close()
        b.close()
    assert (rb.iters, rb.slots, rb.status, rb.halvings, rb.lr_final) == \
        (ra.iters, ra.slots, ra.status, ra.halvings, ra.lr_final)
    assert ra.iters == 12 and np.array_equal(Wa, Wb)
    assert [c.iter for c in cb] == [c.iter for c in ra.checkpoints] == [3, 6, 9, 12]
    for x, y in zip(ra.checkpoints, cb):
        for f in REC_FIELDS:
            assert getattr(x, f) == getattr(y, f), (x.iter, f)


# ------------------------------------------------------------------ d. line search at every DS
@pytest.mark.parametrize("d", SEARCH_D)
def test_line_search_halvings(d):
    """scale 0.8 at lr 0.3: the oracle halves lr 1 .. 4 times within 12 steps (pinned on the CPU);
    ACT_HALVE in both code forms (DS <= 32 and DS = 64).  The slot after a halving starts from the
    inverse of the out-of-domain W and always falls back to Gauss-Jordan (g >= 5, CPU file)."""
    scale, lr = bc.SMALL_SEARCH
    Wr, tr = _oracle(d, 1000).minimize(bc.make_W(d, scale, d), 1.0, 12, 1.0, lr, tol=-1.0)
    assert tr.halvings == bc.SMALL_SEARCH_HALVINGS[d]
    sol = _solver(d)
    try:
        W = bc.make_W(d, scale, d)
        res = sol.minimize(W, 1.0, 12, 1.0, lr, tol=-1.0, checkpoint=1000)
    finally:
        sol.close()
    dw = float(np.abs(W - Wr).max())
    print(f"SMALLINV search d={d}: halvings {res.halvings} (oracle {tr.halvings}), lr {res.lr_final}, max|dW| {dw:.2e}")
    assert (res.iters, res.success, res.halvings, res.lr_final) == (tr.iters, tr.success, tr.halvings, tr.lr_final)
    assert dw <= 1e-8


@pytest.mark.parametrize("d", SEARCH_D)
def test_out_of_domain_failure(d):
    """The same start at s = 0.9: out of domain on the first step that tests it (iteration 0 at
    d = 32, 1 elsewhere), no halving below s = 1 (linear.py:230-232)."""
    scale, lr = bc.SMALL_SEARCH
    Wr, tr = _oracle(d, 1000).minimize(bc.make_W(d, scale, d), 1.0, 12, 0.9, lr, tol=-1.0)
    assert not tr.success and tr.iters == (0 if d == 32 else 1)
    sol = _solver(d)
    try:
        W = bc.make_W(d, scale, d)
        res = sol.minimize(W, 1.0, 12, 0.9, lr, tol=-1.0, checkpoint=1000)
    finally:
        sol.close()
    assert res.success is False and res.iters == tr.iters and res.halvings == 0
    assert np.abs(W - Wr).max() <= 1e-9


# ------------------------------------------------------------------ e. the batch away from W = 0
@pytest.mark.parametrize("d", [16, 20, 48])
def test_batch_bit_identical_at_ill_conditioned_starts(d):
    """HipBatch(d, 4): scales 0.3 / 0.6 / 0.8 at lr 3e-4 and the search-band problem (lr 0.3), so
    the problems take different inverse forms, and the fourth halves, on the same slot: per-problem
    offsets of the stored inverses and carry words.  Each bit-identical to the single solver."""
    from midagma_amd.solver import HipBatch
    o = _oracle(d, 3)
    W0 = np.stack([bc.make_W(d, sc, d) for sc in (0.3, 0.6, 0.8, bc.SMALL_SEARCH[0])])
    lrs, ss = [3e-4, 3e-4, 3e-4, bc.SMALL_SEARCH[1]], [1.0, 1.0, 1.0, 1.0]
    bt = HipBatch(d, 4, device=0)
    try:
        bt.set_cov(np.stack([o.cov] * 4))
        W = W0.copy()
        res = bt.minimize(W, 1.0, ss, lrs, 0.03, 12, tol=-1.0, checkpoint=3, want_checkpoints=True)
    finally:
        bt.close()
    for b in range(4):
        sol = _solver(d)
        try:
            Ws = W0[b].copy()
            ref = sol.minimize(Ws, 1.0, 12, ss[b], lrs[b], tol=-1.0, lambda1=0.03, checkpoint=3, want_checkpoints=True)
        finally:
            sol.close()
        assert np.array_equal(W[b], Ws), b
        _same(res[b], ref)
    assert res[3].halvings == bc.SMALL_SEARCH_HALVINGS[d] and res[0].halvings == 0
    Wr, tr = o.minimize(W0[1].copy(), 1.0, 12, 1.0, lrs[1], tol=-1.0)
    assert tr.iters == res[1].iters == 12 and np.abs(W[1] - Wr).max() <= 1e-9
    _check_records(res[1], tr)
