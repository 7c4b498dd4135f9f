"""The two-level blocked inverse (blockinv.hip, binv_tile.h, nm16.h, nm_series.h, the gemm_trail* /
trail128* kernels of gemm.hip) at ill-conditioned W, one case per dispatch cell.

The solver's other tests reach this path only through trajectories from W = 0, where
A = sI - W∘W ≈ I and W barely depends on the inverse.  Here W0 comes from tests/blockinv_cases.py
(rho(W∘W) 0.2 / 0.6 / 0.9, cond_1 up to 6e4) and every slot's Mt is read back with the read-only hook
midagma_debug_slot_matrices and checked against LAPACK by blockinv_cases.check_inverse: two-sided
residual <= 8x LAPACK's at every d, forward error <= 8x LAPACK's against a longdouble-refined
inverse at d <= 300.

The cells (cov mode; read off midagma_create's padding, binv_block, TRAIL128_MIN = 1792 for D - B2,
trail_series_workers and alloc_core's cov_split / at_fold rules):

    d     D     B2   K2  trailing update and what else is particular
    100   128   128  1   none (one block: the series / the pivoted block is the whole inverse)
    130   256   256  1   none; 126 padded rows
    300   512   256  2   32-tile, split-K 4 score GEMM and control folded into the last one
    600   768   256  3   32-tile + fold; odd K2: the ping-pong starts in Malt
    800   896   128  7   32-tile + fold at B2 = 128
    1000  1024  256  4   32-tile + fold; outer step 0 reads A0 (build_at folded into the update)
    1800  1920  128  15  128-tile (EPI_SUB_BAND), score GEMM apart (split 1)
    2000  2048  256  8   128-tile (EPI_SUB_MID), score GEMM apart (split 1)
    4300  4352  256  17  128-tile with the next block's series inside the trailing launch
    data mode d = 300 -> D = 384, B2 = 128, K2 = 3: n = 2000 fast slots forked on the side stream,
    n = 20000 (> 16384 rows) the pivoted blocked inverse forked on every slot

run_slots(n) counts launched slots, so a fast slot that hands back (ST_NEED_GJ) uses one up without
advancing `iters`; _iteration() below then launches the pivoted re-run itself, once, and asserts
that the pair advanced `iters` by exactly one and the hand-back counter by one.

Largest ratios measured on an MI355X (residual / forward, of the bar 8), per cell over its bands
and slots, and the hand-backs of the slot test's warm slots ("-": d > 300, no forward check):

    cell                      fast bands          near band (lr 1e-7)
    d100  (D128)              1.64 / 1.79, 1      1.42 / 0.79, 0
    d130  (D256)              1.93 / 2.59, 1
    d300  (D512)              3.38 / 2.64, 1      1.88 / 1.30, 0
    d600  (D768)              1.26 / -,    1
    d800  (D896)              1.32 / -,    1      1.22 / -,    0
    d1000 (D1024)             1.29 / -,    1      1.07 / -,    0
    d1800 (D1920)             1.12 / -,    1
    d2000 (D2048)             1.25 / -,    1
    d4300 (D4352)             1.69 / -,    1
    data d300 n=2000          1.57 / 2.63, 1
    data d300 n=20000         2.43 / 2.17, 0
    far d300 / d1000          1.49 / 2.27 and 1.64 / -; slots 2, 3 and 4 hand back
    spoiled d800              1.24 / -; iterations 2, 4 and 5 hand back
    flat entries, d <= 200    2.65 / 0.87; log-det 1.5e-14 relative

The one hand-back of every fast-band case is slot 2's (see test_slow_and_fast_slots).  The 3.38 is
slot 3 at d = 300, scale 0.8 (the first extrapolated 3-pass slot); every other slot is under 2.7.
Log-det test: h within 4.4e-13 relative (bar 1e-10), objectives 2.5e-16, W 6.1e-15.  Line search:
2 / 4 / 4 / 5 / 6 halvings at d = 100 / 300 / 800 / 1000 / 2000, equal to the oracle's, W within
6.7e-12 (bar 1e-8).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import blockinv_cases as bc  # noqa: E402

# d -> the cell's id in the parametrized names; PADDED: the D each solver must report
CELLS = {
    100: "d100-D128-B128x1",
    130: "d130-D256-B256x1-pad126",
    300: "d300-D512-B256x2-trail32fold",
    600: "d600-D768-B256x3-oddpingpong",
    800: "d800-D896-B128x7-trail32fold",
    1000: "d1000-D1024-B256x4-trail32fold-A0",
    1800: "d1800-D1920-B128x15-trail128band",
    2000: "d2000-D2048-B256x8-trail128mid",
    4300: "d4300-D4352-B256x17-trail128series",
}
PADDED = {100: 128, 130: 256, 300: 512, 600: 768, 800: 896, 1000: 1024, 1800: 1920, 2000: 2048, 4300: 4352}


@pytest.fixture(scope="module")
def hip():
    from midagma_amd import _lib
    from midagma_amd.solver import device_count
    _lib.load()
    assert device_count() >= 1, "no ROCm device visible"
    return _lib


_ORACLES = {}


def _oracle(d, n=None):
    """The shared covariance of a cell (make_dataset(d, 2d, seed=d)); never modified but for the
    checkpoint interval, which every user sets."""
    key = (d, n)
    if key not in _ORACLES:
        _ORACLES[key] = bc.make_oracle(d, n=n)
    return _ORACLES[key]


def _cov_solver(hip, d):
    from midagma_amd.solver import HipSolver
    s = HipSolver(d, "l2", "cov", device=0)
    assert hip.lib().midagma_padded_dim(s.h) == PADDED[d]
    s.set_cov(_oracle(d).cov)
    return s


def _iteration(sol, it):
    """One iteration through run_slots(1).  Returns whether its fast slot handed back (then re-run
    pivoted by a second run_slots(1)); asserts iters == it and the hand-back counter's step."""
    hb0 = sol.debug_handbacks()
    sol.run_slots(1)
    sol.sync()
    r = sol.poll()
    handed = r.iters == it - 1 and r.status == 0
    if handed:  # the slot was launched, handed back and applied nothing: its pivoted re-run
        sol.run_slots(1)
        sol.sync()
        r = sol.poll()
    assert r.iters == it and r.status == 0, (it, r.iters, r.status)
    assert sol.debug_handbacks() - hb0 == (1 if handed else 0)
    return handed, r


def _run_checked_slots(sol, W0, lr, n_iter, label, forward=None, before=None):
    """begin at W0, n_iter iterations; every slot's Mt against the W it started from.  `before`
    (it -> None) runs ahead of an iteration.  Returns (max residual ratio, max forward ratio or
    None, the iterations that handed back)."""
    sol.begin(W0, 1.0, 1000, 1.0, lr, tol=-1.0, checkpoint=1000)
    W_in, res_max, fwd_max, handed_at = W0, 0.0, None, []
    for it in range(1, n_iter + 1):
        if before is not None:
            before(it)
        handed, r = _iteration(sol, it)
        if handed:
            handed_at.append(it)
        assert r.halvings == 0
        W_next, Mt = sol.debug_slot_matrices()
        res, fwd = bc.check_inverse(W_in, Mt, 1.0, forward=forward)
        print(f"BLOCKINV {label} slot {it}{' (handed back, pivoted)' if handed else ''}: residual ratio "
              f"{res:.2f}" + (f", forward ratio {fwd:.2f}" if fwd is not None else ""))
        res_max = max(res_max, res)
        if fwd is not None:
            fwd_max = fwd if fwd_max is None else max(fwd_max, fwd)
        W_in = W_next
    return res_max, fwd_max, handed_at


def _slot_cases():
    for d, cid in CELLS.items():
        for scale, lr in bc.FAST_BANDS:
            if d >= 1800 and scale != 0.6:
                continue
            yield pytest.param(d, scale, lr, id=f"{cid}-scale{scale}")


# ------------------------------------------------------------------ a. slow and fast slots
@pytest.mark.parametrize("d,scale,lr", list(_slot_cases()))
def test_slow_and_fast_slots(hip, d, scale, lr):
    """Slot 1 is the pivoted blocked inverse of W0; slots 2.. are warm starts (slot 2 from P(k-1)
    alone, 3.. from the extrapolation 2 P(k-1) - P(k-2), in both store parities).  The bands' whole
    warm-start residuals are <= 0.05 (first) and 2e-3 (extrapolated), far under the 0.25 gate, so at
    most one hand-back is legitimate over the warm slots: slot 2's, whose two passes cannot finish
    from a residual over 1e-4 (blockinv_cases.NEAR_BAND); it is re-run pivoted and the slots after
    it run three passes from the extrapolation (measured: exactly that in every cell and band).
    d >= 1800: band 0.6, three slots; d = 4300 checks the residual only (as every d > 300)."""
    sol = _cov_solver(hip, d)
    try:
        n_iter = 3 if d >= 1800 else 5
        res, fwd, handed = _run_checked_slots(sol, bc.make_W(d, scale, d), lr, n_iter, f"{CELLS[d]} scale {scale}")
        print(f"BLOCKINV-MAX slots {CELLS[d]} scale {scale}: residual {res:.2f} forward "
              f"{'-' if fwd is None else format(fwd, '.2f')} handbacks {len(handed)}")
        assert len(handed) <= 1 and sol.debug_handbacks() <= 1, handed
    finally:
        sol.close()


@pytest.mark.parametrize("d", [pytest.param(d, id=CELLS[d]) for d in (100, 300, 800, 1000)])
def test_two_pass_slots_from_a_near_warm_start(hip, d):
    """lr = 1e-7 at scale 0.6: the first warm slot's residual is <= 2.5e-5, so slot 2 converges in
    the two passes every call starts with, from P(k-1) alone, and no slot hands back: the 2-pass
    graphs' panels and trailing updates at an ill-conditioned A, which the bands above never reach
    (their slot 2 hands back and holds the scheduler at three passes)."""
    scale, lr = bc.NEAR_BAND
    sol = _cov_solver(hip, d)
    try:
        res, fwd, handed = _run_checked_slots(sol, bc.make_W(d, scale, d), lr, 4, f"near {CELLS[d]}")
        print(f"BLOCKINV-MAX near {CELLS[d]}: residual {res:.2f} forward "
              f"{'-' if fwd is None else format(fwd, '.2f')} handbacks {len(handed)}")
        assert handed == [] and sol.debug_handbacks() == 0
    finally:
        sol.close()


@pytest.mark.parametrize("n,forked", [(2000, "fast-forked"), (20000, "pivoted-forked")])
@pytest.mark.parametrize("scale,lr", bc.FAST_BANDS[1:])
def test_data_mode_slots(hip, n, forked, scale, lr):
    """Data mode, d = 300 -> D = 384 (B2 = 128, K2 = 3, a cell cov mode never pads to): the same
    five slots with the inverse forked beside the n x d GEMMs: warm-started fast slots at n = 2000,
    the pivoted blocked inverse on every slot at n = 20000 (no warm start, so no hand-back)."""
    from midagma_amd.solver import HipSolver
    d = 300
    o = _oracle(d, n)
    sol = HipSolver(d, "l2", "data", device=0)
    try:
        assert hip.lib().midagma_padded_dim(sol.h) == 384
        sol.set_data(o.X, n_global=n)
        res, fwd, handed = _run_checked_slots(sol, bc.make_W(d, scale, d), lr, 5, f"data n={n} scale {scale}")
        print(f"BLOCKINV-MAX data n={n} ({forked}) scale {scale}: residual {res:.2f} forward {fwd:.2f} "
              f"handbacks {len(handed)}")
        assert len(handed) <= (1 if n == 2000 else 0)
    finally:
        sol.close()


# ------------------------------------------------------------------ b. far warm start
@pytest.mark.parametrize("d", [300, 1000])
def test_far_warm_start_hands_back(hip, d):
    """scale 0.8 at lr 3e-4: ||I - A(W1) M(W0)||_inf is 1.77 (d = 300) and 1.80 (d = 1000), over the
    0.25 gate, so slot 2 must hand back and be re-run pivoted; every slot's Mt still passes.
    (Measured: slots 3 and 4 hand back too; W moves as far again, so the extrapolated start is no
    nearer.)"""
    scale, lr = bc.FAR_BAND
    sol = _cov_solver(hip, d)
    try:
        res, fwd, handed = _run_checked_slots(sol, bc.make_W(d, scale, d), lr, 4, f"far {CELLS[d]}")
        print(f"BLOCKINV-MAX far {CELLS[d]}: residual {res:.2f} forward "
              f"{'-' if fwd is None else format(fwd, '.2f')} handed back at {handed}")
        assert 2 in handed and sol.debug_handbacks() >= 1
    finally:
        sol.close()


def test_spoiled_warm_start_hands_back(hip):
    """d = 800 (B2 = 128): the stored warm starts zeroed before iteration 4, whose fast slot then
    starts from 0 (residual I) and must hand back; its pivoted re-run and the slots after it pass.
    (Iteration 5 hands back as well: its extrapolation 2 P(4) - P(3) reads the zeroed P(3).)"""
    d = 800
    scale, lr = bc.FAST_BANDS[1]
    sol = _cov_solver(hip, d)
    try:
        res, _, handed = _run_checked_slots(sol, bc.make_W(d, scale, d), lr, 5, f"spoil {CELLS[d]}",
                                            before=lambda it: sol.debug_spoil_warm() if it == 4 else None)
        print(f"BLOCKINV-MAX spoil {CELLS[d]}: residual {res:.2f} handed back at {handed}")
        assert 4 in handed
    finally:
        sol.close()


# ------------------------------------------------------------------ c. log-det from the blocked pivots
@pytest.mark.parametrize("d", [pytest.param(d, id=cid) for d, cid in CELLS.items() if d <= 2000])
def test_logdet_from_blocked_pivots(hip, d):
    """checkpoint = 1: every slot is pivoted and its log-det comes from the blocked path's pivots.
    Three steps from the scale-0.8 W0 (h is O(1) and more, so the relative bars bite) against the
    oracle: iterations, W, and every checkpoint's objective and h."""
    scale, lr = 0.8, 3e-6
    o = _oracle(d)
    o.checkpoint = 1
    sol = _cov_solver(hip, d)
    try:
        W = bc.make_W(d, scale, d)
        res = sol.minimize(W, 1.0, 3, 1.0, lr, tol=-1.0, checkpoint=1, want_checkpoints=True)
    finally:
        sol.close()
    Wr, tr = o.minimize(bc.make_W(d, scale, d), 1.0, 3, 1.0, lr, tol=-1.0)
    assert res.iters == tr.iters == 3 and res.success
    dw = float(np.abs(W - Wr).max())
    assert len(res.checkpoints) == len(tr.checkpoints) == 3
    for c, (it, obj_r, _, h_r) in zip(res.checkpoints, tr.checkpoints):
        print(f"BLOCKINV logdet {CELLS[d]} it {it}: h {c[3]:.12g} (oracle {h_r:.12g}, rel "
              f"{abs(c[3] - h_r) / max(1.0, abs(h_r)):.1e}), obj rel {abs(c[1] - obj_r) / abs(obj_r):.1e}")
    print(f"BLOCKINV logdet {CELLS[d]}: max|dW| {dw:.2e}")
    assert dw <= 1e-9
    for c, (it, obj_r, _, h_r) in zip(res.checkpoints, tr.checkpoints):
        assert c[0] == it
        assert abs(c[1] - obj_r) <= 1e-10 * abs(obj_r)
        assert abs(c[3] - h_r) <= 1e-10 * max(1.0, abs(h_r))


# ------------------------------------------------------------------ d. domain flags per cell
@pytest.mark.parametrize("d", [pytest.param(d, id=CELLS[d]) for d in (100, 300, 800, 1000, 2000)])
def test_domain_flags_line_search(hip, d):
    """scale 0.8 at lr 3e-2: the oracle's domain line search (an entry of M < 0) halves lr within 12
    steps (2, 4, 5 times at d = 100, 300, 1000); the fast slots must raise the same flags from
    their last outer step's outputs, in every cell."""
    scale, lr = bc.SEARCH_BAND
    o = _oracle(d)
    o.checkpoint = 1000
    Wr, tr = o.minimize(bc.make_W(d, scale, d), 1.0, 12, 1.0, lr, tol=-1.0)
    assert tr.halvings >= 1, "the case no longer exercises the domain flag"
    sol = _cov_solver(hip, d)
    try:
        W = bc.make_W(d, scale, d)
        res = sol.minimize(W, 1.0, 12, 1.0, lr, tol=-1.0, checkpoint=1000)
    finally:
        sol.close()
    dw = float(np.abs(W - Wr).max())
    print(f"BLOCKINV flags {CELLS[d]}: halvings {res.halvings} (oracle {tr.halvings}), lr {res.lr_final}, "
          f"max|dW| {dw:.2e}")
    assert (res.iters, res.success, res.halvings, res.lr_final) == (tr.iters, tr.success, tr.halvings, tr.lr_final)
    assert dw <= 1e-8


# ------------------------------------------------------------------ e. the flat Gauss-Jordan entries
@pytest.mark.parametrize("scale", [0.6, 0.8])
@pytest.mark.parametrize("d", [20, 33, 64, 65, 200])
@pytest.mark.parametrize("entry", ["logdet_inv_dev", "logdet_h_dev"])
def test_flat_gauss_jordan_entries(hip, entry, d, scale):
    """midagma_logdet_inv_dev / midagma_logdet_h_dev on torch device tensors, A = W∘W of the same
    family, with leading dimensions that differ from d (lda = d + 3, ldm = d + 5): Mt by
    check_inverse, the log-det against slogdet."""
    W = bc.make_W(d, scale, d)
    lda, ldm = d + 3, d + 5
    dev = torch.device("cuda", 0)
    Ah = np.full((d, lda), np.nan)
    Ah[:, :d] = W * W
    A = torch.from_numpy(Ah).to(dev)
    Mt = torch.full((d, ldm), float("nan"), dtype=torch.float64, device=dev)
    out = torch.zeros(1, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    fn = getattr(hip.lib(), "midagma_" + entry)
    with torch.cuda.device(dev):
        hip.check(fn(C.c_void_p(A.data_ptr()), d, lda, 1.0, C.c_void_p(out.data_ptr()), C.c_void_p(Mt.data_ptr()),
                     ldm, C.c_void_p(stream) if stream else None), None, entry)
    torch.cuda.synchronize(dev)
    Mh = Mt.cpu().numpy()
    assert np.isnan(Mh[:, d:]).all(), "wrote past column d of Mt"
    res, fwd = bc.check_inverse(W, np.ascontiguousarray(Mh[:, :d]), 1.0)
    logdet = np.linalg.slogdet(bc.a_matrix(W))[1]
    ref = logdet if entry == "logdet_inv_dev" else -logdet  # h = -log det(sI - A) + d log s, s = 1
    got = float(out.item())
    print(f"BLOCKINV flat {entry} d={d} scale {scale}: residual ratio {res:.2f}, forward ratio {fwd:.2f}, "
          f"log-det rel {abs(got - ref) / max(1.0, abs(ref)):.1e}")
    assert abs(got - ref) <= 1e-10 * max(1.0, abs(ref))
