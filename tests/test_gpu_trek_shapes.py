"""csrc/trek.hip at every shape branch, squaring count and pair-list edge (HipSolver.trek_value
and the minimize loop), against the long-double restatement tests/trek_numpy.py for d <= 65 and
the float64 oracle above that, at norms where tests/test_trek_numpy_cpu.py certifies the oracle.

  shape cells     padded D and gemm_dd's split (1 / 2 / 3 / 4 / none at 256 tiles), d == D and
                  mostly padding, cov and data mode, log at its default K = 2d, binom at all-bits
                  and single-bit powers; the aggregators rotate over the cells
  squaring counts exp at both edges of the buckets s = 0, 1, 2, 4, 6, 9 and at s = TREK_SMAX; the
                  test computes s by the kernel's rule and asserts the count it means to reach
  one handle      s = 12, 0, 6, 0 on one handle, bit-equal to fresh handles ('opt' and 'log')
  pair lists      m = 1, mirrored pairs, a diagonal pair, 70 001 entries with heavy duplicates,
                  exact ties under max, all 89 700 ordered pairs at d = 300
  in the loop     inv and checkpoint-only log at a blocked D, data mode

Bars (those of test_gpu_trek.py): D <= 128 value 1e-11 max(1, |v|), gradient 1e-10 max(1, max|g|);
D > 128 value 1e-10 |v|, gradient 1e-9 max|g|.  At s >= 6 the bar is max(that, 4 x the oracle's own
deviation from long double on the same case): both are float64 scaling-and-squaring whose error
grows like 2^s ("PST regularizer", has the measured maxima).
Every cell prints its deviation (and its s): run with -s.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from midagma_amd.simulate import make_dataset  # noqa: E402
from oracle.dagma_oracle import LinearOracle  # noqa: E402
from oracle.trek_oracle import pst_value_grad  # noqa: E402
from tests import trek_numpy as tn  # noqa: E402

LD = np.longdouble


@pytest.fixture(scope="module")
def hip():
    from midagma_amd import _lib
    _lib.load()
    return _lib


def _solver(d, mode="cov"):
    from midagma_amd.solver import HipSolver
    s = HipSolver(d, "l2", mode, device=0)
    if mode == "cov":
        s.set_cov(np.eye(d))
    else:   # any small X: the regularizer does not read it
        X = np.random.default_rng(d).standard_normal((256, d))
        s.set_data(X - X.mean(axis=0, keepdims=True), n_global=256)
    return s


def _gpu(d, W, pairs, seq, agg, K_log=None, mode="cov", run="opt"):
    s = _solver(d, mode)
    s.set_trek(pairs, seq, agg=agg, mode=run, weight=0.5, K_log=K_log)
    v, g = s.trek_value(W)
    D = s.D
    s.close()
    return v, g, D


def _deviation(v, g, v_ref, g_ref, D):
    """(value deviation, gradient deviation), each divided by what its bar is relative to."""
    v_ref, g_ref = LD(v_ref), np.asarray(g_ref, dtype=LD)
    if D <= 128:
        sv, sg = max(LD(1.0), abs(v_ref)), max(LD(1.0), np.abs(g_ref).max())
    else:
        sv, sg = abs(v_ref), np.abs(g_ref).max()
    return float(abs(LD(v) - v_ref) / sv), float(np.abs(np.asarray(g, dtype=LD) - g_ref).max() / sg)


def _bars(D):
    return (1e-11, 1e-10) if D <= 128 else (1e-10, 1e-9)


def _reference(key, d, W, pairs, seq, agg, K_log):
    if d <= tn.LD_MAX_D:
        return tn.reference_ld(key, W, pairs, seq, agg, K_log)
    return pst_value_grad(W, pairs, seq, K_log=K_log, agg=agg)


# ---- a. shape cells ------------------------------------------------------------------------------

@pytest.mark.parametrize("cell,seq", [(i, seq) for i, c in enumerate(tn.SHAPE_CELLS) for seq in c[3]],
                         ids=lambda x: x if isinstance(x, str) else f"d{tn.SHAPE_CELLS[x][1]}{tn.SHAPE_CELLS[x][0]}")
def test_shape_cell(hip, cell, seq):
    mode, d, D_expect, _ = tn.SHAPE_CELLS[cell]
    agg, K = tn.shape_cell_agg(cell, seq), tn.shape_cell_klog(d, seq)
    W, pairs = tn.shape_case(d, seq)
    nrm = tn.norm1_w2(W)
    assert nrm <= 4 and (seq != "binom" or (d * nrm <= 8 * (1 + 1e-12) and d <= 300))
    s_count = tn.squaring_count(W)
    assert seq != "exp" or s_count == 4
    v, g, D = _gpu(d, W, pairs, seq, agg, K, mode)
    assert D == D_expect
    v_ref, g_ref = _reference(("shape", d, seq), d, W, pairs, seq, agg, K)
    dv, dg = _deviation(v, g, v_ref, g_ref, D)
    print(f"\n{mode} d={d} D={D} {seq} {agg} K_log={K} m={len(pairs)} s={s_count if seq == 'exp' else '-'}: "
          f"value {dv:.2e} gradient {dg:.2e}")
    bv, bg = _bars(D)
    assert dv <= bv and dg <= bg


# ---- b. squaring counts --------------------------------------------------------------------------

@pytest.mark.parametrize("agg", ["mean", "max", "lse"])
@pytest.mark.parametrize("s_want,edge,norm", tn.bucket_norms(), ids=lambda x: x if isinstance(x, str) else f"{x:g}")
@pytest.mark.parametrize("d", [20, 65])
def test_squaring_count(hip, d, s_want, edge, norm, agg):
    """exp, 'opt', at both edges of each squaring bucket.  The upper edge (||X||_1 = 0.2475 after
    scaling) is where the degree-12 Taylor polynomial has the least room; the high counts walk the
    E[t] chain and the dQ[t & 1] ping-pong to their ends."""
    W, pairs = tn.squaring_case(d, norm)
    assert tn.squaring_count(W) == s_want
    v, g, D = _gpu(d, W, pairs, "exp", agg)
    v_ref, g_ref = tn.reference_ld(("sq", d, norm, agg), W, pairs, "exp", agg)
    assert np.isfinite(v) and np.isfinite(g).all()
    dv, dg = _deviation(v, g, v_ref, g_ref, D)
    bv, bg = _bars(D)
    line = f"\nexp d={d} D={D} s={s_want} {edge} ||W2||_1={norm:.4f} {agg}: value {dv:.2e} gradient {dg:.2e}"
    if s_want >= 6:
        ov, og = _deviation(*pst_value_grad(W, pairs, "exp", agg=agg), v_ref, g_ref, D)
        line += f" (oracle: value {ov:.2e} gradient {og:.2e})"
        bv, bg = max(bv, 4 * ov), max(bg, 4 * og)
    print(line)
    assert dv <= bv and dg <= bg


@pytest.mark.parametrize("d", [20, 65])
def test_squaring_threshold_value(hip, d):
    """||W o W||_1 = 0.25 exactly: s = 0 or 1 are both legitimate, so the value alone is checked."""
    W, pairs = tn.threshold_case(d)
    v, g, D = _gpu(d, W, pairs, "exp", "sum")
    v_ref, g_ref = tn.reference_ld(("thr", d), W, pairs, "exp", "sum")
    dv, dg = _deviation(v, g, v_ref, g_ref, D)
    print(f"\nexp d={d} threshold: value {dv:.2e} (gradient {dg:.2e}, not asserted)")
    assert dv <= _bars(D)[0]


# ---- c. one handle, many calls -------------------------------------------------------------------

@pytest.mark.parametrize("d", [20, 129])
def test_one_handle_many_squaring_counts(hip, d):
    """s = 12, 0, 6, 0 on one handle: the gate words, E[], dQ[] and scal left by a call must not
    reach the next.  Bit-equal to a fresh handle: the pair list has no duplicates and no mirrored
    pairs, so every entry of S receives one add, and the split-K slices are summed in fixed order."""
    cases = []
    for s_want, norm in ((12, 517.12), (0, 0.2), (6, 12.0), (0, 0.2)):
        W, pairs = tn.squaring_case(d, norm)
        assert tn.squaring_count(W) == s_want
        cases.append(W)
    fresh = [_gpu(d, W, pairs, "exp", "mean")[:2] for W in cases]
    assert all(np.isfinite(v) and np.abs(g).max() > 0 for v, g in fresh)
    one = _solver(d)
    one.set_trek(pairs, "exp", agg="mean", mode="opt", weight=0.5)
    for W, (v0, g0) in zip(cases, fresh):
        v, g = one.trek_value(W)
        assert v == v0 and np.array_equal(g, g0)
    one.set_trek(pairs, "exp", agg="mean", mode="log", weight=0.5)
    for W, (v0, _) in zip(cases, fresh):
        v, g = one.trek_value(W)
        assert v == v0 and not g.any()
    one.close()


# ---- d. pair lists -------------------------------------------------------------------------------

_PAIRLISTS = tn.pairlist_cases()


@pytest.mark.parametrize("name,agg", [(n, a) for n, c in _PAIRLISTS.items() for a in c[3]])
def test_pair_list(hip, name, agg):
    """d = 20 against long double.  'tiled' runs the grid-stride loops of the 256 x 256-thread pair
    kernels more than once and sends ~1000 atomic adds to each S entry; under max its duplicates
    are ties, so the 1 / ties share is what keeps the gradient from being ~1000 times too large.
    'ties-*': exact zeros below one positive maximum take no share; 'allzero-*': every pair ties
    at 0 (the gradient is 0 by the structure: an edge that would join a pair is absent);
    'dyadic-*': two edges tie at a positive maximum and halve a non-zero gradient."""
    d = 20
    W, pairs, seq, _ = _PAIRLISTS[name]
    K = 7 if seq == "log" else None
    v, g, D = _gpu(d, W, pairs, seq, agg, K)
    v_ref, g_ref = tn.reference_ld(("pl", name, agg), W, pairs, seq, agg, K)
    dv, dg = _deviation(v, g, v_ref, g_ref, D)
    s_count = tn.squaring_count(W) if seq == "exp" else "-"
    print(f"\npair list {name} {seq} {agg} m={len(pairs)} s={s_count}: value {dv:.2e} gradient {dg:.2e}")
    bv, bg = _bars(D)
    assert dv <= bv and dg <= bg
    if name.startswith(("allzero-", "dyadic-")) and agg == "max":
        assert v == float(v_ref)                       # exact by construction


@pytest.mark.parametrize("agg", ["mean", "lse"])
def test_all_ordered_pairs_d300(hip, agg):
    d = 300
    W = tn.sparse_w(d, 3.0, seed=5)
    pairs = tn.ordered_pairs(d)
    assert len(pairs) == 89700
    v, g, D = _gpu(d, W, pairs, "exp", agg)
    dv, dg = _deviation(v, g, *pst_value_grad(W, pairs, "exp", agg=agg), D)
    print(f"\nall ordered pairs d=300 D={D} exp {agg} s={tn.squaring_count(W)}: value {dv:.2e} gradient {dg:.2e}")
    assert dv <= 1e-10 and dg <= 1e-9


def test_trek_value_rejects_nonfinite_w(hip):
    W, pairs = tn.squaring_case(20, 1.0)
    s = _solver(20)
    s.set_trek(pairs, "exp", agg="mean", mode="opt", weight=0.5)
    W[2, 5] = np.nan
    with pytest.raises(ValueError):
        s.trek_value(W)
    s.close()


# ---- e. in the loop ------------------------------------------------------------------------------

@pytest.mark.parametrize("smode,d,n,seq,mode,K", [("cov", 300, 600, "inv", "opt", 50), ("cov", 300, 600, "exp", "log", 50),
                                                  ("data", 150, 400, "exp", "opt", 40),
                                                  ("data", 20, 1000, "inv", "opt", 90)])
def test_minimize_with_trek_shapes(hip, smode, d, n, seq, mode, K):
    """The harness and bars of test_gpu_trek.py::test_minimize_with_trek_matches_oracle.  cov d=300
    (D = 512, blocked): inv borrows the blocked inverse's Gauss-Jordan side panels; 'log' runs the
    regularizer on checkpoint slots only (checkpoint 20), between fast slots.  Data mode (the
    inverse forked on the side stream) against the cov-mode oracle, as tests/test_gpu_edges.py."""
    from midagma_amd.solver import HipSolver
    X, _, _ = make_dataset(d, n, seed=5)
    rng = np.random.default_rng(5)
    iu = np.array(np.triu_indices(d, 1)).T
    pairs = iu[rng.uniform(size=len(iu)) < 0.3]
    ckpt = 20 if mode == "log" else 40
    o = LinearOracle("l2")
    o.prepare(X, 0.03, ckpt)                      # centres X in place
    o.trek = dict(pairs=pairs, seq=seq, agg="mean", mode=mode, weight=0.2, K_log=10)
    s = HipSolver(d, "l2", smode, device=0)
    if smode == "cov":
        s.set_cov(o.cov)
    else:
        s.set_data(X, n_global=n)
    s.set_trek(pairs, seq, agg="mean", mode=mode, weight=0.2, K_log=10)
    W = np.zeros((d, d))
    res = s.minimize(W, 1.0, K, 1.0, 3e-4, tol=-1.0, lambda1=0.03, checkpoint=ckpt, want_checkpoints=True)
    Wr, tr = o.minimize(np.zeros((d, d)), 1.0, K, 1.0, 3e-4, tol=-1.0)
    s.close()
    assert res.iters == tr.iters == K
    print(f"\nloop {smode} d={d} {seq} {mode}: max|dW| {np.abs(W - Wr).max():.2e}")
    assert np.abs(W - Wr).max() <= 1e-9
    assert [c.iter for c in res.checkpoints] == [r["iter"] for r in tr.records]
    assert res.checkpoints
    for c, r in zip(res.checkpoints, tr.records):
        assert abs(c.obj - r["obj_total"]) <= 1e-10 * abs(r["obj_total"])
        assert abs(c.reg_trek_value - r["reg_trek_value"]) <= 1e-9 * abs(r["reg_trek_value"]) + 1e-13
        assert abs(c.grad_trek_norm - r["grad_trek_norm"]) <= 1e-9 * r["grad_trek_norm"] + 1e-13
    if mode == "log":
        assert all(c.grad_trek_norm == 0.0 for c in res.checkpoints)
