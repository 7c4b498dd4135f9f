"""Certifies the long-double restatement of the PST penalty (tests/trek_numpy.py), and the float64
oracle (oracle/trek_oracle.py) where tests/test_gpu_trek_shapes.py uses it.  CPU only.

  1. the restatement against the reference's own recordings (tests/golden/trek_pst.npz, 32 cells);
  2. its gradient against long-double central differences, exp up to ||W o W||_1 = 517;
  3. the oracle against the restatement on the GPU tests' inputs with d <= 65: at
     ||W o W||_1 <= 8 it meets the bars the GPU tests ask of the kernel, above that its
     gradient is printed, not asserted -- torch's matrix_exp backward scales the block matrix by
     the upstream gradient's norm and loses digits there, which is why the large-norm GPU cells are
     judged by the restatement ("PST regularizer");
  4. the tie cases of the GPU tests do hold exact ties.

Run with -s for the oracle-versus-long-double table.
"""
import numpy as np
import pytest

from tests import trek_numpy as tn

LD = np.longdouble


def _dev(v, g, v_ref, g_ref):
    """Deviations relative to max(1, |.|), as floats."""
    dv = abs(LD(v) - v_ref) / max(LD(1.0), abs(v_ref))
    dg = np.abs(np.asarray(g, dtype=LD) - g_ref).max() / max(LD(1.0), np.abs(g_ref).max())
    return float(dv), float(dg)


@pytest.mark.parametrize("d", [8, 20])
@pytest.mark.parametrize("seq", tn.SEQS)
@pytest.mark.parametrize("agg", tn.AGGS)
def test_restatement_matches_reference_recordings(golden, d, seq, agg):
    """Bars 1e-12 max(1, |.|): the fixture is the reference's float64 output."""
    f = golden("trek_pst.npz")
    v, g = tn.pst_value_grad_ld(f[f"W_d{d}"], f[f"pairs_d{d}"], seq, agg, K_log=12 if seq == "log" else None)
    dv, dg = _dev(float(f[f"val_{seq}_{agg}_d{d}"]), f[f"grad_{seq}_{agg}_d{d}"], v, g)
    assert dv <= 1e-12 and dg <= 1e-12, (dv, dg)


@pytest.mark.parametrize("seq,norm,agg", [("exp", 0.2475, "lse"), ("exp", 16 * 0.99, "mean"), ("exp", 517.0, "max"),
                                          ("exp", 517.0, "lse"), ("inv", 0.7, "max"), ("log", 0.9, "lse"),
                                          ("binom", 0.4, "mean")])
def test_restatement_gradient_matches_central_differences(seq, norm, agg):
    """The three largest-|g| entries against (v(w + h) - v(w - h)) / 2h in long double,
    h = 2^-24 |w|: truncation ~ h^2 f'''/f' and rounding ~ 2^-64 / 2^-24 both sit far below the
    2e-9 bar."""
    d = 20
    W, pairs = tn.squaring_case(d, norm)
    K = None
    v, g = tn.pst_value_grad_ld(W, pairs, seq, agg, K)
    assert np.isfinite(float(v)) and np.abs(g).max() > 0
    worst = 0.0
    for e in np.argsort(-np.abs(g), axis=None)[:3]:
        i, j = divmod(int(e), d)
        Wp, Wm = W.astype(LD), W.astype(LD)
        h = LD(2.0) ** -24 * abs(Wp[i, j])
        Wp[i, j] += h
        Wm[i, j] -= h
        fd = (tn.pst_value_ld(Wp, pairs, seq, agg, K) - tn.pst_value_ld(Wm, pairs, seq, agg, K)) / (2 * h)
        worst = max(worst, float(abs(fd - g[i, j]) / abs(g[i, j])))
    print(f"\ncentral differences {seq} ||W2||_1={norm:g} {agg}: worst relative gap {worst:.2e}")
    assert worst <= 2e-9


def _oracle(W, pairs, seq, agg, K_log):
    from oracle.trek_oracle import pst_value_grad
    return pst_value_grad(W, pairs, seq, K_log=K_log, agg=agg)


@pytest.mark.parametrize("cell", [i for i, c in enumerate(tn.SHAPE_CELLS) if c[1] <= tn.LD_MAX_D])
def test_oracle_certified_on_small_shape_cells(cell):
    pytest.importorskip("torch")
    _, d, _, seqs = tn.SHAPE_CELLS[cell]
    for seq in seqs:
        agg, K = tn.shape_cell_agg(cell, seq), tn.shape_cell_klog(d, seq)
        W, pairs = tn.shape_case(d, seq)
        assert tn.norm1_w2(W) <= 8
        dv, dg = _dev(*_oracle(W, pairs, seq, agg, K), *tn.pst_value_grad_ld(W, pairs, seq, agg, K))
        print(f"\noracle vs long double, shape cell d={d} {seq} {agg}: value {dv:.1e} gradient {dg:.1e}")
        assert dv <= 1e-11 and dg <= 1e-10


@pytest.mark.parametrize("agg", ["mean", "max", "lse"])
@pytest.mark.parametrize("d", [20, 65])
def test_oracle_against_long_double_over_the_squaring_buckets(d, agg):
    """The table of DESIGN.md section 5: at ||W o W||_1 <= 8 the oracle meets the GPU bars (value
    1e-11, gradient 1e-10, relative to max(1, |.|)); above, its value still does and its gradient
    is printed only."""
    pytest.importorskip("torch")
    print(f"\noracle vs long double, exp, d={d}, {agg}:   s  ||W2||_1    value     gradient")
    for s, edge, norm in tn.bucket_norms():
        W, pairs = tn.squaring_case(d, norm)
        assert tn.squaring_count(W) == s
        dv, dg = _dev(*_oracle(W, pairs, "exp", agg, None), *tn.pst_value_grad_ld(W, pairs, "exp", agg))
        print(f"    {s:2d} {edge} {norm:9.4f}  {dv:.1e}  {dg:.1e}")
        assert dv <= 1e-11
        if norm <= 8:
            assert dg <= 1e-10


def test_oracle_certified_on_the_pair_list_cases():
    pytest.importorskip("torch")
    for name, (W, pairs, seq, aggs) in tn.pairlist_cases().items():
        K = 7 if seq == "log" else None
        for agg in aggs:
            dv, dg = _dev(*_oracle(W, pairs, seq, agg, K), *tn.pst_value_grad_ld(W, pairs, seq, agg, K))
            print(f"\noracle vs long double, pair list {name} {seq} {agg} m={len(pairs)}: value {dv:.1e} "
                  f"gradient {dg:.1e}")
            assert dv <= 1e-11 and dg <= 1e-10


@pytest.mark.parametrize("name", sorted(tn.TIE_CASES))
def test_tie_cases_hold_exact_ties(name):
    """A tie case must not pass vacuously: the restatement sees the exact ties it is about."""
    W, pairs, seq, _ = tn.pairlist_cases()[name]
    _, v = tn.pair_values_ld(W, pairs, seq, 7 if seq == "log" else None)
    if name.startswith("ties-"):          # zeros below one positive maximum
        assert int((v == 0).sum()) >= tn.TIE_CASES[name] and int((v == v.max()).sum()) == 1 and v.max() > 0
    else:                                 # ties at the maximum itself
        assert int((v == v.max()).sum()) >= tn.TIE_CASES[name]
    if name.startswith("allzero-"):
        assert not v.any()
    if name.startswith(("dyadic-", "ties-", "tiled")):   # a gradient for the ties to share, or stay out of
        assert v.max() > 0 and tn.pst_value_grad_ld(W, pairs, seq, "max", 7)[1].any()


def test_threshold_case_sits_on_the_threshold():
    W, _ = tn.threshold_case(20)
    assert tn.norm1_w2(W) == tn.THETA and tn.squaring_count(W) == 0
