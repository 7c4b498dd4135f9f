"""The DagmaMLP kernels (csrc/mlp.hip, csrc/adam.hip, the LdFast log-det) at every shape branch of
the production code, against the np.longdouble reference of tests/mlp_numpy.py (certified by
tests/test_mlp_numpy_cpu.py) and the CPU oracle's trajectories.  dims = [d, m1, 1] is user input:
each test's docstring names the branches its shapes select.

Value and gradient (test_objective_*): for each of h, obj and the four gradients,
err = max|got - ref| / max|ref| must be <= 8 max(e64, 2^-50), e64 the same error of OracleMLP's
float64 CPU autograd on the same inputs; 8 is the project's margin for another float64 summation
order (tests/blockinv_cases.check_inverse, tests/test_gpu_xty_strassen.py).  Largest err / e64
measured on an MI355X (the floor applied to e64), over the nine shapes:
    h 1.02 at (20, 10, 160), obj 1.00 at (1, 1, 5), fc1.weight 0.75 at (260, 8, 36), fc1.bias 0.45,
    fc2.0.weight 0.51, fc2.0.bias 0.46; the fallback's ssq 0.05 and its gradients 0.27
(h's error is that of forming sI - A in float64, which both sides share: err = e64 to three digits
at five shapes.  No quantity needs more than the 8.)
Steps (test_step_*, test_ldfast_*): the project's trajectory bars, 1e-9 max(1, |p|) against the CPU
oracle, 1e-12 between the graph and the eager loop and between the warm-started and the all-exact
log-det, bit identity between the one-launch step and the separate launches.  Largest deviations
measured, as max|dp| / max(1, |p|):
    12 steps: eager vs graph 1.4e-17, graph vs oracle 3.6e-15 (at (260, 8, 36))
    LdFast cells, 30 steps: fast vs all-exact 8.3e-17, fast vs oracle 9.3e-15 (d = 129); 4 of the
    30 steps ran the Gauss-Jordan chain at d = 128, 129 and 256

Mutations tried on a scratch copy of csrc/mlp.hip, one at a time (each fails the cases listed and
no other; "objective" and "step" are the two parametrised tests below):
    mlp_tail_fwd_kernel, the `j != j0` reload `b2[j]` -> `b2[j0]` (d > 256): objective and step at
        (260, 8, 36), objective at (496, 16, 40), test_ldfast_cells[257]
    mlp_tail_fwd_kernel, the staging loop reading `z[c - 2048]` for c >= 2048 (d m1 > 2048):
        objective and step at (260, 8, 36), objective at (496, 16, 40)
    fc1_terms_bwd_kernel, `lin[e]` -> `lin[(j m1) d + i]` (nlin = 1): objective at (7, 3, 33),
        (16, 17, 60), (260, 8, 36), (496, 16, 40) (every n that misses the split, m1 > 1); step at
        (7, 3, 33), (16, 17, 60), (260, 8, 36) (its runs with the separate launches)
    mlp_step_kernel, the register path taking 15 of its 16 weights (m1 = MU): step at (16, 16, 64)
    mlp_step_kernel, the generic loop's A from the weights before the update (m1 > 16): step at
        (16, 17, 60) and (12, 40, 1060)
    chunk_sum, the remainder loop of the `nchunk > KU` path dropped: step at (12, 40, 1060)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import mlp_numpy as ref  # noqa: E402

KEYS = list(ref.KEYS)
MU, LAMBDA1, S = 0.1, 0.02, 1.0
RATIO_BAR = 8.0
FLOOR = 2.0 ** -50
ARGS = (2e-4, 0.02, 0.005, 0.1, 1.0)  # lr, lambda1, lambda2, mu, s


def _gpu_model(d, m1, X, params, **kw):
    from midagma_amd.nonlinear import DagmaMLP, DagmaNonlinear
    from oracle.mlp_oracle import load_params
    model = DagmaMLP(dims=[d, m1, 1], bias=True).to("cuda:0")
    load_params(model, params)
    dn = DagmaNonlinear(model, device=0, **kw)
    dn.X = torch.from_numpy(np.ascontiguousarray(X)).to("cuda:0")
    return model, dn


def _grads(model):
    return {k: p.grad.detach().cpu().numpy().copy() for k, p in model.named_parameters()}


def _check(label, got, want, e64):
    """err <= 8 max(e64, 2^-50) for every quantity; prints err / e64 first."""
    bad = []
    for k in want:
        err, e = ref.rel_err(got[k], want[k]), max(ref.rel_err(e64[k], want[k]), FLOOR)
        print(f"{label} {k}: err {err:.3e}, e64 {e:.3e}, ratio {err / e:.2f}")
        if not err <= RATIO_BAR * e:
            bad.append((k, err, e))
    assert not bad, bad


OBJECTIVE_SHAPES = [(1, 1, 5), (7, 3, 33), (20, 10, 160), (16, 16, 64), (16, 17, 60), (12, 40, 1060), (260, 8, 36),
                    (496, 16, 40)]


@pytest.mark.parametrize("d,m1,n", OBJECTIVE_SHAPES)
def test_objective_value_and_gradient(d, m1, n):
    """DagmaNonlinear._h_and_objective and obj.backward() through the fused kernels: h, obj and the
    gradients of fc1.weight, fc1.bias, fc2.0.weight, fc2.0.bias against the longdouble reference.
    What each shape selects:
    (1, 1, 5)       every grid degenerate (one column, one (j, i) pair); nlin = 1; one partial row
                    chunk in mlp_tail_bwd_kernel.
    (7, 3, 33)      `_MLPObjective.backward` with nlin = 1 (n % 4 != 0: lin = dZ^T X, then
                    fc1_terms_bwd_kernel, thread per (j, i)) through the objective; two row chunks
                    (mlp_tail_dw_kernel's remainder loop only), the last one partial.
    (20, 10, 160)   nlin = 4 (fc1_terms_bwd_elem_kernel); five chunks: one group of four plus a
                    remainder in mlp_tail_dw_kernel.
    (16, 16, 64)    n = 16 LIN_SPLIT, the smallest n that takes the split-K dZ^T X.
    (16, 17, 60)    n % 4 = 0 but n < 64: nlin = 1 by the size rule.
    (12, 40, 1060)  34 chunks (mlp_tail_dw_kernel's groups of four with remainder 2); nlin = 4.
    (260, 8, 36)    mlp_tail_fwd_kernel's second passes: d m1 = 2080 > 2048 (the staging loop's
                    `c0 += SU * NTHREADS`) and d > 256 (`j += NTHREADS`, the `j != j0` reloads of
                    b2[j] and X[row d + j]); d^2 no multiple of 256 (fc1_terms' last workgroup);
                    nlin = 1 (n < 64), as at (496, 16, 40).
    (496, 16, 40)   d m1 = 7936 = MLP_TAIL_MAX_DM: launch_mlp_tail_fwd with exactly 64 KB of
                    dynamic LDS; fused_tail() is True at its bound (also d > 256 and four passes
                    of the staging loop)."""
    X, p = ref.draw_case(d, m1, n)
    want = ref.objective(X, p, MU, LAMBDA1, S)
    o64 = ref.oracle_objective(X, p, MU, LAMBDA1, S)
    assert float(want["h"]) > 0
    model, dn = _gpu_model(d, m1, X, p)
    assert model.fused_tail()
    h, obj = dn._h_and_objective(MU, LAMBDA1, S)
    obj.backward()
    got = dict(_grads(model), h=h.item(), obj=obj.item())
    _check(f"({d}, {m1}, {n})", got, dict(want["grads"], h=want["h"], obj=want["obj"]),
           dict(o64["grads"], h=o64["h"], obj=o64["obj"]))


def test_objective_above_the_lds_cap_falls_back():
    """(497, 16, 8): d m1 = 7952 > 7936, so `DagmaMLP.fused_tail()` is False and the objective runs
    PyTorch's expressions around the HIP log-det: h, obj, squared_residual and all their gradients
    meet the same bar."""
    d, m1, n = 497, 16, 8
    X, p = ref.draw_case(d, m1, n)
    want = ref.objective(X, p, MU, LAMBDA1, S)
    sq = ref.squared_residual(X, p)
    o64 = ref.oracle_objective(X, p, MU, LAMBDA1, S)
    model, dn = _gpu_model(d, m1, X, p)
    assert not model.fused_tail()
    ssq = model.squared_residual(dn.X)
    ssq.backward()
    _check(f"({d}, {m1}, {n}) ssq", dict(_grads(model), ssq=ssq.item()), dict(sq["grads"], ssq=sq["ssq"]),
           dict(o64["ssq_grads"], ssq=o64["ssq"]))
    model.zero_grad()
    h, obj = dn._h_and_objective(MU, LAMBDA1, S)
    obj.backward()
    _check(f"({d}, {m1}, {n})", dict(_grads(model), h=h.item(), obj=obj.item()),
           dict(want["grads"], h=want["h"], obj=want["obj"]), dict(o64["grads"], h=o64["h"], obj=o64["obj"]))


def _oracle_run(d, m1, X, params, K, checkpoint):
    from oracle.mlp_oracle import OracleMLP, load_params, nonlinear_minimize
    model = OracleMLP([d, m1, 1])
    load_params(model, params)
    ok, it = nonlinear_minimize(model, torch.from_numpy(np.ascontiguousarray(X)), K, *ARGS, tol=-1,
                                checkpoint=checkpoint)
    return ok, it, {k: v.detach().numpy().copy() for k, v in model.state_dict().items() if k in KEYS}


def _gpu_run(d, m1, X, params, K, checkpoint, **kw):
    model, dn = _gpu_model(d, m1, X, params, **kw)
    dn.checkpoint = checkpoint
    ok = dn.minimize(K, *ARGS, tol=-1)
    return ok, dn, {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items() if k in KEYS}


def _dev(a, b):
    """max over the parameters of max|a - b| / max(1, max|b|)."""
    return max(np.abs(a[k] - b[k]).max() / max(1.0, np.abs(b[k]).max()) for k in KEYS)


def _three_gpu_runs(monkeypatch, d, m1, X, p, K, checkpoint):
    """(i) the graph loop with the one-launch step, (ii) with MIDAGMA_NO_MLP_STEP=1, (iii) eager."""
    monkeypatch.delenv("MIDAGMA_NO_MLP_STEP", raising=False)
    monkeypatch.delenv("MIDAGMA_NO_GRAPH", raising=False)
    one = _gpu_run(d, m1, X, p, K, checkpoint)
    monkeypatch.setenv("MIDAGMA_NO_MLP_STEP", "1")
    sep = _gpu_run(d, m1, X, p, K, checkpoint)
    monkeypatch.delenv("MIDAGMA_NO_MLP_STEP", raising=False)
    eager = _gpu_run(d, m1, X, p, K, checkpoint, graph=False)
    return one, sep, eager


@pytest.mark.parametrize("d,m1,n", [(7, 3, 33), (16, 16, 64), (16, 17, 60), (12, 40, 1060), (260, 8, 36)])
def test_step_at_every_branch(d, m1, n, monkeypatch, parity):
    """12 Adam steps (checkpoints every 5) from identical parameters: (i) the graph loop closed by
    the one-launch `mlp_step_kernel`, (ii) the graph loop with the separate launches
    (MIDAGMA_NO_MLP_STEP=1), (iii) the eager loop, (iv) the CPU oracle.  (i) = (ii) bit for bit
    (`_MlpStep`'s claim), (iii) within 1e-12 of (i), (i) within 1e-9 of (iv), equal return values.
    (The graph loop's warm-up bodies run `mlp_step_kernel` with the gate shut: the A and l1part
    they leave, from the weights as they are, feed the first replayed step of (i).)
    What each shape selects in `mlp_step_kernel`:
    (7, 3, 33)      nlin = 1 through a step; `chunk_sum` with nchunk = 2 (remainder only).
    (16, 16, 64)    the register path at its bound m1 = MU = 16, nlin = 4 = LU; nchunk = 2.
    (16, 17, 60)    m1 = MU + 1: the generic loop instead of the register path; nlin = 1.
    (12, 40, 1060)  m1 >> 16: the generic loop with nlin = 4; `chunk_sum`'s `nchunk > KU` loop
                    (34 chunks, n > 1024) with remainder 34 % 4 = 2.
    (260, 8, 36)    the tail forward's second passes (d > 256, d m1 > 2048) inside a step; the
                    d > 256 log-det (no LdFast); nchunk = 2."""
    K, checkpoint = 12, 5
    X, p = ref.draw_case(d, m1, n)
    (ok1, _, one), (ok2, _, sep), (ok3, _, eager) = _three_gpu_runs(monkeypatch, d, m1, X, p, K, checkpoint)
    ok4, it, orc = _oracle_run(d, m1, X, p, K, checkpoint)
    assert ok1 is True and ok1 == ok2 == ok3 == ok4 and it == K
    moved = max(np.abs(one[k] - p[k].reshape(one[k].shape)).max() for k in KEYS)
    d_eager, d_orc = _dev(eager, one), _dev(one, orc)
    print(f"({d}, {m1}, {n}): moved {moved:.3e}, eager vs graph {d_eager:.3e}, graph vs oracle {d_orc:.3e}")
    parity("config5", d_orc, 1e-9, f"max|dparam|/max(1,|p|) K={K} dims [{d}, {m1}, 1] n={n}")
    assert moved > 1e-4  # (K steps of lr = 2e-4: the parameters did move)
    for k in KEYS:
        assert np.array_equal(one[k], sep[k]), k
    assert d_eager <= 1e-12
    assert d_orc <= 1e-9


@pytest.mark.parametrize("d", [128, 129, 256, 257])
def test_ldfast_cells(d, monkeypatch, parity):
    """LdFast (`midagma_ldfast_create`) at the edges of its series block: d = 128 (B = 128 full),
    129 (B = 256, the smallest), 256 (B = 256 full), 257 (no fast path: `_ldfast` is None and
    every step runs the Gauss-Jordan chain).  30 steps with checkpoints every 10, m1 = 2, n = 64:
    within 1e-9 of the oracle and 1e-12 of the all-exact run (MIDAGMA_NO_LDFAST=1), the bars of
    test_config5_ldfast_path_matches_oracle; for d <= 256 the fast path carried steps.  (d = 257 is
    also a d > 256 run through `minimize`: the tail forward's `j != j0` reloads.)"""
    m1, n, K, checkpoint = 2, 64, 30, 10
    X, p = ref.draw_case(d, m1, n)
    monkeypatch.delenv("MIDAGMA_NO_LDFAST", raising=False)
    ok1, dn, fast = _gpu_run(d, m1, X, p, K, checkpoint)
    if d <= 256:
        steps, exact = dn._ld.stats()
        print(f"d={d}: LdFast steps {steps}, of which exact {exact}")
        assert steps == K and exact < steps, (steps, exact)
    else:
        assert dn._ldfast(torch.device("cuda", 0)) is None
    monkeypatch.setenv("MIDAGMA_NO_LDFAST", "1")
    ok2, dn2, exact_only = _gpu_run(d, m1, X, p, K, checkpoint)
    assert dn2._ldfast(torch.device("cuda", 0)) is None
    ok4, it, orc = _oracle_run(d, m1, X, p, K, checkpoint)
    assert ok1 is True and ok1 == ok2 == ok4 and it == K
    d_exact, d_orc = _dev(fast, exact_only), _dev(fast, orc)
    print(f"d={d}: fast vs all-exact {d_exact:.3e}, fast vs oracle {d_orc:.3e}")
    parity("config5", d_orc, 1e-9, f"max|dparam|/max(1,|p|) K={K} dims [{d}, {m1}, 1] n={n} (LdFast cell)")
    assert d_orc <= 1e-9
    assert d_exact <= 1e-12


def test_shut_gate_moves_nothing(monkeypatch):
    """A start with h < 0 (d = 5, m1 = 4, fc1.weight = 0.6: h = -1.82): `mlp_step_kernel` and the
    `adam_*` kernels with the gate shut (`*gate < 0`) move nothing, in the graph loop with the
    one-launch step, with the separate launches and in the eager loop: each returns False with all
    four parameter tensors bit-equal to the start, as the oracle returns False before stepping."""
    from oracle.mlp_oracle import OracleMLP, load_params
    d, m1, n, K = 5, 4, 50, 6
    X, p = ref.draw_case(d, m1, n)
    p["fc1.weight"] = np.full((d * m1, d), 0.6)
    cpu = OracleMLP([d, m1, 1])
    load_params(cpu, p)
    h0 = cpu.h_func(1.0).item()
    assert h0 < -1.0, h0
    ok4, it, orc = _oracle_run(d, m1, X, p, K, 5)
    assert ok4 is False and it == 0
    for ok, _, out in _three_gpu_runs(monkeypatch, d, m1, X, p, K, 5):
        assert ok is False
        for k in KEYS:
            assert np.array_equal(out[k], p[k].reshape(out[k].shape)), k
            assert np.array_equal(out[k], orc[k]), k
