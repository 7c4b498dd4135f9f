"""Certifies tests/mlp_numpy.py, the np.longdouble reference the GPU shape tests
(tests/test_gpu_mlp_shapes.py) hold csrc/mlp.hip to.  No GPU.

(a) Its analytic gradient against its own value by central differences taken in longdouble, along
    directions: per parameter tensor three random unit-max directions and six coordinate directions
    (the first and last element and four random ones), so that both a wrong term and a wrong index
    show.  Step t = eps^(1/3) (4.8e-7 with eps = 1.08e-19, the balance of the truncation t^2 f'''/6
    and the rounding eps |obj| / t, each ~eps^(2/3) = 2.3e-13).  Bar: |fd - <grad, v>| <= 100
    eps^(2/3) max(1, |obj|) = 2.3e-11 max(1, |obj|); the 100 is the allowance for f''' / 6 and for
    the rounding of the value's own sums, both O(1) to O(10) multiples of eps^(2/3) here.  Largest
    deviation seen: 3.7e-13 at (5, 3, 17), 4.6e-12 at (12, 17, 60) (|obj| = 2.9: 1.6e-12
    max(1, |obj|), 7% of the bar), 1.4e-12 at (33, 2, 64); the derivatives are 1e-3 .. 1.
(b) OracleMLP's float64 CPU autograd against the reference on h, obj, the squared residual sum and
    every gradient of obj and of ssq, as err = max|got - ref| / max|ref|.  Bar 1e-12: float64 sums
    of up to n d m1 = 12240 terms, eps64 n d m1 = 2.7e-12 at worst and ~eps64 sqrt(n d m1) =
    2.5e-14 typically; h = -log|det(I - A)| ~ 0.1 is a sum of d logs of pivots near 1 whose
    float64 rounding (1.1e-16 absolute each) is 1e-15 .. 1e-14 of h.  Seen (e64, the yardstick of
    the GPU tier's 8 x bar), largest over the three shapes:
        h 2.7e-15, obj 1.1e-16, ssq 8.2e-17, d obj: fc1.weight 5.3e-16, fc1.bias 3.1e-16,
        fc2.0.weight 3.1e-16, fc2.0.bias 2.6e-16; d ssq: 4.4e-16, 1.0e-16, 1.8e-16, 1.7e-16
    and at the GPU tier's own shapes (up to (496, 16, 40)): h up to 7.5e-14 (d = 260), the
    gradients up to 1.1e-15 (fc1.weight at d = 496), obj up to 1.3e-15.
"""
import numpy as np
import pytest

from tests import mlp_numpy as ref

SHAPES = [(5, 3, 17), (12, 17, 60), (33, 2, 64)]
MU, LAMBDA1, S = 0.1, 0.02, 1.0


def test_logdet_inverse_pivots():
    """The elimination on a matrix that needs its row exchanges (a permuted, scaled M-matrix):
    log|det| and the inverse against the factors it was built from."""
    rng = np.random.default_rng(0)
    d = 9
    M0 = (np.eye(d) - rng.uniform(0, 1, (d, d)) * 0.5 / d).astype(ref.LD)
    perm = rng.permutation(d)
    scale = np.exp(rng.uniform(-3, 3, d)).astype(ref.LD)
    M = (M0 * scale[:, None])[perm]  # (the products round in longdouble: ~1e-19 of each entry)
    ld0, inv0 = ref.logdet_inverse(M0)
    ld, inv = ref.logdet_inverse(M)
    assert abs(float(ld - (ld0 + np.log(scale).sum()))) <= 1e-17 * d
    want = (inv0 / scale[None, :])[:, perm]  # inv(P D M0) = inv(M0) inv(D) P^T
    assert float(np.abs(inv - want).max()) <= 1e-16 * float(np.abs(want).max())


@pytest.mark.parametrize("d,m1,n", SHAPES)
def test_gradient_matches_central_differences(d, m1, n):
    """(a) of the module docstring."""
    eps = float(np.finfo(ref.LD).eps)
    t = ref.LD(eps ** (1.0 / 3.0))
    X, p = ref.draw_case(d, m1, n)
    out = ref.objective(X, p, MU, LAMBDA1, S)
    bar = 100 * eps ** (2.0 / 3.0) * max(1.0, abs(float(out["obj"])))
    rng = np.random.default_rng(d + m1 + n)
    worst = 0.0
    for k in ref.KEYS:
        g = out["grads"][k]
        assert g.shape == p[k].shape and g.dtype == ref.LD
        dirs = [rng.uniform(-1, 1, g.shape) for _ in range(3)]
        for flat in [0, g.size - 1] + list(rng.integers(0, g.size, 4)):
            v = np.zeros(g.size)
            v[flat] = 1.0
            dirs.append(v.reshape(g.shape))
        for v in dirs:
            v = v.astype(ref.LD)
            vals = []
            for sign in (1, -1):
                q = {kk: np.asarray(vv, dtype=ref.LD) for kk, vv in p.items()}
                q[k] = q[k] + sign * t * v
                vals.append(ref.value(X, q, MU, LAMBDA1, S)[1])
            fd = (vals[0] - vals[1]) / (2 * t)
            dev = abs(float(fd - (g * v).sum()))
            worst = max(worst, dev)
            assert dev <= bar, (k, dev, bar)
    print(f"({d}, {m1}, {n}): central differences, worst |fd - <grad, v>| = {worst:.3e} (bar {bar:.3e})")


@pytest.mark.parametrize("d,m1,n", SHAPES)
def test_oracle_autograd_matches_reference(d, m1, n):
    """(b) of the module docstring; also the reference's squared residual sum and its gradients
    (the GPU tier's yardstick where the model falls back to PyTorch's tail)."""
    pytest.importorskip("torch")
    X, p = ref.draw_case(d, m1, n)
    out = ref.objective(X, p, MU, LAMBDA1, S)
    sq = ref.squared_residual(X, p)
    o64 = ref.oracle_objective(X, p, MU, LAMBDA1, S)
    assert float(out["h"]) > 0
    errs = {"h": ref.rel_err(o64["h"], out["h"]), "obj": ref.rel_err(o64["obj"], out["obj"]),
            "ssq": ref.rel_err(o64["ssq"], sq["ssq"])}
    for k in ref.KEYS:
        errs[k] = ref.rel_err(o64["grads"][k], out["grads"][k])
        errs["ssq " + k] = ref.rel_err(o64["ssq_grads"][k], sq["grads"][k])
    print(f"({d}, {m1}, {n}): e64 " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= 1e-12, (k, v)
