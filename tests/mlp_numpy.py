"""Plain np.longdouble statement of the [d, m1, 1] DagmaMLP objective and its analytic gradient
(tests/test_mlp_numpy_cpu.py certifies it, tests/test_gpu_mlp_shapes.py holds csrc/mlp.hip to it).
It follows oracle/mlp_oracle.py and the reference's nonlinear.py:68-86, 139-159, 198-204:

    Z = X W1^T + b1,  S = sigmoid(Z),  Xhat[r, j] = sum_m S[r, j m1 + m] w2[j, m] + b2[j]
    ssq = sum (Xhat - X)^2,  score = 0.5 d log(ssq / n),  l1 = sum |W1|
    A[i, j] = sum_m W1[j m1 + m, i]^2,  h = -log|det(sI - A)| + d log s
    obj = mu (score + lambda1 l1) + h

No torch and no BLAS: numpy's longdouble matmul is its own loop, and the log-det and (sI - A)^-1
come from one longdouble Gauss-Jordan elimination with partial pivoting, a row operation at a time.
"""
import numpy as np

LD = np.longdouble
KEYS = ("fc1.weight", "fc1.bias", "fc2.0.weight", "fc2.0.bias")
QUANTITIES = ("h", "obj") + KEYS


def _check_longdouble():
    assert np.finfo(LD).eps < 2e-19, "np.longdouble is not the 80-bit extended type here"


def logdet_inverse(M):
    """(log|det M|, inv(M)) of a square longdouble M by Gauss-Jordan elimination with partial
    pivoting on [M | I]; the inverse's own residual max|I - M inv| is asserted <= 1e-17 max|inv|."""
    _check_longdouble()
    M = np.asarray(M, dtype=LD)
    d = M.shape[0]
    T = np.concatenate([M, np.eye(d, dtype=LD)], axis=1)
    logdet = LD(0)
    for k in range(d):
        p = k + int(np.argmax(np.abs(T[k:, k])))
        if p != k:
            T[[k, p]] = T[[p, k]]
        piv = T[k, k]
        assert piv != 0, "singular matrix"
        logdet += np.log(np.abs(piv))
        T[k] = T[k] / piv
        col = T[:, k].copy()
        col[k] = 0
        # about d + 1 of the 2 d columns: the rest of row k is zero.  Left of d they are k .. d - 1;
        # right of it a leading run when no rows were exchanged (a slice, not a gather)
        T[:, k:d] -= col[:, None] * T[k, k:d][None, :]
        nz = np.flatnonzero(T[k, d:])
        if nz.size and nz[-1] + 1 == nz.size:
            T[:, d:d + nz.size] -= col[:, None] * T[k, d:d + nz.size][None, :]
        else:
            T[:, d + nz] -= col[:, None] * T[k, d + nz][None, :]
    inv = T[:, d:].copy()
    res = float(np.abs(np.eye(d, dtype=LD) - M @ inv).max())
    assert res <= 1e-17 * float(np.abs(inv).max()), res
    return logdet, inv


def sigmoid(Z):
    return 1 / (1 + np.exp(-Z))


def residual_terms(X, W1, b1, w2, b2):
    """(S as (n, d, m1), E = Xhat - X, ssq) in longdouble; w2 is (d, m1), b2 is (d,)."""
    n, d = X.shape
    m1 = w2.shape[1]
    S = sigmoid(X @ W1.T + b1).reshape(n, d, m1)
    E = (S * w2[None]).sum(axis=2) + b2[None] - X
    return S, E, (E * E).sum()


def _as_ld(X, params):
    _check_longdouble()
    X = np.asarray(X, dtype=LD)
    d = X.shape[1]
    W1 = np.asarray(params["fc1.weight"], dtype=LD)
    m1 = W1.shape[0] // d
    assert W1.shape == (d * m1, d)
    b1 = np.asarray(params["fc1.bias"], dtype=LD).reshape(d * m1)
    w2 = np.asarray(params["fc2.0.weight"], dtype=LD).reshape(d, m1)
    b2 = np.asarray(params["fc2.0.bias"], dtype=LD).reshape(d)
    return X, W1, b1, w2, b2, d, m1


def _tail_grads(X, S, w2, G):
    """The gradients of sum_rj G-weighted Xhat, G = d(.)/dXhat (n, d): (dZ^T X, db1, dw2, db2)."""
    n, d = X.shape
    dZ = (G[:, :, None] * w2[None] * S * (1 - S)).reshape(n, -1)
    return dZ.T @ X, dZ.sum(axis=0), (G[:, :, None] * S).sum(axis=0), G.sum(axis=0)


def squared_residual(X, params):
    """ssq and its gradients by parameter name (the shapes of the model's tensors)."""
    X, W1, b1, w2, b2, d, m1 = _as_ld(X, params)
    S, E, ssq = residual_terms(X, W1, b1, w2, b2)
    gW1, gb1, gw2, gb2 = _tail_grads(X, S, w2, 2 * E)
    return {"ssq": ssq, "grads": {"fc1.weight": gW1, "fc1.bias": gb1, "fc2.0.weight": gw2.reshape(d, m1, 1),
                                  "fc2.0.bias": gb2.reshape(d, 1)}}


def value(X, params, mu, lambda1, s):
    """(h, obj) alone (the finite-difference check's function)."""
    X, W1, b1, w2, b2, d, m1 = _as_ld(X, params)
    n = X.shape[0]
    _, _, ssq = residual_terms(X, W1, b1, w2, b2)
    A = (W1.reshape(d, m1, d) ** 2).sum(axis=1).T
    logdet, _ = logdet_inverse(LD(s) * np.eye(d, dtype=LD) - A)
    h = -logdet + d * np.log(LD(s))
    score = LD(0.5) * d * np.log(ssq / n)
    return h, LD(mu) * (score + LD(lambda1) * np.abs(W1).sum()) + h


def objective(X, params, mu, lambda1, s):
    """{"h", "obj", "ssq", "grads": d obj / d parameter by name}, everything np.longdouble."""
    X, W1, b1, w2, b2, d, m1 = _as_ld(X, params)
    n = X.shape[0]
    mu, lambda1, s = LD(mu), LD(lambda1), LD(s)
    S, E, ssq = residual_terms(X, W1, b1, w2, b2)
    score = LD(0.5) * d * np.log(ssq / n)
    W3 = W1.reshape(d, m1, d)  # [j, m, i]
    A = (W3 ** 2).sum(axis=1).T  # [i, j]
    logdet, inv = logdet_inverse(s * np.eye(d, dtype=LD) - A)
    h = -logdet + d * np.log(s)
    obj = mu * (score + lambda1 * np.abs(W1).sum()) + h
    # d score / d Xhat = d E / ssq;  d h / d A = (sI - A)^-T, so d h / d W1[j m1 + m, i] = 2 W1 inv[j, i]
    gW1, gb1, gw2, gb2 = _tail_grads(X, S, w2, mu * d / ssq * E)
    gW1 = gW1 + mu * lambda1 * np.sign(W1) + (2 * W3 * inv[:, None, :]).reshape(d * m1, d)
    return {"h": h, "obj": obj, "ssq": ssq,
            "grads": {"fc1.weight": gW1, "fc1.bias": gb1, "fc2.0.weight": gw2.reshape(d, m1, 1),
                      "fc2.0.bias": gb2.reshape(d, 1)}}


def draw_case(d, m1, n, seed=None):
    """(X, params) in float64 as the shape tests draw them: fc1 ~ N(0, 0.3 / sqrt(d m1)) (sI - A an
    M-matrix), b1 ~ N(0, 0.1), w2 and b2 with magnitudes in [0.5, 1.5] and random signs (nonzero
    and distinct per column: a swapped column is an O(1) error), X standard normal with per-column
    scales e^U(-1, 1)."""
    rng = np.random.default_rng(1000003 * d + 1009 * m1 + n if seed is None else seed)
    X = rng.standard_normal((n, d)) * np.exp(rng.uniform(-1, 1, d))[None, :]
    sgn = lambda shape: rng.choice([-1.0, 1.0], size=shape)  # noqa: E731
    params = {"fc1.weight": rng.standard_normal((d * m1, d)) * (0.3 / np.sqrt(d * m1)),
              "fc1.bias": rng.standard_normal(d * m1) * 0.1,
              "fc2.0.weight": rng.uniform(0.5, 1.5, (d, m1, 1)) * sgn((d, m1, 1)),
              "fc2.0.bias": rng.uniform(0.5, 1.5, (d, 1)) * sgn((d, 1))}
    return X, params


def oracle_objective(X, params, mu, lambda1, s):
    """OracleMLP's float64 CPU autograd on the same inputs (torch; the e64 yardstick):
    {"h", "obj", "ssq", "grads", "ssq_grads"} as float64 numpy."""
    import torch

    from oracle.mlp_oracle import OracleMLP, load_params
    d = X.shape[1]
    m1 = params["fc1.weight"].shape[0] // d
    model = OracleMLP([d, m1, 1])
    load_params(model, params)
    Xt = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64))
    n = Xt.shape[0]
    names = dict(model.named_parameters())
    ssq = torch.sum((model(Xt) - Xt) ** 2)
    ssq.backward()
    ssq_grads = {k: names[k].grad.numpy().copy() for k in KEYS}
    model.zero_grad()
    h = model.h_func(s)
    obj = mu * (0.5 * d * torch.log(1 / n * torch.sum((model(Xt) - Xt) ** 2)) + lambda1 * model.fc1_l1_reg()) + h
    obj.backward()
    return {"h": h.item(), "obj": obj.item(), "ssq": ssq.item(),
            "grads": {k: names[k].grad.numpy().copy() for k in KEYS}, "ssq_grads": ssq_grads}


def rel_err(got, ref):
    """max|got - ref| / max|ref| with the difference taken in longdouble."""
    ref = np.asarray(ref, dtype=LD)
    got = np.asarray(got, dtype=LD).reshape(ref.shape)
    return float(np.abs(got - ref).max() / np.abs(ref).max())
