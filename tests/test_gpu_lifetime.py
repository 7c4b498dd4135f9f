"""Every device and pinned buffer of the library frees itself (csrc/owned_buf.h, csrc/devmem.h):
a call's scratch on return, also when the call raises, and a handle's buffers when it is destroyed.

All cases read midagma_debug_live_bytes(), the library's own count of the bytes its live buffers
asked for.  The device's free memory says nothing here: other jobs share the device.  The one
deliberate cache, the per-device log-det workspace, is filled by a warm-up before a baseline is
taken, and a second call must add nothing to it."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from midagma_amd import _lib  # noqa: E402
from midagma_amd.simulate import make_dataset  # noqa: E402


def live() -> int:
    return int(_lib.load().midagma_debug_live_bytes())


def warm_logdet(d: int) -> int:
    """One midagma_logdet_h_dev at d (fills the workspace cache for its padded size), then a second
    one that must add no byte.  Returns the baseline."""
    L = _lib.load()
    A = torch.full((d, d), 0.1 / d, dtype=torch.float64, device="cuda:0")
    h = torch.zeros((), dtype=torch.float64, device="cuda:0")

    def call():
        _lib.check(L.midagma_logdet_h_dev(C.c_void_p(A.data_ptr()), d, d, 1.0, C.c_void_p(h.data_ptr()), None, d,
                                          None), None, "logdet_h_dev")
        torch.cuda.synchronize()

    call()
    base = live()
    call()
    assert live() == base, "the log-det workspace cache grew on a second call at the same d"
    return base


def dataset(d, n, sem_type="gauss"):
    X, _, _ = make_dataset(d, n, seed=7, sem_type=sem_type)
    if sem_type == "gauss":
        X = X - X.mean(axis=0, keepdims=True)
    return np.ascontiguousarray(X, dtype=np.float64)


@pytest.mark.parametrize("n,d", [(1000, 20), (1000, 200)])   # the Gram's padded D = 128 and 256
def test_gram_and_colsum_free_their_scratch(n, d):
    from midagma_amd.solver import colsum_dev, gram
    X = dataset(d, n)
    Xd = torch.from_numpy(X).to("cuda:0")
    torch.cuda.synchronize()
    base = live()
    G = [gram(X, device=0) for _ in range(3)]
    assert live() == base, "midagma_gram (host X) kept scratch"
    Gd = [gram(Xd) for _ in range(3)]
    assert live() == base, "midagma_gram (device X) kept scratch"
    cs = [colsum_dev(Xd) for _ in range(3)]
    assert live() == base, "midagma_colsum_dev kept its partials"
    torch.cuda.synchronize()
    # (the calls did run: what they return is right)
    ref = X.T @ X
    assert np.abs(G[2].cpu().numpy() - ref).max() <= 1e-9 * np.abs(ref).max()
    assert np.abs(Gd[2].cpu().numpy() - ref).max() <= 1e-9 * np.abs(ref).max()
    assert np.abs(cs[2].cpu().numpy() - X.sum(axis=0)).max() <= 1e-9 * np.abs(X).sum(axis=0).max()
    # the error return: scratch allocated, the chunks run, then the non-finite flag raises
    Xbad = X.copy()
    Xbad[n // 2, d // 3] = np.nan
    with pytest.raises(ValueError):
        gram(Xbad, device=0)
    assert live() == base, "midagma_gram kept scratch on its non-finite error return"


def _cov_solver(d, n=None):
    from midagma_amd.solver import HipSolver
    X = dataset(d, n or 2 * d + 100)
    s = HipSolver(d, "l2", "cov", device=0)
    s.set_cov(X.T @ X / float(X.shape[0]))
    return s


def _pairs(d):
    iu = np.triu_indices(d, 1)
    return np.stack(iu, axis=1)[::3].astype(np.int64)


def life_cov_small():            # the one-workgroup path
    s = _cov_solver(20)
    W = np.zeros((20, 20))
    assert s.minimize(W, 1.0, 40, 1.0, 3e-4, tol=-1.0, lambda1=0.03).iters == 40
    return s


def life_cov_blocked():          # blocked inverse, fast slots; _h and _score allocate call scratch
    s = _cov_solver(300)
    W = np.zeros((300, 300))
    assert s.minimize(W, 1.0, 40, 1.0, 3e-4, tol=-1.0, lambda1=0.03).iters == 40
    s.h_value(W, 1.0)
    s.score_value(W)
    mid = live()                 # (the solver's own scratch and gradient buffers are sized now)
    s.h_value(W, 1.0)
    s.score_value(W)
    assert live() == mid, "midagma_h / midagma_score: their work buffer outlived the call"
    return s


def life_cov_trek():             # PST (tbufs, tgates), then TCC (cgates) on the same solver
    s = _cov_solver(20)
    W = np.zeros((20, 20))
    s.set_trek(_pairs(20), "exp", agg="mean", mode="opt", weight=0.2)
    assert s.minimize(W, 1.0, 20, 1.0, 3e-4, tol=-1.0, lambda1=0.03).iters == 20
    s.trek_value(W)
    s.set_trek_tcc(_pairs(20), mode="opt", weight=0.2)
    assert s.minimize(W, 1.0, 20, 1.0, 3e-4, tol=-1.0, lambda1=0.03).iters == 20
    s.trek_value(W)
    return s


def life_data_logistic():
    from midagma_amd.solver import HipSolver
    d, n = 70, 500
    X = dataset(d, n, "logistic")
    s = HipSolver(d, "logistic", "data", device=0)
    s.set_cov(X.T @ X / float(n))
    s.set_data(X, n_global=n)
    W = np.zeros((d, d))
    assert s.minimize(W, 1.0, 20, 1.0, 3e-4, tol=-1.0, lambda1=0.03).iters == 20
    return s


def life_cov_float32():
    s = _cov_solver(20)
    s.set_w_float32(True)
    W = np.zeros((20, 20))
    assert s.minimize(W, 1.0, 20, 1.0, 3e-4, tol=-1.0, lambda1=0.03).iters == 20
    return s


@pytest.mark.parametrize("life", [life_cov_small, life_cov_blocked, life_cov_trek, life_data_logistic,
                                  life_cov_float32], ids=lambda f: f.__name__)
def test_solver_returns_to_baseline(life):
    base = live()
    s = life()
    assert live() > base  # (the counter sees the solver's buffers)
    s.close()
    assert live() == base


def test_ldfast_returns_to_baseline():
    L = _lib.load()
    d = 100
    base = warm_logdet(d)
    A = torch.full((d, d), 0.1 / d, dtype=torch.float64, device="cuda:0")
    hv = torch.zeros((), dtype=torch.float64, device="cuda:0")
    Mt = torch.zeros((d, d), dtype=torch.float64, device="cuda:0")
    h = C.c_void_p()
    _lib.check(L.midagma_ldfast_create(C.byref(h), d), None, "ldfast_create")
    try:
        assert live() > base
        for exact in (1, 0):  # an exact step leaves the warm start the fast step needs
            _lib.check(L.midagma_ldfast_enqueue(h, C.c_void_p(A.data_ptr()), d, d, 1.0, C.c_void_p(hv.data_ptr()),
                                                C.c_void_p(Mt.data_ptr()), d, None, exact, -1), None, "ldfast_enqueue")
        torch.cuda.synchronize()
        assert np.isfinite(float(hv.item()))
    finally:
        L.midagma_ldfast_destroy(h)
    assert live() == base


def test_indep_returns_to_baseline():
    from midagma_amd.solver import HipIndep
    X = dataset(4, 64)
    pairs = np.array([[0, 1], [2, 3], [0, 3]])
    base = live()
    e = HipIndep(X, device=0)
    e.median_bandwidths()
    e.run("hsic", pairs, 8, seed=1)
    e.run("dcor", pairs, 8, seed=1)
    assert live() > base
    e.close()
    assert live() == base


def test_emulated_group_returns_to_baseline():
    from midagma_amd.solver import HipGroup
    d, n = 70, 512
    X = dataset(d, n)
    base = live()
    g = HipGroup(d, "l2", devices=[0, 0])
    assert g.emulated
    g.set_data(X)
    g.set_cov(X.T @ X / float(n))
    W = np.zeros((d, d))
    assert g.minimize(W, 1.0, 10, 1.0, 3e-4, tol=-1.0, lambda1=0.03).iters == 10
    assert live() > base
    g.close()
    assert live() == base
