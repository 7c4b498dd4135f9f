"""Bootstrap covariances on the device (csrc/boot.hip, `HipBatch.boot_cov`) and
`DagmaLinearBatch.bootstrap`: replicate b's covariance against numpy on `bootstrap_indices`, its
independence of how the replicates are grouped, the downstream bit identity with `set_cov`, and the
fits against `LinearOracle.fit` on the gathered resamples.

The row tile of the Gram kernel is 64 rows and a row range (one partial) is max(256, ceil(n / 32)
rounded up to 64) rows, so n = 63..65 crosses a tile and n = 255..257 a range; n = 8300 takes ranges
of 320 rows."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from midagma_amd import _lib  # noqa: E402
from midagma_amd.batch import DagmaLinearBatch, bootstrap_indices  # noqa: E402
from midagma_amd.simulate import make_dataset  # noqa: E402
from oracle.dagma_oracle import LinearOracle  # noqa: E402
from tests.test_batch_cpu import FIT_ARGS  # noqa: E402

U = 2.0 ** -53
NS = [1, 2, 37, 63, 64, 65, 255, 256, 257, 1000]


def _data(n, d, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)) @ (np.eye(d) + 0.3 * rng.standard_normal((d, d))) + rng.standard_normal(d)


def _reference(X, seed, b):
    """(cov of replicate b as numpy states it, the per-entry tolerance 2 n 2^-53 sqrt(S_ii S_jj) with
    S the second moment of the resampled, globally centred rows)."""
    n = X.shape[0]
    idx = bootstrap_indices(seed, b, n)
    Xb = X[idx]
    Xb = Xb - Xb.mean(axis=0, keepdims=True)
    cov = Xb.T @ Xb / float(n)
    Yb = (X - X.mean(axis=0, keepdims=True))[idx]
    s = np.sqrt(np.diag(Yb.T @ Yb / float(n)))
    return cov, 2.0 * n * U * np.outer(s, s)


def _slabs(bt):
    out = np.empty((bt.B, 64, 64))
    assert bt.L.midagma_debug_batch_cov_slabs(bt.h, _lib.dptr(out)) == 0
    return out


def _check_covs(bt, X, seed, first=0):
    n, d = X.shape
    got = bt.get_cov()
    slabs = _slabs(bt)
    worst = 0.0
    for b in range(bt.B):
        ref, tol = _reference(X, seed, first + b)
        err = np.abs(got[b] - ref)
        if tol.max() > 0:
            worst = max(worst, float((err / np.where(tol > 0, tol, 1.0)).max()))
        assert (err <= tol).all(), (n, d, b, float(err.max()), float(tol.max()))
        assert np.array_equal(got[b], got[b].T), (n, d, b)
        if n == 1:
            assert not got[b].any()
        assert np.array_equal(slabs[b, :d, :d], got[b])
        pad = slabs[b].copy()
        pad[:d, :d] = 0
        assert not pad.any(), (n, d, b)
    return worst


@pytest.mark.parametrize("d", [1, 5, 16, 17, 20, 32, 33, 64])
def test_boot_cov_matches_numpy_on_bootstrap_indices(d):
    from midagma_amd.solver import HipBatch
    B, seed = 5, 7  # (5 is no multiple of a replicate group: 8, 16 or 32)
    bt = HipBatch(d, B, device=0)
    try:
        worst = 0.0
        for n in NS + ([8300] if d in (20, 64) else []):
            X = _data(n, d, 100 * d + n)
            X0 = X.copy()
            bt.boot_cov(X, seed)
            assert np.array_equal(X, X0)
            worst = max(worst, _check_covs(bt, X, seed))
        print(f"d={d}: worst error / tolerance = {worst:.3g}")
    finally:
        bt.close()


def test_boot_cov_with_a_large_offset():
    """Fails if the global centring is skipped: a column mean of 1e6 then costs about 4 digits."""
    from midagma_amd.solver import HipBatch
    d, n, seed = 20, 400, 11
    X = _data(n, d, 3) + 1e6
    bt = HipBatch(d, 5, device=0)
    try:
        bt.boot_cov(X, seed)
        print(f"offset 1e6: worst error / tolerance = {_check_covs(bt, X, seed):.3g}")
    finally:
        bt.close()


@pytest.mark.parametrize("d,n", [(5, 300), (20, 1000), (64, 300)])
def test_boot_cov_does_not_depend_on_the_grouping(d, n):
    from midagma_amd.solver import HipBatch
    seed = 0xFEEDFACE12345
    X = _data(n, d, 5)
    X0 = X.copy()
    bt = HipBatch(d, 8, device=0)
    one = HipBatch(d, 1, device=0)
    try:
        bt.boot_cov(X, seed)
        want = bt.get_cov()
        bt.boot_cov(X, seed)  # a repeated call
        assert np.array_equal(bt.get_cov(), want)
        bt.boot_cov(X, seed, budget_bytes=1)  # one replicate per chunk
        assert np.array_equal(bt.get_cov(), want)
        for b in range(8):  # a batch of one from first = b
            one.boot_cov(X, seed, first=b)
            assert np.array_equal(one.get_cov()[0], want[b]), b
        bt.boot_cov(X, seed, first=3)
        assert np.array_equal(bt.get_cov()[:5], want[3:])
        # a device X whose rows are not contiguous gives the bits of the host X
        wide = torch.zeros((n, d + 7), dtype=torch.float64, device="cuda")
        wide[:, 3:3 + d] = torch.from_numpy(X)
        Xd = wide[:, 3:3 + d]
        assert Xd.stride(0) == d + 7
        keep = wide.clone()
        bt.boot_cov(Xd, seed)
        assert np.array_equal(bt.get_cov(), want)
        assert torch.equal(wide, keep) and np.array_equal(X, X0)
    finally:
        bt.close()
        one.close()


@pytest.mark.parametrize("d", [20, 64])
def test_boot_cov_then_minimize_equals_set_cov_of_the_same_bits(d):
    from midagma_amd.solver import HipBatch
    B, K, seed = 3, 300, 21
    X = make_dataset(d, 400, seed=2)[0]
    a, b = HipBatch(d, B, device=0), HipBatch(d, B, device=0)
    try:
        a.boot_cov(X, seed)
        b.set_cov(a.get_cov())
        Wa, Wb = np.zeros((B, d, d)), np.zeros((B, d, d))
        ra = a.minimize(Wa, 1.0, 1.0, 3e-4, 0.03, K, tol=-1.0, checkpoint=50)
        rb = b.minimize(Wb, 1.0, 1.0, 3e-4, 0.03, K, tol=-1.0, checkpoint=50)
        assert np.array_equal(Wa, Wb) and np.abs(Wa).max() > 0
        for x, y in zip(ra, rb):
            assert (x.iters, x.slots, x.status, x.halvings, x.early_stop, x.lr_final, x.obj_last, x.score_last,
                    x.h_last) == (y.iters, y.slots, y.status, y.halvings, y.early_stop, y.lr_final, y.obj_last,
                                  y.score_last, y.h_last)
            assert x.iters == K
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("data_seed", [0, 1, 2, 3])
def test_bootstrap_end_to_end_against_the_oracle(data_seed):
    """W_boot[b] against `LinearOracle.fit` on the gathered resample: identical support and
    max |dW| <= 1e-9, the project's GPU-to-oracle trajectory tolerance.  (On the CPU the oracle fed
    the two roundings of cov moves W by at most 3.6e-11 on these inputs; DESIGN.md records what the
    GPU gave.)"""
    X = make_dataset(20, 400, seed=data_seed)[0]
    X0 = X.copy()
    boot_seed, n_boot = 1234, 2
    m = DagmaLinearBatch()
    freq = m.bootstrap(X, n_boot, lambda1=0.03, seed=boot_seed, **dict(FIT_ARGS, s=list(FIT_ARGS["s"])))
    assert np.array_equal(X, X0)
    assert m.fit_timing["cov_on"] == "device" and m.boot_seed == boot_seed
    worst = 0.0
    for b in range(n_boot):
        o = LinearOracle("l2")
        W_ref = o.fit(X0[bootstrap_indices(boot_seed, b, 400)].copy(), lambda1=0.03,
                      **dict(FIT_ARGS, s=list(FIT_ARGS["s"])))
        assert np.array_equal(m.W_boot[b] != 0, W_ref != 0), b
        worst = max(worst, float(np.abs(m.W_boot[b] - W_ref).max()))
        print(f"  replicate {b}: h {m.h_final[b]:.3e} (oracle {o.h_final:.3e}), "
              f"score {m.score_final[b]:.12g} (oracle {o.score_final:.12g})")
    print(f"data seed {data_seed}: max |W_boot - W_oracle| = {worst:.3g}")
    assert worst <= 1e-9
    assert np.array_equal(freq, (m.W_boot != 0).mean(axis=0))


SHORT_ARGS = dict(T=2, s=[1.0, .9], warm_iter=100, max_iter=200, lr=0.3, checkpoint=50)


def test_bootstrap_with_more_replicates_than_compute_units():
    from midagma_amd.solver import HipBatch
    d, n, seed = 16, 64, 99
    X = make_dataset(d, n, seed=4)[0]
    m = DagmaLinearBatch()
    m.bootstrap(X, 300, lambda1=0.03, seed=seed, **dict(SHORT_ARGS, s=list(SHORT_ARGS["s"])))
    assert m.W_boot.shape == (300, d, d)
    for b in (0, 137, 299):
        class FromB(HipBatch):
            def boot_cov(self, X, seed, first=0, budget_bytes=None, _b=b):
                return super().boot_cov(X, seed, first=_b, budget_bytes=budget_bytes)

        one = DagmaLinearBatch(batch_factory=FromB)
        one.bootstrap(X, 1, lambda1=0.03, seed=seed, **dict(SHORT_ARGS, s=list(SHORT_ARGS["s"])))
        assert np.array_equal(one.cov[0], m.cov[b]), b
        assert np.array_equal(one.W_boot[0], m.W_boot[b]), b
        assert one.minimize_log[0][-1]["iters"] == m.minimize_log[b][-1]["iters"]


def test_boot_errors_and_lifetime():
    from midagma_amd.solver import HipBatch
    L = _lib.lib()
    gc.collect()
    base = L.midagma_debug_live_bytes()
    d, n = 20, 300
    X = _data(n, d, 8)
    m = DagmaLinearBatch()
    m.bootstrap(X, 4, lambda1=0.03, seed=1, **dict(SHORT_ARGS, s=list(SHORT_ARGS["s"])))
    assert L.midagma_debug_live_bytes() == base
    bt = HipBatch(d, 4, device=0)
    bt.boot_cov(X, 1)
    good = bt.get_cov()
    bad = X.copy()
    bad[17, 3] = np.nan
    live = L.midagma_debug_live_bytes()
    with pytest.raises(ValueError, match="infs or NaNs"):
        bt.boot_cov(bad, 1)
    assert L.midagma_debug_live_bytes() == live  # the scratch is freed on the error return
    with pytest.raises(ValueError, match="infs or NaNs"):
        bt.boot_cov(torch.from_numpy(bad).cuda(), 1)
    assert L.midagma_debug_live_bytes() == live
    assert np.array_equal(bt.get_cov(), good)  # the batch's cov is left as it was
    for args in ((0, d, 0), (2**31, d, 0), (n, d - 1, 0), (n, d, -1)):  # n, ldx, first
        assert L.midagma_boot_cov(bt.h, X.ctypes.data_as(C.c_void_p), args[0], args[1], 0, 1, args[2], 0) == _lib.E_ARG
    with pytest.raises(ValueError):
        bt.boot_cov(X[:, :d - 1], 1)
    bt.close()
    assert L.midagma_debug_live_bytes() == base
