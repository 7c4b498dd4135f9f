"""`DagmaLinearBatch`: many small-d DAGMA fits at once, one persistent workgroup per problem.

One l2 fit at d <= 64 runs its whole inner loop in one workgroup, on one compute unit of the
GPU.  Bootstrap resamples, a `lambda1` grid or a table over seeds and datasets are B such fits;
this class runs them as one batch (`HipBatch`, csrc/batch.hip) instead of a Python loop over
`DagmaLinear.fit`:

    W = DagmaLinearBatch().fit([X0, X1, ...], lambda1=0.03)        # (B, d, d)
    W = DagmaLinearBatch().fit(X, lambda1=[0.01, 0.03, 0.1])       # a lambda1 grid on one X

Problem b returns exactly (bit for bit) what `DagmaLinear("l2").fit(Xs[b].copy(), lambda1[b], ...)`
returns with the same arguments: the stages of the path-following loop (linear.py:441-453) run
in lockstep over the problems, and within a stage the problems that have not yet succeeded are
re-run, each with its own halved lr and enlarged s, until none is left.

The PST trek regularizer (seq exp or inv, d <= 32) runs inside each problem's workgroup
(csrc/pst_blk.h), with one pair set and a weight per problem, so the knob every PST user turns is a
grid like any other:

    m = DagmaLinearBatch(trek_reg=PSTRegularizer(I=I, seq="exp", mode="opt", weight=0.1))
    W = m.fit(X, lambda1=0.03, trek_weight=[0.01, 0.1, 1.0])       # a weight grid on one X

With a regularizer a problem's result does not depend on the rest of the batch, and it matches
`DagmaLinear(trek_reg=...).fit` (which runs the launch chain of csrc/trek.hip) to rounding along
the trajectory, not bit for bit.

Bootstrap edge frequencies come from one X, host or device, without B gathered copies of it:

    freq = DagmaLinearBatch().bootstrap(X, n_boot=1024, lambda1=0.03, seed=7)     # (d, d)

The device draws replicate b's row indices (`bootstrap_indices(seed, b, n)` restates the rule on
the host) and forms its covariance from counts over one pass of X (csrc/boot.hip), straight into
problem b of the batch; the stage and retry loop is `fit`'s.

`DagmaLogisticBatch` is the same batch for the reference's other loss, `DagmaLinear("logistic")`,
the one for binary data:

    W = DagmaLogisticBatch().fit([X0, X1, ...], lambda1=0.02)                 # (B, d, d)
    W = DagmaLogisticBatch().fit(X, lambda1=[0.005, 0.01, 0.02, 0.05])        # one X on the device, a grid

The logistic loss cannot fold n into a covariance: every Adam step needs X^T expit(X W).  Each
problem's workgroup streams its X through that step in row blocks on the FP64 matrix cores
(csrc/logit_blk.h, the logistic score phase); a shared X is stored once.  X is not centred
(linear.py:410 centres for l2 only).  A problem's result does not depend on the rest of the batch,
bit for bit, and matches `DagmaLinear("logistic").fit` (the large-tile launch chain) to rounding.

Not in the batch: the TCC trek regularizer, PST with seq log or binom or at d > 32, a pair set per
problem, float32 W, d > 64, the l2 loss in data mode, several devices, a device X in `fit`
(`bootstrap` takes one), weighted or m-out-of-n bootstraps.  Not in the logistic batch either: any
trek regularizer, a different n per problem, a bootstrap.
"""
from __future__ import annotations

import time
import typing

import numpy as np

from . import _lib
from .solver import HipBatch, HipSolver, is_device_tensor

__all__ = ["DagmaLinearBatch", "DagmaLogisticBatch", "bootstrap_indices"]

_M32 = np.uint64(0xFFFFFFFF)


def _philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """Philox4x32-10 (Salmon et al., SC'11) over arrays of counter words held in uint64; the four
    output words.  csrc/philox.h is the device's."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in (c0, c1, c2, c3))
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    sh = np.uint64(32)
    for r in range(10):
        ka, kb = np.uint64((k0 + r * 0x9E3779B9) & 0xFFFFFFFF), np.uint64((k1 + r * 0xBB67AE85) & 0xFFFFFFFF)
        p0, p1 = m0 * c0, m1 * c2  # 32 x 32 -> 64 bits, no overflow
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ ka, p1 & _M32, (p0 >> sh) ^ c3 ^ kb, p0 & _M32
    return c0, c1, c2, c3


def bootstrap_indices(seed: int, b: int, n: int) -> np.ndarray:
    """The n row indices (int64, in [0, n)) of bootstrap replicate `b` of `seed`, as the device draws
    them (csrc/boot.hip): o = Philox4x32-10(counter (j, b, 0, 0), key (seed & 0xffffffff, seed >> 32)),
    r = (o0 << 32) | o1, idx[j] = (r * n) >> 64.  `X[bootstrap_indices(seed, b, len(X))]` is the
    resample that replicate b of `DagmaLinearBatch.bootstrap(X, ..., seed=seed)` fits."""
    seed, b, n = int(seed) & (2**64 - 1), int(b), int(n)
    if not 1 <= n < 2**31:
        raise ValueError(f"bootstrap_indices needs 1 <= n < 2^31, got {n}")
    if not 0 <= b < 2**32:
        raise ValueError(f"bootstrap_indices needs 0 <= b < 2^32, got {b}")
    j = np.arange(n, dtype=np.uint64)
    zero = np.zeros(n, dtype=np.uint64)
    o0, o1, _, _ = _philox4x32_10(j, zero + np.uint64(b), zero, zero, seed & 0xFFFFFFFF, seed >> 32)
    # the high 64 bits of r * n with r = o0 2^32 + o1: (o0 n + ((o1 n) >> 32)) >> 32, all below 2^64
    nn, sh = np.uint64(n), np.uint64(32)
    return ((o0 * nn + ((o1 * nn) >> sh)) >> sh).astype(np.int64)


def _edges(edges):
    """(rows, cols) of a tuple of 2-tuples; anything else is ignored, as the reference ignores it
    (linear.py:416-426)."""
    if edges is not None and type(edges) is tuple and len(edges) > 0 and type(edges[0]) is tuple and \
            all(len(e) == 2 for e in edges):
        return tuple(zip(*edges))
    return None


class _BatchLoop:
    """What the batch classes share: the checked problem list, the masks and the lockstep stage and
    retry loop over a batch backend (`HipBatch`, or a test's CPU double)."""

    _MINIMIZE = "minimize"  # the backend method that runs one minimize call over the batch

    # ------------------------------------------------------------------ inputs
    def _problems(self, Xs, lambda1, trek_weight=None):
        """(list of B host X, B lambda1 values), checked; no device work."""
        def host2d(X):
            if is_device_tensor(X) or hasattr(X, "data_ptr"):
                raise ValueError(f"{type(self).__name__} takes host arrays, not device tensors")
            if not isinstance(X, np.ndarray) or X.dtype != np.float64 or X.ndim != 2:
                raise ValueError("every X must be a 2-d float64 host array (n x d)")
            return X

        lam_seq = None if np.ndim(lambda1) == 0 else [float(x) for x in lambda1]
        tw_len = None if trek_weight is None or np.ndim(trek_weight) == 0 else len(trek_weight)
        if lam_seq is not None and tw_len is not None and tw_len != len(lam_seq):
            raise ValueError(f"lambda1 holds {len(lam_seq)} values and trek_weight {tw_len}")
        if is_device_tensor(Xs) or hasattr(Xs, "data_ptr"):
            raise ValueError(f"{type(self).__name__} takes host arrays, not device tensors")
        if isinstance(Xs, np.ndarray) and Xs.ndim == 2:
            # one X: a lambda1 and / or trek_weight grid (X centred once, cov formed once, shared by
            # the problems)
            X = host2d(Xs)
            xs = [X] * (len(lam_seq) if lam_seq is not None else (tw_len if tw_len is not None else 1))
        elif isinstance(Xs, np.ndarray):
            if Xs.ndim != 3 or Xs.dtype != np.float64:
                raise ValueError("Xs must be a sequence of (n_b, d) float64 arrays, a (B, n, d) array or one (n, d) X")
            xs = [Xs[b] for b in range(Xs.shape[0])]
        else:
            xs = [host2d(X) for X in Xs]
        B = len(xs)
        if B == 0:
            raise ValueError("an empty batch")
        if B > HipBatch.MAX_B:
            raise ValueError(f"at most {HipBatch.MAX_B} problems in a batch, got {B}")
        ds = {int(X.shape[1]) for X in xs}
        if len(ds) != 1:
            raise ValueError(f"the problems must share d, got {sorted(ds)}")
        d = ds.pop()
        if d < 1 or d > HipBatch.MAX_D:
            raise ValueError(f"{type(self).__name__} needs 1 <= d <= {HipBatch.MAX_D}, got d = {d}")
        if any(X.shape[0] < 1 for X in xs):
            raise ValueError("every X needs at least one row")
        if lam_seq is None:
            lam_seq = [lambda1] * B
        elif len(lam_seq) != B:
            raise ValueError(f"lambda1 holds {len(lam_seq)} values for {B} problems")
        return xs, lam_seq, d

    def _masks(self, mu: float, lam, inc, exc, B: int, d: int):
        """linear.py:217-222 per problem (mask_inc depends on the problem's lambda1)."""
        mask_inc = mask_exc = None
        if inc is not None:
            mask_inc = np.zeros((B, d, d))
            for b in range(B):
                mask_inc[b][inc[0], inc[1]] = -2 * mu * lam[b]
        if exc is not None:
            mask_exc = np.ones((B, d, d))
            mask_exc[:, exc[0], exc[1]] = 0.
        return mask_inc, mask_exc

    # ------------------------------------------------- the loop of fit and bootstrap
    @staticmethod
    def _s_list(s, T: int):
        if isinstance(s, (list, tuple)):
            return list(s) + max(0, T - len(s)) * [s[-1]]  # linear.py:431-434
        if type(s) in (int, float):
            return T * [s]
        raise ValueError("s should be a list, int, or float.")

    def _stages(self, batch, B, d, lam, T, s0, inc, exc, mu_init, mu_factor, warm_iter, max_iter, lr, checkpoint,
                beta_1, beta_2):
        """The path-following loop (linear.py:441-453) over a batch whose cov is set: the stages in
        lockstep, within a stage every problem that has not yet succeeded re-run with its own
        halved lr and enlarged s.  Leaves W_est (unthresholded) and minimize_log."""
        self.W_est = np.zeros((B, d, d))
        self.minimize_log = [[] for _ in range(B)]
        s_of = [list(s0) for _ in range(B)]  # each problem enlarges its own s on a failure
        mu = mu_init
        for i in range(T):
            self.vprint(f'\nIteration -- {i+1}:')
            inner_iters = int(max_iter) if i == T - 1 else int(warm_iter)
            lr_of = [lr] * B
            todo = np.ones(B, dtype=bool)
            batch.set_masks(*self._masks(mu, lam, inc, exc, B, d))
            while todo.any():
                t0 = time.time()
                W_try = self.W_est.copy()
                s_now = [s_of[b][i] for b in range(B)]
                res = getattr(batch, self._MINIMIZE)(W_try, mu, s_now, lr_of, lam, inner_iters, beta_1=beta_1, beta_2=beta_2,
                                     checkpoint=checkpoint, active=todo)
                seconds = time.time() - t0
                singular = [b for b in np.flatnonzero(todo) if res[b].status == _lib.ST_SINGULAR]
                if singular:
                    raise np.linalg.LinAlgError(
                        f"singular matrix: inverse of sI - W*W is not finite in problems {singular}")
                for b in np.flatnonzero(todo):
                    r = res[b]
                    self.minimize_log[b].append(dict(mu=mu, s=s_now[b], lr=lr_of[b], max_iter=inner_iters,
                                                     iters=r.iters, success=r.success, early_stop=r.early_stop,
                                                     halvings=r.halvings, seconds=seconds))
                    if r.success:
                        self.W_est[b] = W_try[b]
                        todo[b] = False
                    else:  # this problem alone: a smaller lr and a larger s (linear.py:449-452)
                        self.vprint(f'problem {b}: W went out of domain for s={s_now[b]} at iteration '
                                    f'{r.iters + 1}; retrying with larger s')
                        lr_of[b] *= 0.5
                        s_of[b][i] += 0.1
            mu *= mu_factor


class DagmaLinearBatch(_BatchLoop):
    """B independent `DagmaLinear('l2')` fits with a common d <= 64 on one GPU."""

    def __init__(self, loss_type: str = "l2", verbose: bool = False, dtype: type = np.float64, *,
                 device: int | None = None, trek_reg=None, batch_factory=None, solver_factory=None) -> None:
        if loss_type != "l2":
            raise ValueError("DagmaLinearBatch runs the l2 loss (cov mode) only; DagmaLogisticBatch runs the "
                             "logistic loss")
        if np.dtype(dtype).type is not np.float64:
            raise ValueError("DagmaLinearBatch runs a float64 W only")
        self._trek = self._read_trek(trek_reg)
        self.loss_type = loss_type
        self.dtype = np.float64
        self.vprint = print if verbose else (lambda *a, **k: None)
        self.device = 0 if device is None else int(device)
        # the backends (tests pass CPU doubles): the batch, and one ordinary solver for h / score
        self._batch_factory = batch_factory or HipBatch
        self._solver_factory = solver_factory or HipSolver
        self.minimize_log: list = []

    # -------------------------------------------------------- trek regularizer
    @staticmethod
    def _read_trek(tr):
        """The PST settings of an enabled regularizer, read as `DagmaLinear._install_trek` reads them
        (None: no regularizer); everything the batch does not run raises."""
        if tr is None or not tr.enabled():
            return None
        if str(tr.name).lower().strip() != "pst":
            raise ValueError(f"DagmaLinearBatch runs the PST trek regularizer only, not {tr.name!r}")
        pairs = tr.cfg.get("I")
        if pairs is None or len(pairs) == 0:
            return None  # (an empty pair set is no regularizer, as in the reference)
        kw = dict(tr.cfg.get("kwargs") or {})
        seq = str(tr.cfg.get("seq", "exp")).lower().strip()
        if seq not in ("exp", "inv"):
            raise ValueError(f"DagmaLinearBatch runs PST with seq 'exp' or 'inv', not {seq!r}")
        if kw.get("K_log") is not None:
            raise ValueError("DagmaLinearBatch runs no log series (K_log)")
        return dict(pairs=np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2)), seq=seq,
                    agg=kw.get("agg", "mean"), mode=tr.mode, weight=float(tr.weight),
                    eps_inv=kw.get("eps_inv", 1e-8))

    def _trek_weights(self, trek_weight, B: int, d: int):
        """The B weights of the regularizer (None without one); no device work."""
        if self._trek is None:
            if trek_weight is not None:
                raise ValueError("trek_weight needs a trek regularizer")
            return None
        if d > HipBatch.MAX_D_TREK:
            raise ValueError(f"DagmaLinearBatch runs a trek regularizer at d <= {HipBatch.MAX_D_TREK}, got d = {d}")
        if trek_weight is None:
            return [self._trek["weight"]] * B
        if np.ndim(trek_weight) == 0:
            return [float(trek_weight)] * B
        w = [float(x) for x in trek_weight]
        if len(w) != B:
            raise ValueError(f"trek_weight holds {len(w)} values for {B} problems")
        return w

    def _install_trek(self, batch, weights):
        if self._trek is not None:
            t = self._trek
            batch.set_trek(t["pairs"], t["seq"], agg=t["agg"], mode=t["mode"], weight=weights, eps_inv=t["eps_inv"])

    def _trek_final(self, batch, B):
        """The PST value at every unthresholded W_est (zeros without a regularizer)."""
        self.trek_final = np.zeros(B) if self._trek is None else np.asarray(batch.trek_value(self.W_est, grad=False)[0])

    def _finals(self, B, d):
        """h and the score of every problem's W_est on self.cov[b], from one ordinary solver: the
        kernels of the single fit."""
        self.h_final, self.score_final = np.empty(B), np.empty(B)
        solver = self._solver_factory(d, "l2", "cov", device=self.device)
        try:
            last = None
            for b in range(B):
                if self.cov[b] is not last:
                    solver.set_cov(self.cov[b])
                    last = self.cov[b]
                self.h_final[b], _ = solver.h_value(self.W_est[b], 1.0, grad=True)
                self.score_final[b], _ = solver.score_value(self.W_est[b])
        finally:
            solver.close()

    # --------------------------------------------------------------- bootstrap
    _FIT_DEFAULTS = dict(w_threshold=0.3, T=5, mu_init=1.0, mu_factor=0.1, s=[1.0, .9, .8, .7, .6], warm_iter=3e4,
                         max_iter=6e4, lr=0.0003, checkpoint=1000, beta_1=0.99, beta_2=0.999, exclude_edges=None,
                         include_edges=None)

    def bootstrap(self, X, n_boot: int, lambda1: float = 0.03, seed: int = 0, trek_weight=None,
                  **fit_kwargs) -> np.ndarray:
        """Edge frequencies over `n_boot` bootstrap resamples of one X, the resampling and the
        covariances on the device (`HipBatch.boot_cov`, csrc/boot.hip).

        X: one (n, d) float64 host array or device tensor, d <= 64; it is not modified.  Replicate
        b fits the rows `X[bootstrap_indices(seed, b, n)]`, so `DagmaLinear('l2').fit(X[idx].copy(),
        lambda1, ...)` reproduces any one of them (up to the rounding of its covariance).  lambda1:
        a scalar.  trek_weight: a scalar that replaces the trek regularizer's weight (None: its own).
        fit_kwargs: `fit`'s other arguments, with its defaults.

        Leaves W_boot (n_boot, d, d; thresholded), edge_freq = (W_boot != 0).mean(0) (also
        returned), boot_seed, and h_final, score_final, trek_final, minimize_log and fit_timing as
        `fit`."""
        t_start = time.perf_counter()
        unknown = sorted(set(fit_kwargs) - set(self._FIT_DEFAULTS))
        if unknown:
            raise TypeError(f"bootstrap got unexpected arguments {unknown}")
        kw = dict(self._FIT_DEFAULTS, **fit_kwargs)
        if np.ndim(lambda1) != 0:
            raise ValueError("bootstrap takes one scalar lambda1")
        if trek_weight is not None and np.ndim(trek_weight) != 0:
            raise ValueError("bootstrap takes one scalar trek_weight")
        if isinstance(n_boot, bool) or int(n_boot) != n_boot or not 1 <= int(n_boot) <= HipBatch.MAX_B:
            raise ValueError(f"bootstrap needs 1 <= n_boot <= {HipBatch.MAX_B}, got {n_boot}")
        if is_device_tensor(X):
            import torch
            if X.dim() != 2 or X.dtype != torch.float64 or X.stride(1) != 1:
                raise ValueError("X must be a 2-d float64 tensor (n x d) with unit column stride")
        elif hasattr(X, "data_ptr") or not isinstance(X, np.ndarray) or X.dtype != np.float64 or X.ndim != 2:
            raise ValueError("X must be one 2-d float64 host array or device tensor (n x d)")
        elif X.strides[1] != 8:
            X = np.ascontiguousarray(X)
        n, d = int(X.shape[0]), int(X.shape[1])
        if d < 1 or d > HipBatch.MAX_D:
            raise ValueError(f"DagmaLinearBatch needs 1 <= d <= {HipBatch.MAX_D}, got d = {d}")
        if n < 1 or n >= 2**31:
            raise ValueError(f"bootstrap needs 1 <= n < 2^31 rows, got {n}")
        B, T, lam = int(n_boot), int(kw["T"]), [float(lambda1)] * int(n_boot)
        tw = self._trek_weights(trek_weight, B, d)
        s0 = self._s_list(kw["s"], T)
        inc, exc = _edges(kw["include_edges"]), _edges(kw["exclude_edges"])
        self.B, self.d, self.lambda1, self.checkpoint, self.boot_seed = B, d, lam, kw["checkpoint"], int(seed)
        batch = self._batch_factory(d, B, device=self.device)
        try:
            batch.boot_cov(X, int(seed))
            self._install_trek(batch, tw)
            t_prep = time.perf_counter()
            self._stages(batch, B, d, lam, T, s0, inc, exc, kw["mu_init"], kw["mu_factor"], kw["warm_iter"],
                         kw["max_iter"], kw["lr"], kw["checkpoint"], kw["beta_1"], kw["beta_2"])
            covs = batch.get_cov()
            self._trek_final(batch, B)
        finally:
            batch.close()
        t_loop = time.perf_counter()
        self.cov = [covs[b] for b in range(B)]
        self._finals(B, d)
        self.fit_timing = dict(prep_s=t_prep - t_start, loop_s=t_loop - t_prep,
                               final_s=time.perf_counter() - t_loop, cov_on="device")
        self.W_est[np.abs(self.W_est) < kw["w_threshold"]] = 0
        self.W_boot = self.W_est
        self.edge_freq = (self.W_boot != 0).mean(axis=0)
        return self.edge_freq

    # --------------------------------------------------------------------- fit
    def fit(self, Xs, lambda1: typing.Union[float, typing.Sequence[float]] = 0.03, w_threshold: float = 0.3,
            T: int = 5, mu_init: float = 1.0, mu_factor: float = 0.1,
            s: typing.Union[typing.List[float], float] = [1.0, .9, .8, .7, .6],
            warm_iter: int = 3e4, max_iter: int = 6e4, lr: float = 0.0003, checkpoint: int = 1000,
            beta_1: float = 0.99, beta_2: float = 0.999,
            exclude_edges: typing.Optional[typing.Tuple[typing.Tuple[int, int], ...]] = None,
            include_edges: typing.Optional[typing.Tuple[typing.Tuple[int, int], ...]] = None,
            trek_weight: typing.Union[None, float, typing.Sequence[float]] = None) -> np.ndarray:
        """Runs DAGMA (linear.py:335-462) on every problem and returns the thresholded weighted
        adjacencies, (B, d, d).

        Xs: a sequence of B host float64 arrays (n_b, d) with a common d (the n_b may differ), a
        (B, n, d) array, or one (n, d) X with `lambda1` a length-B sequence (a lambda1 grid).
        lambda1: a scalar or a length-B sequence.  trek_weight: a scalar or a length-B sequence that
        replaces the trek regularizer's weight per problem (None: its own); one X with a
        `trek_weight` sequence is a weight grid, and with both sequences given their lengths must
        agree.  The other arguments are `DagmaLinear.fit`'s and shared by the problems.  Every
        distinct X is centred in place, once, as the reference centres its X; the caller's `s` list
        is not changed.

        Leaves W_est (B, d, d), h_final (B,), score_final (B,), trek_final (B,; the PST value at the
        unthresholded W_est, zeros without a regularizer), minimize_log (B lists with
        `DagmaLinear.minimize_log`'s fields) and fit_timing.  Raises np.linalg.LinAlgError naming
        the problems whose s I - W o W became singular."""
        t_start = time.perf_counter()
        xs, lam, d = self._problems(Xs, lambda1, trek_weight)
        B, T = len(xs), int(T)
        tw = self._trek_weights(trek_weight, B, d)
        s0 = self._s_list(s, T)
        inc, exc = _edges(include_edges), _edges(exclude_edges)
        self.B, self.d, self.lambda1, self.checkpoint = B, d, lam, checkpoint
        # centring and cov = X^T X / n on the host, once per distinct X (linear.py:411, 428)
        covs: dict = {}
        for X in xs:
            if id(X) not in covs:
                X -= X.mean(axis=0, keepdims=True)
                covs[id(X)] = X.T @ X / float(X.shape[0])
        self.cov = [covs[id(X)] for X in xs]
        batch = self._batch_factory(d, B, device=self.device)
        try:
            batch.set_cov(np.stack(self.cov))
            self._install_trek(batch, tw)
            t_prep = time.perf_counter()
            self._stages(batch, B, d, lam, T, s0, inc, exc, mu_init, mu_factor, warm_iter, max_iter, lr, checkpoint,
                         beta_1, beta_2)
            self._trek_final(batch, B)
        finally:
            batch.close()
        t_loop = time.perf_counter()
        self._finals(B, d)
        self.fit_timing = dict(prep_s=t_prep - t_start, loop_s=t_loop - t_prep,
                               final_s=time.perf_counter() - t_loop, cov_on="host")
        self.W_est[np.abs(self.W_est) < w_threshold] = 0
        return self.W_est


class DagmaLogisticBatch(_BatchLoop):
    """B independent `DagmaLinear('logistic')` fits with a common n and d <= 64 on one GPU."""

    _MINIMIZE = "minimize_logistic"

    def __init__(self, verbose: bool = False, dtype: type = np.float64, *, device: int | None = None,
                 trek_reg=None, batch_factory=None, solver_factory=None) -> None:
        if np.dtype(dtype).type is not np.float64:
            raise ValueError("DagmaLogisticBatch runs a float64 W only")
        if trek_reg is not None and trek_reg.enabled():
            raise ValueError("DagmaLogisticBatch runs no trek regularizer")
        self.loss_type = "logistic"
        self.dtype = np.float64
        self.vprint = print if verbose else (lambda *a, **k: None)
        self.device = 0 if device is None else int(device)
        # the backends (tests pass CPU doubles): the batch, and one ordinary solver for h
        self._batch_factory = batch_factory or HipBatch
        self._solver_factory = solver_factory or HipSolver
        self.minimize_log: list = []

    def fit(self, Xs, lambda1: typing.Union[float, typing.Sequence[float]] = 0.03, w_threshold: float = 0.3,
            T: int = 5, mu_init: float = 1.0, mu_factor: float = 0.1,
            s: typing.Union[typing.List[float], float] = [1.0, .9, .8, .7, .6],
            warm_iter: int = 3e4, max_iter: int = 6e4, lr: float = 0.0003, checkpoint: int = 1000,
            beta_1: float = 0.99, beta_2: float = 0.999,
            exclude_edges: typing.Optional[typing.Tuple[typing.Tuple[int, int], ...]] = None,
            include_edges: typing.Optional[typing.Tuple[typing.Tuple[int, int], ...]] = None) -> np.ndarray:
        """Runs DAGMA with the logistic loss (linear.py:335-462) on every problem and returns the
        thresholded weighted adjacencies, (B, d, d).

        Xs: a sequence of B host float64 arrays (n, d) with a common n and d, a (B, n, d) array, or
        one (n, d) X with `lambda1` a length-B sequence (a lambda1 grid: X is stored once on the
        device and every problem reads it).  X is neither centred nor written.  The other
        arguments are `DagmaLinear.fit`'s and shared by the problems; the caller's `s` list is not
        changed.

        Leaves W_est (B, d, d), W_unthresholded (its values before the threshold), h_final (B,),
        score_final (B,; the logistic loss of the unthresholded W_est, from the batch's own
        row-block kernel), minimize_log (B lists with
        `DagmaLinear.minimize_log`'s fields) and fit_timing.  Raises ValueError, before any device
        work, for Xs of different n, d > 64, a device tensor or a non-float64 X, and
        np.linalg.LinAlgError naming the problems whose s I - W o W became singular."""
        t_start = time.perf_counter()
        xs, lam, d = self._problems(Xs, lambda1)
        ns = {int(X.shape[0]) for X in xs}
        if len(ns) != 1:
            raise ValueError(f"DagmaLogisticBatch needs one n for all problems, got {sorted(ns)}")
        B, T = len(xs), int(T)
        s0 = self._s_list(s, T)
        inc, exc = _edges(include_edges), _edges(exclude_edges)
        self.B, self.d, self.lambda1, self.checkpoint = B, d, lam, checkpoint
        shared = all(X is xs[0] for X in xs)
        # cov = X^T X / n of the uncentred X, once per distinct X (linear.py:428)
        covs: dict = {}
        for X in xs:
            if id(X) not in covs:
                covs[id(X)] = X.T @ X / float(X.shape[0])
        self.cov = [covs[id(X)] for X in xs]
        batch = self._batch_factory(d, B, device=self.device)
        try:
            batch.set_cov(np.stack(self.cov))
            batch.set_data(xs[0] if shared else np.stack(xs), shared=shared)
            t_prep = time.perf_counter()
            self._stages(batch, B, d, lam, T, s0, inc, exc, mu_init, mu_factor, warm_iter, max_iter, lr, checkpoint,
                         beta_1, beta_2)
            self.score_final = np.asarray(batch.score_logistic(self.W_est, grad=False)[0], dtype=np.float64)
        finally:
            batch.close()
        t_loop = time.perf_counter()
        self.h_final = np.empty(B)
        solver = self._solver_factory(d, "l2", "cov", device=self.device)  # (h does not read the loss)
        try:
            for b in range(B):
                self.h_final[b], _ = solver.h_value(self.W_est[b], 1.0, grad=True)
        finally:
            solver.close()
        self.fit_timing = dict(prep_s=t_prep - t_start, loop_s=t_loop - t_prep,
                               final_s=time.perf_counter() - t_loop, cov_on="host")
        self.W_unthresholded = self.W_est.copy()
        self.W_est[np.abs(self.W_est) < w_threshold] = 0
        return self.W_est
