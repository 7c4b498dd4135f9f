"""Python handle over the C ABI: one `HipSolver` per (fit, device).

`HipSolver.minimize` is the single-process hot path (the whole inner loop runs
on the GPU from replayed hipGraphs).  `run_allreduce_minimize` is the
multi-rank data-parallel loop: every step the GPU computes this rank's score
partial Z_k = X_k^T(...), the caller's all-reduce sums it over ranks
(torch.distributed -> RCCL over xGMI), and the GPU finishes the step.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import check, dptr

__all__ = ["HipSolver", "HipGroup", "HipIndep", "HipBatch", "MinimizeResult", "CheckpointRecord", "run_allreduce_minimize",
           "device_count", "colsum_dev", "center_dev", "gram", "row_range", "column_ranks", "correlation"]


CheckpointRecord = namedtuple("CheckpointRecord", [f for f, _ in _lib.MidagmaCkpt._fields_])


@dataclass
class MinimizeResult:
    iters: int
    success: bool
    status: int
    halvings: int
    early_stop: bool
    lr_final: float
    slots: int
    obj_last: float
    score_last: float
    h_last: float
    checkpoints: list = field(default_factory=list)

    @classmethod
    def from_c(cls, r: _lib.MidagmaResult, ckpts=()):
        return cls(iters=int(r.iters), success=r.status != _lib.ST_FAILED, status=int(r.status),
                   halvings=int(r.halvings), early_stop=bool(r.early_stop), lr_final=float(r.lr_final),
                   slots=int(r.slots), obj_last=float(r.obj_last), score_last=float(r.score_last),
                   h_last=float(r.h_last), checkpoints=list(ckpts))


def device_count() -> int:
    n = C.c_int(0)
    check(_lib.lib().midagma_device_count(C.byref(n)), None, "device_count")
    return int(n.value)


def _as_f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def is_device_tensor(X) -> bool:
    """True for a torch CUDA (HIP) tensor."""
    return hasattr(X, "data_ptr") and getattr(getattr(X, "device", None), "type", None) == "cuda"


def _rows(X):
    """(n, d, ld) of a row-major float64 matrix (host ndarray or device tensor)."""
    if hasattr(X, "data_ptr"):
        import torch
        if X.dtype != torch.float64 or X.dim() != 2 or X.stride(1) != 1:
            raise ValueError("X must be a 2-d float64 tensor with unit column stride")
        return int(X.shape[0]), int(X.shape[1]), int(X.stride(0))
    if X.dtype != np.float64 or X.ndim != 2 or X.strides[1] != 8:
        raise ValueError("X must be a 2-d float64 array with unit column stride")
    return int(X.shape[0]), int(X.shape[1]), int(X.strides[0] // 8)


def _cur_stream(dev):
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def colsum_dev(X):
    """Column sums of a device X (fixed order; `X.mean(axis=0)` of linear.py:411 is this / n),
    on torch's current stream.  Returns a float64 device tensor of length d."""
    import torch
    n, d, ld = _rows(X)
    out = torch.empty(d, dtype=torch.float64, device=X.device)
    with torch.cuda.device(X.device):  # (the library's scratch on X's device, not the current one)
        check(_lib.lib().midagma_colsum_dev(C.c_void_p(X.data_ptr()), n, d, ld, C.c_void_p(out.data_ptr()),
                                            _cur_stream(X.device)), None, "colsum_dev")
    return out


def center_dev(X, colsum, nrows: float):
    """X -= colsum / nrows in place on the device (the l2 centring, linear.py:411)."""
    import torch
    n, d, ld = _rows(X)
    assert colsum.numel() == d and colsum.device == X.device
    with torch.cuda.device(X.device):
        check(_lib.lib().midagma_center_dev(C.c_void_p(X.data_ptr()), n, d, ld, C.c_void_p(colsum.data_ptr()),
                                            float(nrows), _cur_stream(X.device)), None, "center_dev")


def gram(X, device: int | None = None):
    """G = X^T X (linear.py:428 before the division) on the GPU, for X on the device or on the
    host (streamed through the device in row chunks).  Returns a d x d float64 device tensor."""
    import torch
    n, d, ld = _rows(X)
    on_dev = is_device_tensor(X)
    dev = X.device if on_dev else torch.device("cuda", 0 if device is None else device)
    G = torch.empty((d, d), dtype=torch.float64, device=dev)
    src = C.c_void_p(X.data_ptr()) if on_dev else X.ctypes.data_as(C.c_void_p)
    with torch.cuda.device(dev):
        check(_lib.lib().midagma_gram(src, n, d, ld, 1 if on_dev else 0, C.c_void_p(G.data_ptr()), d,
                                      _cur_stream(dev)), None, "gram")
    return G


def _check_shape(shape, what: str, max_n):
    if len(shape) != 2:
        raise ValueError(f"{what}: X must be 2-d (n samples x d variables)")
    n, d = int(shape[0]), int(shape[1])
    if max_n is not None and not 2 <= n <= max_n:
        raise ValueError(f"{what}: need 2 <= n <= {max_n} samples, got {n}")
    if n < 2 or d < 1:
        raise ValueError(f"{what}: need at least 2 samples and 1 variable")


def _device_x(X, what: str, max_n: int | None = None):
    """A device X checked (a 2-d float64 tensor, n >= 2 samples, at most max_n, of d >= 1 variables)
    and returned with unit column stride: as it is, anything else through `.contiguous()`.  The
    library looks for inf and nan on the device."""
    import torch
    if X.dtype != torch.float64:
        raise ValueError(f"{what}: a device tensor X must be float64")
    _check_shape(X.shape, what, max_n)
    if X.stride(1) != 1 or X.stride(0) < X.shape[1]:
        X = X.contiguous()
    return X


def _host_x(X, what: str, max_n: int | None = None, copy: bool = False):
    """A host X as a C-contiguous float64 array (copy=True: always a copy, so the caller's X is
    never touched; else a view where X already is one), checked as `_device_x` and for inf and nan."""
    X = np.array(X, dtype=np.float64, order="C", copy=True) if copy else _as_f64(X)
    _check_shape(X.shape, what, max_n)
    if not np.isfinite(X).all():
        raise ValueError(f"{what}: X holds inf or nan")
    return X


def _device_matrix(X, what: str, device=None):
    """X as a 2-d float64 CUDA tensor with unit column stride: a device tensor as it is (checked),
    a host float64 array uploaded with torch (to `device`; None: torch's current device).  No GPU:
    HipSolverError (there is no CPU path)."""
    import torch
    if is_device_tensor(X):
        return _device_x(X, what)
    if hasattr(X, "data_ptr"):  # a host torch tensor
        X = X.detach().numpy()
    X = np.asarray(X)
    if X.dtype != np.float64:
        raise ValueError(f"{what}: X must be float64, got {X.dtype}")
    X = _host_x(X, what)
    _lib.lib()
    if not torch.cuda.is_available():
        raise _lib.HipSolverError(f"{what}: no GPU (there is no CPU path)")
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    return torch.from_numpy(X).to(dev)


def column_ranks(X, budget_bytes: int = 0):
    """The 1-based average-tie ranks of every column of X (`scipy.stats.rankdata(method="average")`
    per column, bit for bit) as an n x d float64 device tensor, by csrc/corr.hip's batched radix
    sort.  X: a float64 CUDA tensor with unit column stride (any row stride), read in place on
    torch's current stream and never written, or a host float64 array (uploaded with torch).
    budget_bytes: the sort's scratch per chunk of columns (0: the library's default); the ranks do
    not depend on it.  ValueError when X holds inf or nan."""
    import torch
    X = _device_matrix(X, "column_ranks")
    n, d, ld = _rows(X)
    R = torch.empty((n, d), dtype=torch.float64, device=X.device)
    with torch.cuda.device(X.device):
        check(_lib.lib().midagma_colrank(C.c_void_p(X.data_ptr()), n, d, ld, C.c_void_p(R.data_ptr()), d,
                                         int(budget_bytes), _cur_stream(X.device)), None, "column_ranks")
    return R


def correlation(X, *, ranks: bool = False, budget_bytes: int = 0):
    """(Rho, const): the d x d Pearson correlation matrix of X's columns (float64 device tensor;
    1 on the diagonal, NaN in the rows and columns of constant columns) and a d-element bool array
    that marks the constant columns (max == min).  ranks=True: Spearman's rho, the same on
    `column_ranks(X)`.  X and budget_bytes as in `column_ranks`."""
    import torch
    X = _device_matrix(X, "correlation")
    if ranks:
        X = column_ranks(X, budget_bytes)
    n, d, ld = _rows(X)
    Rho = torch.empty((d, d), dtype=torch.float64, device=X.device)
    const = torch.empty(d, dtype=torch.int32, device=X.device)
    with torch.cuda.device(X.device):
        check(_lib.lib().midagma_corr(C.c_void_p(X.data_ptr()), n, d, ld, C.c_void_p(Rho.data_ptr()), d,
                                      C.c_void_p(const.data_ptr()), int(budget_bytes), _cur_stream(X.device)),
              None, "correlation")
    return Rho, const.cpu().numpy().astype(bool)


class _Handle:
    """A handle of one family of the C ABI.  A subclass names the family once (its `*_destroy` and
    `*_last_error` symbols) and sets self.L and self.h; it inherits close, __del__ and _check."""

    _destroy = _last_error = ""
    L = h = None

    def _check(self, rc, handle, what):
        """Raise for a negative rc with the family's message: of `handle`, or (None) the family's
        last message of this thread raised without one."""
        return check(rc, handle, what, getattr(self.L, self._last_error))

    def close(self):
        if self.h:
            getattr(self.L, self._destroy)(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class HipSolver(_Handle):
    """Owns device buffers for one d and one score mode on one GPU."""

    _destroy, _last_error = "midagma_destroy", "midagma_last_error"

    def __init__(self, d: int, loss: str = "l2", mode: str = "cov", device: int = 0, stream: int | None = None,
                 _handle=None):
        self.L = _lib.lib()
        self.d = int(d)
        self.loss = loss
        self.mode = mode
        lt = {"l2": _lib.LOSS_L2, "logistic": _lib.LOSS_LOGISTIC}[loss]
        md = {"cov": _lib.MODE_COV, "data": _lib.MODE_DATA}[mode]
        # _handle: a solver owned by something else (a HipGroup's member); never destroyed here
        self._owned = _handle is None
        if _handle is None:
            h = C.c_void_p()
            check(self.L.midagma_create(C.byref(h), lt, md, self.d, int(device), stream), None, "midagma_create")
        else:
            h = C.c_void_p(_handle)
        self.h = h
        self.device = device
        self.D = int(self.L.midagma_padded_dim(self.h))

    def close(self):
        if not getattr(self, "_owned", True):
            self.h = None
        super().close()

    @property
    def stream(self) -> int:
        return int(self.L.midagma_stream(self.h) or 0)

    # -- data -----------------------------------------------------------------
    def set_cov(self, cov: np.ndarray):
        cov = _as_f64(cov)
        check(self.L.midagma_set_cov(self.h, dptr(cov), cov.shape[1]), self.h, "set_cov")

    def set_w_float32(self, on: bool):
        """W's dtype in the reference's arithmetic for the next minimize (ABI 8): True emulates
        numpy's float32 operations on a float32 W (linear.py:29, 226, 244, 248, 275)."""
        check(self.L.midagma_set_w_float32(self.h, 1 if on else 0), self.h, "set_w_float32")

    def set_masks(self, mask_inc: np.ndarray | None, mask_exc: np.ndarray | None):
        mi = None if mask_inc is None else _as_f64(mask_inc)
        me = None if mask_exc is None else _as_f64(mask_exc)
        check(self.L.midagma_set_masks(self.h, dptr(mi), dptr(me)), self.h, "set_masks")

    TREK_SEQ = {"exp": 0, "inv": 1, "log": 2, "binom": 3}
    TREK_AGG = {"mean": 0, "sum": 1, "max": 2, "lse": 3}
    TREK_MODE = {"off": 0, "log": 1, "opt": 2}

    def set_trek(self, pairs, seq: str = "exp", *, agg: str = "mean", mode: str = "opt", weight: float = 0.0,
                 eps_inv: float = 1e-8, K_log: int | None = None):
        """The PST trek regularizer (notreks.pst) inside the loop; mode 'off' or no pairs disables it."""
        P = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2)) if pairs is not None \
            else np.zeros((0, 2), dtype=np.int64)
        seq, agg, mode = seq.lower().strip(), agg.lower().strip(), mode.lower().strip()
        if seq not in self.TREK_SEQ or agg not in self.TREK_AGG or mode not in self.TREK_MODE:
            raise ValueError(f"unsupported PST configuration seq={seq!r} agg={agg!r} mode={mode!r}")
        K = 2 * self.d if K_log is None else int(K_log)
        check(self.L.midagma_set_trek(self.h, self.TREK_SEQ[seq], self.TREK_AGG[agg], self.TREK_MODE[mode],
                                      float(weight), float(eps_inv), K, P.ctypes.data_as(C.POINTER(C.c_int64)),
                                      int(P.shape[0])), self.h, "set_trek")

    def set_trek_tcc(self, pairs, *, mode: str = "opt", weight: float = 0.0, w: float = 1.0, eps: float = 1e-12):
        """The TCC trek regularizer as the reference's loop runs it (trek_value_grad -> spectral,
        'approx_trek_graph'); mode 'off' or no pairs disables it."""
        P = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2)) if pairs is not None \
            else np.zeros((0, 2), dtype=np.int64)
        mode = mode.lower().strip()
        if mode not in self.TREK_MODE:
            raise ValueError(f"unsupported TCC mode {mode!r}")
        check(self.L.midagma_set_trek_tcc(self.h, self.TREK_MODE[mode], float(weight), float(w), float(eps),
                                          P.ctypes.data_as(C.POINTER(C.c_int64)), int(P.shape[0])), self.h,
              "set_trek_tcc")

    def trek_value(self, W: np.ndarray, grad: bool = True):
        """notreks.trek_value_grad(W, tr) for the configured regularizer: (value, grad or None)."""
        W = _as_f64(W)
        v = C.c_double()
        G = np.empty((self.d, self.d)) if grad else None
        check(self.L.midagma_trek(self.h, dptr(W), C.byref(v), dptr(G)), self.h, "trek")
        return float(v.value), G

    def set_data(self, X, n_global: int | None = None):
        """X: host ndarray (n_local x d) or a torch CUDA tensor (copied)."""
        if hasattr(X, "data_ptr"):
            X = X.contiguous()
            n_local = X.shape[0]
            check(self.L.midagma_set_data(self.h, C.c_void_p(X.data_ptr()), n_local, int(n_global or n_local), 1),
                  self.h, "set_data")
            self._keep = X
        else:
            X = _as_f64(X)
            n_local = X.shape[0]
            check(self.L.midagma_set_data(self.h, X.ctypes.data_as(C.c_void_p), n_local,
                                          int(n_global or n_local), 0), self.h, "set_data")

    def debug_sig_split(self, mode: int | None = None) -> int:
        """Test hook (not part of the public header): the logistic sigmoid GEMM's form for the
        next set_data (None: leave it; 0: the size rule, 1: the one-pass kernel, 2: the serial K
        split wherever the shape allows).  Returns the form the current data uses (1 or 2)."""
        fn = self.L.midagma_debug_sig_split
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
        cur = fn(self.h, -1)
        if mode is not None and fn(self.h, int(mode)) < 0:
            raise ValueError(f"debug_sig_split: bad mode {mode!r}")
        return int(cur)

    @property
    def xty_form(self) -> int:
        """The form of the data-mode X^T Y GEMM the current data uses: 1 the classical split-K
        GEMM, 2 one level of Strassen (0: no data set)."""
        return int(self.L.midagma_xty_form(self.h))

    def debug_xty_form(self, mode: int | None = None, split: int | None = None) -> int:
        """Test hook (not part of the public header): the X^T Y GEMM's form for the next set_data
        (None: leave it; 0: the size rule, 1: always classical, 2: Strassen wherever the shape
        allows) and the split-K of the Strassen products (None: leave it; 0: the rule's; > 0: at
        most that many slices).  Returns the form the current data uses (1 or 2)."""
        fn = self.L.midagma_debug_xty_form
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int]
        cur = fn(self.h, -1, -1)
        if (mode is not None or split is not None) and \
                fn(self.h, -1 if mode is None else int(mode), -1 if split is None else int(split)) < 0:
            raise ValueError(f"debug_xty_form: bad mode {mode!r} or split {split!r}")
        return int(cur)

    def debug_spoil_warm(self):
        """Test hook: zero the blocked inverse's stored warm starts, so the next fast slot hands
        back (ST_NEED_GJ) from inside its forked inverse."""
        fn = self.L.midagma_debug_spoil_warm
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
        check(fn(self.h), self.h, "debug_spoil_warm")

    def debug_tcc_fast_steps(self, steps: int | None = None) -> int:
        """Test hook: the Noda steps a fast cov slot's TCC chain runs before handing the slot back
        (0: the whole gated chain on every slot; None: leave it).  Returns the previous value."""
        fn = self.L.midagma_debug_tcc_fast_steps
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
        return int(fn(self.h, -1 if steps is None else int(steps)))

    def debug_tcc_fix(self, on=None) -> int:
        """Test hook: the TCC fixed-shift stage before Noda (True/False; None leaves it). Returns
        the old setting."""
        fn = self.L.midagma_debug_tcc_fix
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
        return int(fn(self.h, -1 if on is None else int(bool(on))))

    def debug_tcc_fastblk(self, on=None) -> int:
        """Test hook: the TCC fixed-stage inverse's fast blocks (D2 >= 2048) for the next set_trek_tcc
        (True/False; None leaves it). Returns the old setting."""
        fn = self.L.midagma_debug_tcc_fastblk
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
        return int(fn(self.h, -1 if on is None else int(bool(on))))

    def debug_at_fold(self, on=None) -> int:
        """Test hook: build_at folded into the previous slot's update (True/False; None leaves it).
        Returns the old setting (0/1), or -1 when the fold cannot apply to this solver."""
        fn = self.L.midagma_debug_at_fold
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
        return int(fn(self.h, -1 if on is None else int(bool(on))))

    def debug_handbacks(self) -> int:
        """Test hook: the hand-backs the slot scheduler has re-run on the pivoted path so far."""
        fn = self.L.midagma_debug_handbacks
        fn.restype, fn.argtypes = C.c_int64, [C.c_void_p]
        return int(fn(self.h))

    def debug_slot_matrices(self):
        """Test hook (read-only): (W, Mt) as the last slot left them on the device, d x d each.  Mt is
        inv(sI - W∘W)^T for the W that slot started from, W the slot's updated W (the next slot's
        input).  On the one-workgroup small-d loop Mt is the inverse the last launch stored for the
        next launch's warm start (of the W its last slot started from, also after a halving).
        Waits for the solver's streams; raises when no slot has run since begin."""
        W, Mt = np.empty((self.d, self.d)), np.empty((self.d, self.d))
        if self.L.midagma_debug_slot_matrices(self.h, dptr(W), dptr(Mt)) != 0:
            raise _lib.HipSolverError("debug_slot_matrices: no slot has run since begin (or no Mt buffer)")
        return W, Mt

    # fit()'s device data preparation (linear.py:406-428; the CPU test doubles override these)
    def colsum(self, X):
        return colsum_dev(X)

    def center(self, X, colsum, nrows: float):
        center_dev(X, colsum, nrows)

    def gram(self, X):
        return gram(X, self.device)

    def set_cov_gram(self, G, n: float):
        """cov = G / n on the device (G: the (all-reduced) d x d Gram matrix, a device tensor)."""
        import torch
        assert G.shape == (self.d, self.d) and G.is_contiguous()
        torch.cuda.current_stream(G.device).synchronize()
        check(self.L.midagma_set_cov_dev(self.h, C.c_void_p(G.data_ptr()), self.d, float(n)), self.h, "set_cov_dev")

    def data_gram(self):
        check(self.L.midagma_data_gram(self.h), self.h, "data_gram")

    def cov_from_zbuf(self, n: float):
        check(self.L.midagma_cov_from_zbuf(self.h, float(n)), self.h, "cov_from_zbuf")

    def get_cov(self) -> np.ndarray:
        out = np.empty((self.d, self.d))
        check(self.L.midagma_get_cov(self.h, dptr(out), self.d), self.h, "get_cov")
        return out

    def torch_zbuf(self):
        """A torch CUDA tensor bound as this solver's score-partial buffer, and a context that
        makes the solver's stream torch's current one: `with ctx: dist.all_reduce(zt)` sums the
        partial over ranks in stream order with the slot kernels (RCCL on the solver stream)."""
        import torch
        dev = torch.device("cuda", self.device)
        zt = torch.zeros(self.zbuf_len, dtype=torch.float64, device=dev)
        self.bind_zbuf(zt.data_ptr(), zt.numel())
        ext = torch.cuda.ExternalStream(self.stream, device=dev)
        return zt, (lambda: torch.cuda.stream(ext))

    def attach_comm(self, group=None):
        """Join an in-library RCCL communicator over `group` (torch.distributed; ABI 7): rank 0's
        ncclUniqueId is broadcast over the group, then every captured slot all-reduces the score
        partial itself, and minimize / run_slots drive the multi-rank loop from the device."""
        import torch
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        uid = torch.zeros(128, dtype=torch.uint8)
        if rank == 0:
            check(self.L.midagma_comm_unique_id(C.c_void_p(uid.data_ptr()), 128), None, "comm_unique_id")
        src = dist.get_global_rank(group, 0) if group is not None else 0
        if dist.get_backend(group) == "nccl":
            t = uid.to(torch.device("cuda", self.device))
            dist.broadcast(t, src=src, group=group)
            uid = t.cpu()
        else:
            dist.broadcast(uid, src=src, group=group)
        check(self.L.midagma_comm_init(self.h, C.c_void_p(uid.data_ptr()), 128, world, rank), self.h, "comm_init")

    def comm_allreduce_zbuf(self):
        check(self.L.midagma_comm_allreduce_zbuf(self.h), self.h, "comm_allreduce_zbuf")

    @property
    def comm_ranks(self) -> int:
        return int(self.L.midagma_comm_ranks(self.h))

    @property
    def zbuf_len(self) -> int:
        return int(self.L.midagma_zbuf_len(self.h))

    def bind_zbuf(self, ptr: int | None, length: int):
        check(self.L.midagma_bind_zbuf(self.h, C.c_void_p(ptr) if ptr else None, int(length)), self.h, "bind_zbuf")

    # -- the inner loop ---------------------------------------------------------
    def minimize(self, W: np.ndarray, mu: float, max_iter: int, s: float, lr: float, tol: float = 1e-6,
                 beta_1: float = 0.99, beta_2: float = 0.999, lambda1: float = 0.03,
                 checkpoint: int = 1000, want_checkpoints: bool = False):
        """Runs linear.py:165-333 on the GPU.  W (d x d float64) is updated in place."""
        assert W.shape == (self.d, self.d) and W.dtype == np.float64 and W.flags.c_contiguous
        res = _lib.MidagmaResult()
        check(self.L.midagma_minimize(self.h, dptr(W), float(mu), int(max_iter), float(s), float(lr), float(tol),
                                      float(beta_1), float(beta_2), float(lambda1), int(checkpoint),
                                      C.byref(res)), self.h, "minimize")
        return MinimizeResult.from_c(res, self.checkpoints() if want_checkpoints else ())

    def begin(self, W, mu, max_iter, s, lr, tol=1e-6, beta_1=0.99, beta_2=0.999, lambda1=0.03, checkpoint=1000):
        W = _as_f64(W)
        check(self.L.midagma_begin(self.h, dptr(W), float(mu), int(max_iter), float(s), float(lr), float(tol),
                                   float(beta_1), float(beta_2), float(lambda1), int(checkpoint)), self.h, "begin")

    def run_slots(self, n: int):
        check(self.L.midagma_run_slots(self.h, int(n)), self.h, "run_slots")

    def sync(self):
        check(self.L.midagma_sync(self.h), self.h, "sync")

    def profile_parts(self, reps: int = 10) -> dict:
        """Average device ms per launch group, measured with hipEvents on the solver stream."""
        out = np.zeros(8)
        check(self.L.midagma_profile_parts(self.h, int(reps), dptr(out)), self.h, "profile_parts")
        keys = ["build_at", "gj_inverse", "score", "slot", "gemm_xw", "gemm_xty", "inverse_fast", "slot_fast"]
        return {k: float(out[i]) for i, k in enumerate(keys)}

    def step_partial(self):
        check(self.L.midagma_step_partial(self.h), self.h, "step_partial")

    def step_finish(self):
        check(self.L.midagma_step_finish(self.h), self.h, "step_finish")

    def poll(self) -> _lib.MidagmaResult:
        r = _lib.MidagmaResult()
        check(self.L.midagma_poll(self.h, C.byref(r)), self.h, "poll")
        return r

    def end(self, W: np.ndarray) -> MinimizeResult:
        r = _lib.MidagmaResult()
        check(self.L.midagma_end(self.h, dptr(W), C.byref(r)), self.h, "end")
        return MinimizeResult.from_c(r)

    def checkpoints(self):
        """Checkpoint records of the last minimize call (`CheckpointRecord`: tuple-indexable
        (iter, obj, score, h, lr, l1, ...) and attribute access)."""
        cap = 1 << 16
        buf = (_lib.MidagmaCkpt * cap)()
        n = self.L.midagma_checkpoints(self.h, buf, cap)
        check(n, self.h, "checkpoints")
        return [CheckpointRecord(*(int(c.iter) if f == "iter" else float(getattr(c, f))
                                   for f in CheckpointRecord._fields)) for c in buf[:n]]

    # -- helpers of the reference API ----------------------------------------------
    def h_value(self, W: np.ndarray, s: float = 1.0, grad: bool = True):
        W = _as_f64(W)
        h = C.c_double()
        G = np.empty((self.d, self.d)) if grad else None
        check(self.L.midagma_h(self.h, dptr(W), float(s), C.byref(h), dptr(G)), self.h, "h")
        return float(h.value), G

    def score_value(self, W: np.ndarray):
        W = _as_f64(W)
        loss = C.c_double()
        G = np.empty((self.d, self.d))
        check(self.L.midagma_score(self.h, dptr(W), C.byref(loss), dptr(G)), self.h, "score")
        return float(loss.value), G

    def score_partial(self, W: np.ndarray):
        W = _as_f64(W)
        check(self.L.midagma_score_partial(self.h, dptr(W)), self.h, "score_partial")

    def score_finish(self):
        loss = C.c_double()
        G = np.empty((self.d, self.d))
        check(self.L.midagma_score_finish(self.h, C.byref(loss), dptr(G)), self.h, "score_finish")
        return float(loss.value), G


def row_range(n: int, parts: int, k: int):
    """Rows [lo, hi) of part k of the even split of n rows (the first n % parts parts take one
    row more): the data-mode shard of rank / group member k."""
    base, extra = divmod(int(n), int(parts))
    lo = k * base + min(k, extra)
    return lo, lo + base + (1 if k < extra else 0)


class HipGroup(_Handle):
    """Data mode on several devices from ONE process (ABI 11, `midagma_group_*`): member k is a
    data-mode `HipSolver` on devices[k] holding row shard k of X, and every slot sums the members'
    score partials (the Python side stays single-process; the reference's own
    entry is the single-process `fit(X)`, linear.py:335-351).

    Distinct devices: an RCCL communicator per member from ncclCommInitAll, the all-reduce inside
    each member's replayed slot graphs, one library thread per device.  Repeated devices (every
    entry the same, e.g. [0, 0, 0, 0]) or emulate=True: an emulated group on that one device, whose
    slots are captured as one graph with a fixed-order device sum of the partials instead of RCCL
    (the sharding's arithmetic on a one-GPU box).

    It answers HipSolver's calls that `DagmaLinear` makes, broadcasting the loop's settings to
    every member and reading results from member 0."""

    is_group = True
    _destroy, _last_error = "midagma_group_destroy", "midagma_group_last_error"

    def __init__(self, d: int, loss: str = "l2", devices=(0,), emulate: bool | None = None):
        self.L = _lib.lib()
        self.members = []
        self.d, self.loss, self.mode = int(d), loss, "data"
        devices = [int(x) for x in devices]
        if not devices:
            raise ValueError("devices must name at least one device")
        if emulate is None:
            emulate = len(set(devices)) < len(devices)
        lt = {"l2": _lib.LOSS_L2, "logistic": _lib.LOSS_LOGISTIC}[loss]
        arr = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        self._check(self.L.midagma_group_create(C.byref(h), lt, self.d, arr, len(devices),
                                                _lib.GROUP_EMULATE if emulate else 0), None, "group_create")
        self.h = h
        self.devices = devices
        self.device = devices[0]
        self.emulated = bool(self.L.midagma_group_emulated(h))
        self.members = [HipSolver(self.d, loss, "data", device=dv, _handle=self.L.midagma_group_member(h, k))
                        for k, dv in enumerate(devices)]
        self.D = self.members[0].D

    def close(self):
        for m in self.members:
            m.close()
        super().close()

    @property
    def size(self) -> int:
        return len(self.members)

    @property
    def comm_ranks(self) -> int:
        return 0 if self.emulated else len(self.members)

    # -- data -----------------------------------------------------------------------
    def set_data(self, X, n_global: int | None = None):
        """X: the whole host ndarray or torch tensor (n x d, n_global ignored), split by rows over
        the members (`row_range`).  A tensor's shards are copied to each member's device."""
        n = int(X.shape[0])
        if n < self.size:
            raise ValueError(f"set_data: {n} rows for {self.size} members")
        if hasattr(X, "data_ptr"):
            import torch
            for k, m in enumerate(self.members):
                lo, hi = row_range(n, self.size, k)
                part = X[lo:hi].to(torch.device("cuda", m.device)).contiguous()
                m.set_data(part, n_global=n)
            return
        X = _as_f64(X)
        self._check(self.L.midagma_group_set_data(self.h, X.ctypes.data_as(_lib._dp), n), self.h, "group_set_data")

    def set_cov(self, cov):
        for m in self.members:
            m.set_cov(cov)

    # fit()'s device data preparation for a device X (on one device; the shards are copied out)
    def colsum(self, X):
        return colsum_dev(X)

    def center(self, X, colsum, nrows: float):
        center_dev(X, colsum, nrows)

    def set_w_float32(self, on: bool):
        for m in self.members:
            m.set_w_float32(on)

    def set_masks(self, mask_inc, mask_exc):
        for m in self.members:
            m.set_masks(mask_inc, mask_exc)

    def set_trek(self, *a, **k):
        for m in self.members:
            m.set_trek(*a, **k)

    def set_trek_tcc(self, *a, **k):
        for m in self.members:
            m.set_trek_tcc(*a, **k)

    def allreduce_zbuf(self):
        """Every member's score buffer <- the sum over the members (RCCL, or the emulated sum)."""
        self._check(self.L.midagma_group_allreduce_zbuf(self.h), self.h, "group_allreduce_zbuf")

    comm_allreduce_zbuf = allreduce_zbuf

    def gram_cov(self, n: float) -> np.ndarray:
        """cov = (sum_k X_k^T X_k) / n (linear.py:428) from the members' device Gram matrices."""
        for m in self.members:
            m.data_gram()
        self.allreduce_zbuf()
        for m in self.members:
            m.cov_from_zbuf(float(n))
        return self.members[0].get_cov()

    def get_cov(self) -> np.ndarray:
        return self.members[0].get_cov()

    # -- the loop -------------------------------------------------------------------
    def minimize(self, W: np.ndarray, mu: float, max_iter: int, s: float, lr: float, tol: float = 1e-6,
                 beta_1: float = 0.99, beta_2: float = 0.999, lambda1: float = 0.03,
                 checkpoint: int = 1000, want_checkpoints: bool = False):
        """linear.py:165-333 over the group; W (d x d float64) updated in place."""
        assert W.shape == (self.d, self.d) and W.dtype == np.float64 and W.flags.c_contiguous
        res = _lib.MidagmaResult()
        self._check(self.L.midagma_group_minimize(self.h, dptr(W), float(mu), int(max_iter), float(s), float(lr),
                                                  float(tol), float(beta_1), float(beta_2), float(lambda1),
                                                  int(checkpoint), C.byref(res)), self.h, "group_minimize")
        return MinimizeResult.from_c(res, self.checkpoints() if want_checkpoints else ())

    def checkpoints(self):
        return self.members[0].checkpoints()

    def h_value(self, W, s: float = 1.0, grad: bool = True):
        return self.members[0].h_value(W, s, grad)

    def trek_value(self, W, grad: bool = True):
        return self.members[0].trek_value(W, grad)

    def score_partial(self, W):
        for m in self.members:
            m.score_partial(W)

    def score_finish(self):
        return self.members[0].score_finish()

    def score(self, W):
        """_score in data mode (linear.py:70-94): every member's partial, summed, finished."""
        self.score_partial(W)
        self.allreduce_zbuf()
        return self.score_finish()


def _vp(a):
    """void* of an array (NULL for None or an empty one, which has no usable address)."""
    return None if a is None or a.size == 0 else C.c_void_p(a.ctypes.data)


class _ColumnEngine(_Handle):
    """What the test engines over the columns of one X spell alike (csrc/coltest.h), once.  A subclass
    names its family, the `<family>` of its `midagma_<family>_*` symbols, and keeps its own
    signatures and docstrings; MAX_N is its cap on n (None: the library's)."""

    _family = ""
    MAX_N = None

    def __init_subclass__(cls):
        cls._destroy, cls._last_error = f"midagma_{cls._family}_destroy", f"midagma_{cls._family}_last_error"

    def _call(self, entry: str, *args):
        """`midagma_<family>_<entry>(handle, *args)`, checked."""
        rc = getattr(self.L, f"midagma_{self._family}_{entry}")(self.h, *args)
        self._check(rc, self.h, f"{self._family}_{entry}")

    def _open(self, X, device: int, *budget):
        """Create the handle on X's device (a device tensor's own) and set the data."""
        self.L = _lib.lib()
        self.h = None
        self.n = self.d = 0
        what = type(self).__name__
        if is_device_tensor(X):
            X = _device_x(X, what, self.MAX_N)
            device = X.device.index
        else:
            X = _host_x(X, what, self.MAX_N)  # (the library copies it to the device and never writes it)
        h = C.c_void_p()
        create = getattr(self.L, f"midagma_{self._family}_create")
        self._check(create(C.byref(h), int(device)), None, f"{self._family}_create")
        self.h = h
        try:
            self._set_data(X, *budget)
        except Exception:
            self.close()
            raise

    def _set_data(self, X, *budget):
        self.n = self.d = 0
        what = type(self).__name__
        if is_device_tensor(X):
            X = _device_x(X, what, self.MAX_N)
            n, d, ld = _rows(X)
            self._call("set_data_dev", C.c_void_p(X.data_ptr()), n, d, ld, *budget, _cur_stream(X.device))
        else:
            X = _host_x(X, what, self.MAX_N)
            n, d = int(X.shape[0]), int(X.shape[1])
            self._call("set_data", dptr(X), n, d, *budget)
        self.n, self.d = n, d

    def _set_bandwidths(self, sigma2):
        s2 = _as_f64(sigma2).ravel()
        self._call("set_bandwidths", dptr(s2), s2.size)

    def _median_bandwidths(self, cols) -> np.ndarray:
        if not self.d:
            raise ValueError(f"{self._family}_median_bandwidths: set the data first")
        s2 = np.zeros(self.d)
        if cols is None:
            cp, nc = None, 0
        else:
            cols = np.ascontiguousarray(cols, dtype=np.int64).ravel()
            if cols.size == 0:  # (an empty array has no usable address)
                s2[:] = 1.0
                self._set_bandwidths(s2)
                return s2
            cp, nc = C.c_void_p(cols.ctypes.data), int(cols.size)
        self._call("median_bandwidths", cp, nc, dptr(s2))
        return s2

    def _run(self, pairs, P: int, perms, seed: int, return_null: bool, *knobs):
        """`midagma_<family>_run` with the family's `knobs` between the seed and the outputs."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
        m, P = int(pairs.shape[0]), int(P)
        if perms is not None:
            perms = np.ascontiguousarray(perms, dtype=np.int32)
            if perms.shape != (m, P, self.n):
                raise ValueError(f"perms must be {(m, P, self.n)}, got {perms.shape}")
        stat = np.zeros(m)
        ge = np.zeros(m, dtype=np.int64)
        null = np.zeros((m, max(P, 0))) if return_null else None
        self._call("run", _vp(pairs), m, P, _vp(perms), C.c_uint64(int(seed) & (2**64 - 1)), *knobs, dptr(stat),
                   _vp(ge), dptr(null) if (return_null and null.size) else None)
        return (stat, ge, null) if return_null else (stat, ge)

    def _device_perms(self, q: int, P: int, seed: int, *inverse):
        out = np.zeros((int(P), self.n), dtype=np.int32)
        self._call("perms", int(q), int(P), C.c_uint64(int(seed) & (2**64 - 1)), C.c_void_p(out.ctypes.data),
                   *[None if a is None else C.c_void_p(a.ctypes.data) for a in inverse])
        return out


class HipIndep(_ColumnEngine):
    """Pairwise permutation independence tests on one GPU (`midagma_indep_*`, csrc/indep.hip):
    the engine under `midagma_amd.mi_tests`.  Holds a device copy of X (n x d).

    X is a host array, or a 2-d float64 torch CUDA tensor: the engine then lives on the tensor's
    device (`device` is ignored), reads X there on torch's current stream for that device without
    a host copy (a unit column stride is used as it is, anything else through `.contiguous()`) and
    never writes it.  No synchronise is needed around the call."""

    KINDS = {"hsic": 0, "dcor": 1}
    MAX_N = 16384
    _family = "indep"

    def __init__(self, X, device: int = 0):
        self._open(X, device)

    def set_data(self, X):
        """Replace the engine's data (bandwidths and pre-passes are dropped).  A device tensor must
        live on the engine's device.  When the library rejects a device X (inf or nan), the engine
        holds no data: every later call raises ValueError until a set_data succeeds."""
        self._set_data(X)

    def set_bandwidths(self, sigma2):
        """The RBF kernels' sigma^2 per variable (hsic)."""
        self._set_bandwidths(sigma2)

    def median_bandwidths(self, cols=None) -> np.ndarray:
        """sigma^2 per variable by the reference's median heuristic, computed on the device (bit for
        bit `mi_tests.median_sigma2` of the column) for the listed columns (None: all) and 1.0 for
        the others; installed as `set_bandwidths` would.  Returns all d values."""
        return self._median_bandwidths(cols)

    def bandwidth_ms(self) -> float:
        """The last `median_bandwidths`' kernel time in ms (device events; diagnostics)."""
        ms = np.zeros(1)
        self._check(self.L.midagma_indep_bandwidth_profile(self.h, dptr(ms)), self.h, "indep_bandwidth_profile")
        return float(ms[0])

    def batch_pairs(self, P: int, budget_bytes: int = 0) -> int:
        """Pairs per device batch under a byte budget (0: the library's default)."""
        return int(self.L.midagma_indep_batch_pairs(self.h, int(P), int(budget_bytes)))

    def profile(self) -> dict:
        """The last run's stage times in ms, summed over its batches (diagnostics)."""
        ms = np.zeros(4)
        self._check(self.L.midagma_indep_profile(self.h, dptr(ms)), self.h, "indep_profile")
        return dict(zip(("host_stage_ms", "upload_ms", "perm_kernel_ms", "stat_kernel_ms"), ms.tolist()))

    def run(self, kind: str, pairs, P: int, perms=None, seed: int = 0, budget_bytes: int = 0,
            return_null: bool = False, return_perms: bool = False):
        """(stat, ge[, null][, perms]) per pair: the observed statistic, ge = #{p : stat_p >= stat}
        over P permutations, the P permuted statistics (m x P) and the device's permutations.
        perms: explicit m x P x n int32 permutations, or None for device permutations from `seed`."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
        m, P = int(pairs.shape[0]), int(P)
        if perms is not None:
            perms = np.ascontiguousarray(perms, dtype=np.int32)
            if perms.shape != (m, P, self.n):
                raise ValueError(f"perms must be {(m, P, self.n)}, got {perms.shape}")
        stat = np.zeros(m)
        ge = np.zeros(m, dtype=np.int64)
        null = np.zeros((m, P)) if return_null else None
        pout = np.zeros((m, P, self.n), dtype=np.int32) if (return_perms and perms is None) else None

        def vp(a):
            return None if a is None else C.c_void_p(a.ctypes.data)

        rc = self.L.midagma_indep_run(self.h, self.KINDS[kind], vp(pairs), m, P, vp(perms),
                                      C.c_uint64(int(seed) & (2**64 - 1)), int(budget_bytes), dptr(stat), vp(ge),
                                      dptr(null), vp(pout))
        self._check(rc, self.h, "indep_run")
        out = [stat, ge]
        if return_null:
            out.append(null)
        if return_perms:
            out.append(perms if perms is not None else pout)
        return tuple(out)


def column_argsort(X, budget_bytes: int = 0):
    """order (d x n int32 device tensor): order[c, i] = the row at position i of the stable argsort
    of column c of X (-0.0 equal to +0.0), the row payload of `column_ranks`' radix sort
    (`midagma_colargsort`).  X and budget_bytes as in `column_ranks`."""
    import torch
    X = _device_matrix(X, "column_argsort")
    n, d, ld = _rows(X)
    order = torch.empty((d, n), dtype=torch.int32, device=X.device)
    with torch.cuda.device(X.device):
        check(_lib.lib().midagma_colargsort(C.c_void_p(X.data_ptr()), n, d, ld, C.c_void_p(order.data_ptr()),
                                            int(budget_bytes), _cur_stream(X.device)), None, "column_argsort")
    return order


class HipDcor(_ColumnEngine):
    """dCor permutation tests of pairs of columns without the n^2 sum, on one GPU
    (`midagma_dcor_*`, csrc/dcor.hip): the engine under `mi_tests.dcor_null` / `dcor_tests`, for
    2 <= n < 2^31.  Holds the per-column sorts, centred values and row sums of X (24 bytes a value).

    X is a host array (copied to `device`), or a 2-d float64 torch CUDA tensor: the engine then
    lives on the tensor's device (`device` is ignored), reads X there on torch's current stream
    without a host copy and never writes it.  No synchronise is needed around the call."""

    _family = "dcor"

    def __init__(self, X, device: int = 0, budget_bytes: int = 0):
        self._open(X, device, int(budget_bytes))

    def set_data(self, X, budget_bytes: int = 0):
        """Replace the engine's data and run the per-column pre-pass.  When the library rejects a
        device X (inf or nan), the engine holds no data."""
        self._set_data(X, int(budget_bytes))

    def run(self, pairs, P: int, perms=None, seed: int = 0, *, unbiased: bool = False, block: int = 0,
            budget_bytes: int = 0, return_null: bool = False):
        """(stat, ge[, null]) per pair, as `HipIndep.run("dcor", ...)`; unbiased: the bias-corrected
        R_U, counted by dcov^2_U.  perms: explicit m x P x n int32 permutations, or None for device
        permutations from `seed` (csrc/coltest.h's rule).  block: the block edge (0: the rule)."""
        return self._run(pairs, P, perms, seed, return_null, int(bool(unbiased)), int(block), int(budget_bytes))

    def device_perms(self, q: int, P: int, seed: int = 0, inverse: bool = False):
        """The P device permutations (P x n int32) of pair q of a call with this seed, and with
        `inverse` their inverses."""
        inv = np.zeros((int(P), self.n), dtype=np.int32) if inverse else None
        out = self._device_perms(q, P, seed, inv)
        return (out, inv) if inverse else out


class HipHsic(_ColumnEngine):
    """HSIC permutation tests of pairs of columns from low-rank factors of the RBF Gram matrices, on
    one GPU (`midagma_hsic_*`, csrc/hsic.hip): the engine under `mi_tests.hsic_null` / `hsic_tests`,
    for 2 <= n < 2^31, and the chi-square test's statistic of every pair at once (`all_pairs`).  Holds the columns of X by row and sorted (16 bytes a value) and the centred
    factors of the columns in use (8 n r_pad bytes each).

    X is a host array (copied to `device`), or a 2-d float64 torch CUDA tensor: the engine then
    lives on the tensor's device (`device` is ignored), reads X there on torch's current stream
    without a host copy and never writes it.  No synchronise is needed around the call."""

    TOL = 1e-13
    _family = "hsic"

    def __init__(self, X, device: int = 0, budget_bytes: int = 0):
        self._open(X, device, int(budget_bytes))

    def set_data(self, X, budget_bytes: int = 0):
        """Replace the engine's data (bandwidths and factors are dropped).  When the library rejects
        a device X (inf or nan), the engine holds no data."""
        self._set_data(X, int(budget_bytes))

    def set_bandwidths(self, sigma2):
        """The RBF kernels' sigma^2 per variable (factors are dropped)."""
        self._set_bandwidths(sigma2)

    def median_bandwidths(self, cols=None) -> np.ndarray:
        """sigma^2 per variable by the reference's median heuristic at any n, on the device (bit for
        bit `mi_tests.median_sigma2` of the column) for the listed columns (None: all) and 1.0 for
        the others; installed as `set_bandwidths` would.  Returns all d values."""
        return self._median_bandwidths(cols)

    def factor(self, cols, tol: float = TOL):
        """(rank, resid) of the listed columns' pivoted incomplete Cholesky factors at `tol`: int32
        ranks and the largest residual diagonal entries reached.  The factors stay on the engine."""
        cols = np.ascontiguousarray(cols, dtype=np.int64).ravel()
        rank = np.zeros(cols.size, dtype=np.int32)
        resid = np.zeros(cols.size)
        if cols.size == 0:
            return rank, resid
        rc = self.L.midagma_hsic_factor(self.h, C.c_void_p(cols.ctypes.data), int(cols.size), float(tol),
                                        C.c_void_p(rank.ctypes.data), dptr(resid))
        self._check(rc, self.h, "hsic_factor")
        return rank, resid

    def get_factor(self, col: int, rank: int):
        """(Fc, mean): the centred factor of a factored column (n x r_pad, r_pad the rank rounded up
        to a multiple of 16) and the column means that were subtracted (diagnostics)."""
        rp = (int(rank) + 15) // 16 * 16
        Fc, mean = np.zeros((self.n, rp)), np.zeros(rp)
        self._check(self.L.midagma_hsic_get_factor(self.h, int(col), dptr(Fc), dptr(mean)), self.h, "hsic_get_factor")
        return Fc, mean

    def run(self, pairs, P: int, perms=None, seed: int = 0, *, tol: float = TOL, chunk: int = 0,
            budget_bytes: int = 0, return_null: bool = False):
        """(stat, ge[, null]) per pair, as `HipIndep.run("hsic", ...)` to within 4 tol (1 + tol) plus
        rounding.  perms: explicit m x P x n int32 permutations, or None for device permutations from
        `seed` (csrc/coltest.h's rule).  chunk: rows per partial product (0: the rule)."""
        return self._run(pairs, P, perms, seed, return_null, float(tol), int(chunk), int(budget_bytes))

    def all_pairs(self, cols=None, *, tol: float = TOL, chunk: int = 0, budget_bytes: int = 0):
        """(cov_u, biased), two k x k host arrays over the listed columns (None: all d): cov_u is
        the U-centred covariance <A~_i, A~_j> / (n (n - 3)) of the distances D = 1 - K (the
        variances on the diagonal), the statistic of the chi-square test; biased is `run`'s
        statistic || Fc_i^T Fc_j ||_F^2 / n^2.  One tiled FP64 MFMA pass over the centred factors
        side by side, one evaluation a pair; needs n >= 4.  chunk: rows per partial product (0:
        the rule).  The bits do not depend on budget_bytes or on the other columns listed."""
        if cols is None:
            cp, k = None, self.d
        else:
            cols = np.ascontiguousarray(cols, dtype=np.int64).ravel()
            k = int(cols.size)
            if k == 0:
                return np.zeros((0, 0)), np.zeros((0, 0))
            cp = C.c_void_p(cols.ctypes.data)
        cov, bia = np.zeros((k, k)), np.zeros((k, k))
        rc = self.L.midagma_hsic_all_pairs(self.h, cp, k, float(tol), int(chunk), int(budget_bytes), dptr(cov),
                                           dptr(bia))
        self._check(rc, self.h, "hsic_all_pairs")
        return cov, bia

    def device_perms(self, q: int, P: int, seed: int = 0):
        """The P device permutations (P x n int32) of pair q of a call with this seed."""
        return self._device_perms(q, P, seed)

    def profile(self) -> dict:
        """Times in ms: the last `median_bandwidths`, and the last run's factorisation, permutations
        and evaluation kernels (diagnostics)."""
        ms = np.zeros(4)
        self._check(self.L.midagma_hsic_profile(self.h, dptr(ms)), self.h, "hsic_profile")
        return dict(zip(("median_ms", "factor_ms", "perm_ms", "eval_ms"), ms.tolist()))

    def all_pairs_profile(self) -> dict:
        """Times in ms of the last `all_pairs`: the factorisation, the tiled pass over the factors,
        and the O(n) vectors with their Grams (diagnostics)."""
        ms = np.zeros(3)
        self._check(self.L.midagma_hsic_all_pairs_profile(self.h, dptr(ms)), self.h, "hsic_all_pairs_profile")
        return dict(zip(("factor_ms", "tile_ms", "vector_ms"), ms.tolist()))


class HipBatch(_Handle):
    """B independent small-d problems (d <= 64, l2, cov mode, float64) on one GPU, one persistent
    workgroup each (`midagma_batch_*`, csrc/batch.hip).  The problems share d and the loop
    settings; each has its own covariance, masks, mu, s, lr and lambda1.  Problem b's W, result
    and checkpoint records are bit-identical to a `HipSolver` run of that problem alone.

    With `set_trek` (d <= 32) the PST trek regularizer runs inside each problem's workgroup
    (csrc/pst_blk.h): one pair list, a weight per problem.  A problem's result then does not
    depend on the rest of the batch, and agrees with `HipSolver.set_trek`'s launch chain to
    rounding, not bit for bit.

    With `set_data` the logistic loss runs in the same slots (`minimize_logistic`,
    `midagma_blogit_*`): each workgroup streams its problem's X in row blocks through the score
    phase.  Float64, no trek regularizer, one n for all problems; results are independent of the
    rest of the batch bit for bit and agree with `HipSolver(d, "logistic", "data")` to rounding."""

    MAX_D, MAX_B, MAX_D_TREK = 64, 16384, 32
    _destroy, _last_error = "midagma_batch_destroy", "midagma_batch_last_error"

    def __init__(self, d: int, B: int, device: int = 0):
        self.L = _lib.lib()
        self.h = None
        self.d, self.B, self.device = int(d), int(B), int(device)
        self._has_cov = self._has_data = False
        h = C.c_void_p()
        self._check(self.L.midagma_batch_create(C.byref(h), self.d, self.B, self.device), None, "batch_create")
        self.h = h

    def _stack(self, a, what) -> np.ndarray:
        a = _as_f64(a)
        if a.shape != (self.B, self.d, self.d):
            raise ValueError(f"{what} must be {(self.B, self.d, self.d)}, got {a.shape}")
        return a

    def _per_problem(self, x, what) -> np.ndarray:
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), (self.B,)))
        if a.shape != (self.B,):  # pragma: no cover (broadcast_to raised already)
            raise ValueError(f"{what} must be a scalar or hold {self.B} values")
        return a

    def set_cov(self, cov):
        """cov: B x d x d (copied); ValueError on inf / nan."""
        cov = self._stack(cov, "cov")
        self._check(self.L.midagma_batch_set_cov(self.h, dptr(cov)), self.h, "batch_set_cov")
        self._has_cov = True

    def boot_cov(self, X, seed: int, first: int = 0, budget_bytes: int | None = None):
        """Problem b's cov <- the covariance of bootstrap replicate `first + b` of `seed` of X
        (`midagma_amd.batch.bootstrap_indices`), formed on the device from one X (csrc/boot.hip).
        X: (n, d) float64, a host array or a device tensor (its row stride is kept); it is not
        written.  budget_bytes: the scratch of one chunk of replicates (None: 1 GiB).  ValueError
        on inf / nan."""
        n, d, ld = _rows(X)
        if d != self.d:
            raise ValueError(f"X must have {self.d} columns, got {d}")
        on_dev = is_device_tensor(X)
        if on_dev:
            import torch
            if X.device.index is not None and X.device.index != self.device:
                raise ValueError(f"X lies on device {X.device.index}, the batch on {self.device}")
            torch.cuda.current_stream(X.device).synchronize()  # (the batch runs on its own stream)
            src = C.c_void_p(X.data_ptr())
        elif hasattr(X, "data_ptr"):
            raise ValueError("X must be a host array or a device tensor")
        else:
            src = X.ctypes.data_as(C.c_void_p)
        rc = self.L.midagma_boot_cov(self.h, src, n, ld, 1 if on_dev else 0, C.c_uint64(int(seed) & (2**64 - 1)),
                                     int(first), 0 if budget_bytes is None else int(budget_bytes))
        self._check(rc, self.h, "boot_cov")
        self._has_cov = True

    def get_cov(self) -> np.ndarray:
        """The problems' current covariances, (B, d, d)."""
        out = np.empty((self.B, self.d, self.d))
        self._check(self.L.midagma_boot_get_cov(self.h, dptr(out)), self.h, "boot_get_cov")
        return out

    def boot_profile(self) -> dict:
        """Device-event times (ms) of the last `boot_cov`, summed over its chunks."""
        ms = np.zeros(4)
        self._check(self.L.midagma_boot_profile(self.h, dptr(ms)), self.h, "boot_profile")
        return dict(zip(("center_ms", "counts_ms", "gram_ms", "finish_ms"), ms.tolist()))

    def set_masks(self, mask_inc, mask_exc):
        """B x d x d each, or None to switch that mask off (linear.py:217-222, per problem)."""
        mi = None if mask_inc is None else self._stack(mask_inc, "mask_inc")
        me = None if mask_exc is None else self._stack(mask_exc, "mask_exc")
        self._check(self.L.midagma_batch_set_masks(self.h, dptr(mi), dptr(me)), self.h, "batch_set_masks")

    def set_trek(self, pairs, seq: str = "exp", *, agg: str = "mean", mode: str = "opt", weight=0.0,
                 eps_inv: float = 1e-8):
        """The PST trek regularizer (notreks.pst) inside every problem's loop: one pair list, `weight`
        a scalar or B values.  seq 'exp' or 'inv', d <= 32; mode 'off' or no pairs disables it."""
        P = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2)) if pairs is not None \
            else np.zeros((0, 2), dtype=np.int64)
        seq, agg, mode = seq.lower().strip(), agg.lower().strip(), mode.lower().strip()
        if seq not in HipSolver.TREK_SEQ or agg not in HipSolver.TREK_AGG or mode not in HipSolver.TREK_MODE:
            raise ValueError(f"unsupported PST configuration seq={seq!r} agg={agg!r} mode={mode!r}")
        w = self._per_problem(weight, "weight")
        rc = self.L.midagma_btrek_set(self.h, HipSolver.TREK_SEQ[seq], HipSolver.TREK_AGG[agg],
                                      HipSolver.TREK_MODE[mode], dptr(w), float(eps_inv),
                                      P.ctypes.data_as(C.POINTER(C.c_int64)), int(P.shape[0]))
        self._check(rc, self.h, "btrek_set")

    def trek_value(self, W: np.ndarray, grad: bool = True):
        """notreks.trek_value_grad of B matrices (B x d x d) for the configured regularizer, no Adam
        step: ((B,) values, (B, d, d) gradients or None); zeros without a regularizer."""
        W = self._stack(W, "W")
        v = np.empty(self.B)
        G = np.empty((self.B, self.d, self.d)) if grad else None
        self._check(self.L.midagma_btrek_value(self.h, dptr(W), dptr(v), dptr(G)), self.h, "btrek_value")
        return v, G

    def set_data(self, X, shared: bool = False):
        """The logistic loss's data (copied, not written): one (n, d) X for all problems, stored once
        on the device (`shared=True`), or (B, n, d).  ValueError on inf / nan, or when the padded
        slabs exceed the device's free memory."""
        X = _as_f64(X)
        if X.ndim != (2 if shared else 3) or X.shape[-1] != self.d or (not shared and X.shape[0] != self.B) \
                or X.shape[-2] < 1:
            raise ValueError(f"X must be (n, {self.d}) shared or ({self.B}, n, {self.d}), got {X.shape} "
                             f"(shared={bool(shared)})")
        rc = self.L.midagma_blogit_set_data(self.h, dptr(X), int(X.shape[-2]), 1 if shared else 0)
        self._check(rc, self.h, "blogit_set_data")
        self._has_data = True

    def score_logistic(self, W: np.ndarray, grad: bool = True):
        """The reference's logistic `_score` (linear.py:89-92) of B matrices (B x d x d) on the
        problems' X and cov, no Adam step: ((B,) losses, (B, d, d) gradients or None)."""
        W = self._stack(W, "W")
        if not self._has_data or (grad and not self._has_cov):
            raise _lib.HipSolverError("blogit_score: set_data (and set_cov for the gradient) first")
        loss = np.empty(self.B)
        G = np.empty((self.B, self.d, self.d)) if grad else None
        self._check(self.L.midagma_blogit_score(self.h, dptr(W), dptr(loss), dptr(G)), self.h, "blogit_score")
        return loss, G

    def minimize_logistic(self, W: np.ndarray, mu, s, lr, lambda1, max_iter: int, tol: float = 1e-6,
                          beta_1: float = 0.99, beta_2: float = 0.999, checkpoint: int = 1000, active=None,
                          want_checkpoints: bool = False):
        """`minimize` with the logistic loss on the X of `set_data`; `set_cov` holds the uncentred
        X^T X / n of each problem (linear.py:428)."""
        if not self._has_data:
            raise _lib.HipSolverError("blogit_minimize: set_data before minimize_logistic")
        return self.minimize(W, mu, s, lr, lambda1, max_iter, tol, beta_1, beta_2, checkpoint, active,
                             want_checkpoints, _entry="midagma_blogit_minimize")

    def minimize(self, W: np.ndarray, mu, s, lr, lambda1, max_iter: int, tol: float = 1e-6, beta_1: float = 0.99,
                 beta_2: float = 0.999, checkpoint: int = 1000, active=None, want_checkpoints: bool = False,
                 _entry: str = "midagma_batch_minimize"):
        """linear.py:165-333 for every active problem in one launch sequence.  W (B x d x d float64)
        is updated in place; mu, s, lr, lambda1 are scalars or hold B values; active: B booleans
        (None: all).  Returns B `MinimizeResult`s; an inactive problem's W is untouched and its
        entry is None.  A singular problem is reported in its result's status, not raised."""
        assert W.shape == (self.B, self.d, self.d) and W.dtype == np.float64 and W.flags.c_contiguous
        if not self._has_cov:
            raise _lib.HipSolverError("batch_minimize: set_cov before minimize")
        mu, s, lr, lambda1 = (self._per_problem(x, n) for x, n in ((mu, "mu"), (s, "s"), (lr, "lr"),
                                                                   (lambda1, "lambda1")))
        act = None if active is None else np.ascontiguousarray(np.asarray(active, dtype=bool).astype(np.uint8))
        if act is not None and act.shape != (self.B,):
            raise ValueError(f"active must hold {self.B} values")
        res = (_lib.MidagmaResult * self.B)()
        rc = getattr(self.L, _entry)(self.h, dptr(W), dptr(mu), dptr(s), dptr(lr), dptr(lambda1), int(max_iter),
                                     float(tol), float(beta_1), float(beta_2), int(checkpoint),
                                     None if act is None else C.c_void_p(act.ctypes.data), res)
        self._check(rc, self.h, _entry[len("midagma_"):])
        return [MinimizeResult.from_c(res[b], self.checkpoints(b) if want_checkpoints else ())
                if act is None or act[b] else None for b in range(self.B)]

    def checkpoints(self, b: int):
        """Problem b's checkpoint records of the last minimize call (`CheckpointRecord`)."""
        cap = 1 << 12
        while True:
            buf = (_lib.MidagmaCkpt * cap)()
            n = self._check(self.L.midagma_batch_checkpoints(self.h, int(b), buf, cap), self.h, "batch_checkpoints")
            if n < cap:
                break
            cap *= 16
        return [CheckpointRecord(*(int(c.iter) if f == "iter" else float(getattr(c, f))
                                   for f in CheckpointRecord._fields)) for c in buf[:n]]


def run_allreduce_minimize(backend, W, mu, max_iter, s, lr, tol=1e-6, beta_1=0.99, beta_2=0.999,
                           lambda1=0.03, checkpoint=1000, allreduce=None, batch: int = 32, agree=None):
    """Data-parallel inner loop over ranks.

    ``backend`` exposes begin/step_partial/step_finish/poll/end (HipSolver, or a
    test double); ``allreduce()`` sums the backend's score partial over ranks
    in place.  Termination is decided on the device by the controller kernel;
    the host polls every ``batch`` steps, extra steps after termination are
    no-ops, so every rank runs the same number of all-reduces.

    The replicas decide identically only while the all-reduce hands every rank the
    same bits (a ring all-reduce does; ``NCCL_ALGO=Ring`` pins it).  ``agree(status,
    iters)``, called at every poll, compares the ranks' states with one small
    collective and raises on a mismatch, so a divergent replica fails loudly instead
    of leaving the other ranks waiting in an all-reduce it no longer issues.
    """
    backend.begin(W, mu, max_iter, s, lr, tol, beta_1, beta_2, lambda1, checkpoint)
    slots = 0
    cap = int(max_iter) + int(max_iter) // max(int(checkpoint), 1) + 512
    while True:
        last = backend.poll()
        if agree is not None:
            agree(int(last.status), int(last.iters))
        if last.status != _lib.ST_RUNNING:
            break
        if slots > cap:
            raise _lib.HipSolverError("allreduce_minimize: slot budget exceeded")
        nb = max(1, min(batch, int(max_iter) - int(last.iters) + 2))
        for _ in range(nb):
            backend.step_partial()
            if allreduce is not None:
                allreduce()
            backend.step_finish()
        slots += nb
    return backend.end(W)
