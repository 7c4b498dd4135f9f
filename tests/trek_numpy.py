"""Long-double restatement of the PST trek penalty (notreks `pst` / `trek_value_grad`) for the
tests of csrc/trek.hip -- TEST INFRASTRUCTURE ONLY, numpy alone (no torch, no autograd).

    W2 = W o W,  F = f(W2),  H = F^T F,  v_p = H[i_p, j_p],  value = agg(v),  grad = d value / d W

Written naively and on purpose unlike the kernel (and unlike oracle/trek_oracle.py):

  f     exp    scale by 2^-k until ||A||_1 <= 2^-6, degree-30 Taylor by Horner, k squarings
        inv    Gauss-Jordan with partial pivoting on (1 + eps) I - A
        log    the plain power sum I + sum_{k<=K} A^k / k
        binom  p - 1 repeated products of I + A
  grad  C = d value / d H,  S = C + C^T,  G_F = F S.  For a power series f the top-right block of
        f([[A, E], [0, A]]) is the Frechet derivative L_f(A, E), and its adjoint in E is
        L_f(A^T, .), so  d value / d W2 = L_f(W2^T, G_F)  and  grad = 2 W o that:  one more
        evaluation of the same naive f on a 2d x 2d matrix, no recurrence of the kernel restated.
        L_f is linear in the direction, so the direction is normalised first (sigma below):
        unnormalised, exp's scaling would follow ||G_F|| instead of ||W2|| and lose digits --
        the defect of an autograd oracle at large norm.

np.longdouble products have no BLAS: this is a reference for d <= 65.

The second half of the file builds the inputs that tests/test_trek_numpy_cpu.py (which certifies
this restatement and, where it is used, the oracle) and tests/test_gpu_trek_shapes.py share.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble

THETA = 0.25   # csrc/trek.hip trek_scale_kernel: scale until ||X||_1 <= THETA ...
SMAX = 12      # ... with at most TREK_SMAX squarings (launch.h)


def _norm1(A):
    return np.abs(A).sum(axis=0).max()


def _exp(A):
    n = A.shape[0]
    k = 0
    nrm = _norm1(A)
    while nrm > LD(2.0) ** -6:
        nrm = nrm / 2
        k += 1
    X = A / LD(2.0) ** k
    eye = np.eye(n, dtype=LD)
    P = eye.copy()
    for j in range(30, 0, -1):
        P = eye + (X @ P) / LD(j)
    for _ in range(k):
        P = P @ P
    return P


def _inv(A, eps):
    n = A.shape[0]
    M = np.concatenate([(LD(1.0) + LD(eps)) * np.eye(n, dtype=LD) - A, np.eye(n, dtype=LD)], axis=1)
    for c in range(n):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        if p != c:
            M[[c, p]] = M[[p, c]]
        M[c] = M[c] / M[c, c]
        col = M[:, c].copy()
        col[c] = 0
        M -= col[:, None] * M[c][None, :]
    return M[:, n:].copy()


def _log(A, K):
    n = A.shape[0]
    out = np.eye(n, dtype=LD)
    P = np.eye(n, dtype=LD)
    for k in range(1, K + 1):
        P = P @ A
        out = out + P / LD(k)
    return out


def _binom(A, p):
    B = np.eye(A.shape[0], dtype=LD) + A
    out = B
    for _ in range(p - 1):
        out = out @ B
    return out


def f_ld(A, seq, d, K_log=None, eps_inv=1e-8):
    """f(A) in long double; `d` is the node count (log's default K = 2d and binom's power d),
    which is not A's size when A is the 2d x 2d block matrix of the gradient."""
    if seq == "exp":
        return _exp(A)
    if seq == "inv":
        return _inv(A, eps_inv)
    if seq == "log":
        return _log(A, 2 * d if K_log is None else int(K_log))
    if seq == "binom":
        return _binom(A, d)
    raise ValueError(seq)


def pair_values_ld(W, pairs, seq, K_log=None, eps_inv=1e-8):
    """(F, v): f(W o W) and the pair values H[i_p, j_p], long double."""
    W = np.asarray(W, dtype=LD)
    P = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    F = f_ld(W * W, seq, W.shape[0], K_log, eps_inv)
    H = F.T @ F
    return F, H[P[:, 0], P[:, 1]]


def agg_ld(v, agg):
    """(value, c) with c_p = d value / d v_p."""
    m = len(v)
    if agg == "mean":
        return v.sum() / LD(m), np.full(m, LD(1.0) / LD(m), dtype=LD)
    if agg == "sum":
        return v.sum(), np.ones(m, dtype=LD)
    if agg == "max":
        mx = v.max()
        ties = v == mx
        return mx, ties.astype(LD) / LD(int(ties.sum()))   # torch's even split over the ties
    if agg == "lse":
        mx = v.max()
        e = np.exp(v - mx)
        return mx + np.log(e.sum()), e / e.sum()
    raise ValueError(agg)


def pst_value_ld(W, pairs, seq, agg, K_log=None, eps_inv=1e-8):
    """The value alone, as a long double (W may be long double: central differences)."""
    _, v = pair_values_ld(W, pairs, seq, K_log, eps_inv)
    return agg_ld(v, agg)[0]


def pst_value_grad_ld(W, pairs, seq, agg, K_log=None, eps_inv=1e-8):
    """(value, grad) of the PST penalty, computed in np.longdouble and returned as such."""
    W = np.asarray(W, dtype=LD)
    d = W.shape[0]
    P = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    F, v = pair_values_ld(W, P, seq, K_log, eps_inv)
    value, c = agg_ld(v, agg)
    C = np.zeros((d, d), dtype=LD)
    np.add.at(C, (P[:, 0], P[:, 1]), c)
    GF = F @ (C + C.T)
    W2 = W * W
    gmax, wmax = np.abs(GF).max(), np.abs(W2).max()
    if gmax == 0:
        return value, np.zeros((d, d), dtype=LD)
    sigma = gmax / wmax if wmax > 0 else LD(1.0)
    M = np.zeros((2 * d, 2 * d), dtype=LD)
    M[:d, :d] = W2.T
    M[d:, d:] = W2.T
    M[:d, d:] = GF / sigma
    L = f_ld(M, seq, d, K_log, eps_inv)[:d, d:]
    return value, LD(2.0) * W * (sigma * L)


# ---- inputs shared by the CPU certification and the GPU tests ------------------------------------

def norm1_w2(W) -> float:
    """||W o W||_1 (largest column sum) in float64, the quantity trek_scale_kernel thresholds."""
    W = np.asarray(W, dtype=np.float64)
    return float((W * W).sum(axis=0).max())


def squaring_count(W) -> int:
    """The exp path's squaring count by the kernel's rule: the smallest s <= SMAX with
    ||W o W||_1 / 2^s <= THETA."""
    nrm, s = norm1_w2(W), 0
    while s < SMAX and nrm / 2.0 ** s > THETA:
        s += 1
    return s


def sparse_w(d: int, norm: float, seed: int = 0, upper: bool = False, equal_columns: bool = False) -> np.ndarray:
    """Random W at about 3/d density with a zero diagonal, rescaled to ||W o W||_1 = norm
    (`upper`: strictly upper triangular, a DAG).  `equal_columns`: every non-empty column of
    W o W is scaled to the sum `norm`, which makes the spectral radius of W o W equal its 1-norm:
    the powers of W o W, and with them a Taylor remainder, are then as large as the norm allows
    (scaled as a whole, a sparse random W o W has a spectral radius of about a third of it)."""
    rng = np.random.default_rng(1000 * d + seed)
    W = rng.uniform(-1.0, 1.0, (d, d)) * (rng.uniform(size=(d, d)) < min(1.0, 3.0 / d))
    np.fill_diagonal(W, 0.0)
    if upper:
        W = np.triu(W, 1)
    if not W.any():                      # tiny d: make sure there is an edge
        W[0, d - 1] = 0.7
    if equal_columns:
        c = (W * W).sum(axis=0)
        W = W * np.sqrt(norm / np.where(c > 0, c, norm))[None, :]
    return W * np.sqrt(norm / norm1_w2(W))


def bucket_norms():
    """[(s, edge, ||W o W||_1)]: both edges of the squaring buckets s in {0, 1, 2, 4, 6, 9} and the
    lower edge of s = SMAX (norm ~ 517; the value is ~1e171 there and the upper edge overflows)."""
    out = []
    for s in (0, 1, 2, 4, 6, 9):
        out.append((s, "hi", THETA * 2.0 ** s * 0.99))
        out.append((s, "lo", THETA * 2.0 ** (s - 1) * 1.01))
    out.append((SMAX, "lo", THETA * 2.0 ** (SMAX - 1) * 1.01))
    return out


def upper_pairs(d: int, frac: float, seed: int = 0) -> np.ndarray:
    """A random subset of the strict upper triangle (no duplicates, no mirrored pairs)."""
    rng = np.random.default_rng(77 * d + seed)
    iu = np.array(np.triu_indices(d, 1)).T
    P = iu[rng.uniform(size=len(iu)) < frac]
    return P if len(P) else iu[:1]


def ordered_pairs(d: int) -> np.ndarray:
    """Every (i, j), i != j: what `undirected=False` produces (mirrored pairs)."""
    i, j = np.nonzero(~np.eye(d, dtype=bool))
    return np.stack([i, j], axis=1)


def squaring_case(d: int, norm: float):
    """(W, pairs) of a squaring-count cell.  Up to ||W o W||_1 = 4 (s <= 4) with equal column
    sums, so that at the upper edge of a bucket the scaled matrix has spectral radius 0.2475 and
    the degree-12 Taylor polynomial is used to its limit: measured on the CPU, a degree-6
    polynomial then moves the value by 4e-10 to 4e-7 of max(1, |v|), against 2e-14 to 6e-12 for W
    scaled as a whole.  Above 4 W is scaled as a whole: the value grows like exp(2 rho), and a
    spectral radius of 517 would overflow double where the kernel's domain does not end."""
    return sparse_w(d, norm, seed=1, equal_columns=norm <= 4), upper_pairs(d, 0.3, seed=1)


def threshold_case(d: int):
    """||W o W||_1 = THETA exactly (a single entry 0.5): either count is legitimate."""
    W = np.zeros((d, d))
    W[1, 3] = 0.5
    return W, np.array([[1, 3], [0, 3], [3, 1], [2, 5]])


def tie_case(d: int, all_zero: bool):
    """Structural ties under `max`: W strictly upper triangular and f a sum of products of
    non-negatives (log, binom), so H[i, j] = sum_k F[k, i] F[k, j] is an exact 0 in any arithmetic
    whenever no k reaches both i and j.  Pairs with H = 0, plus (unless all_zero) one positive
    pair.  Returns (W, pairs, number of H = 0 pairs)."""
    W = sparse_w(d, 0.8, seed=2, upper=True)
    R = np.eye(d, dtype=bool) | (W != 0)
    for _ in range(d):                                   # reachability closure (DAG: d steps do)
        R = R | ((R.astype(np.int64) @ R.astype(np.int64)) > 0)
    common = (R.T.astype(np.int64) @ R.astype(np.int64)) > 0   # some k reaches both i and j
    zi, zj = np.nonzero(~common)
    zeros = np.stack([zi, zj], axis=1)[:9]
    assert len(zeros) >= 4, "tie_case: W leaves too few unreachable pairs"
    if all_zero:
        return W, zeros, len(zeros)
    pi, pj = np.nonzero(np.triu(W != 0, 1))
    pos = np.array([[pi[0], pj[0]]])                     # an edge i -> j: k = i reaches both
    return W, np.concatenate([zeros[:4], pos, zeros[4:]]), len(zeros)


def dyadic_tie_case(d: int):
    """Ties at a positive maximum with a non-zero gradient: two isolated edges of weight +-1/2.
    W o W has the two entries 1/4 and a zero square, so log gives F = I + W o W and binom
    F = I + d (W o W), every entry a small dyadic number that float64 holds exactly in any
    summation order: H is 1/4 (log) or d/4 (binom) at both edges, bit for bit, on any machine.
    The two edges share the gradient evenly; a third pair, with H = 0, must stay out of it."""
    W = np.zeros((d, d))
    W[0, 2] = 0.5
    W[d - 3, d - 1] = -0.5
    return W, np.array([[0, 2], [1, 4], [d - 3, d - 1]])


AGGS = ("mean", "sum", "max", "lse")
SEQS = ("exp", "inv", "log", "binom")

# (solver mode, d, padded D, seqs): the shape cells of tests/test_gpu_trek_shapes.py.  D is what
# midagma_create pads d to (asserted there); binom (d - 1 products in the oracle, values like
# exp(d ||W o W||_1)) stays at d <= 300.
SHAPE_CELLS = (
    ("cov", 64, 64, SEQS),            # d == D
    ("cov", 33, 64, SEQS),            # log at its default K = 2d = 66
    ("cov", 65, 128, SEQS),           # mostly padding
    ("cov", 128, 128, SEQS),          # d == D
    ("cov", 129, 256, SEQS),          # gemm_dd split 2
    ("cov", 255, 256, SEQS),          # binom: all bits set
    ("cov", 256, 256, SEQS),          # binom: a single bit, d == D
    ("cov", 257, 512, SEQS),          # split 4
    ("cov", 700, 768, SEQS[:3]),      # split 4 at 6 x 6 tiles
    ("data", 150, 192, SEQS),         # D not a multiple of 128: split 1 on a ragged tile grid
    ("data", 300, 384, SEQS),         # split 3
    ("cov", 1930, 2048, ("inv",)),    # 256 tiles: split 1, no slice buffer
    ("cov", 7, 64, ("binom",)),       # binom: all bits set, small
    ("cov", 31, 64, ("binom",)),
)
LD_MAX_D = 65   # the long-double restatement judges d <= 65, the (certified) oracle above


def shape_cell_agg(cell: int, seq: str) -> str:
    """The aggregators rotate over cells and seqs: every (seq, agg) occurs at some D >= 128."""
    return AGGS[(cell + SEQS.index(seq)) % 4]


def shape_cell_klog(d: int, seq: str):
    return None if seq != "log" or d == 33 else 7


def shape_case(d: int, seq: str):
    """(W, pairs) of a shape cell.  ||W o W||_1: exp 3 (four squarings; the oracle is certified
    up to 8), inv 0.7 (spectral radius below 1), log 0.9, binom 8 / d."""
    norm = {"exp": 3.0, "inv": 0.7, "log": 0.9, "binom": 8.0 / d}[seq]
    return sparse_w(d, norm, seed=3), upper_pairs(d, min(0.3, 8000.0 / (d * d)), seed=3)


def pairlist_cases(d: int = 20):
    """{name: (W, pairs, seq, aggs)}: the pair-list edges at small d (long-double reference)."""
    W = sparse_w(d, 1.5, seed=4)
    base = upper_pairs(d, 0.3, seed=4)
    tiled = np.concatenate([base, base[::-1, ::-1]])          # mirrored too
    tiled = np.resize(tiled, (70001, 2))                      # duplicates, m > 65536
    diag = np.concatenate([base[:5], [[4, 4]], base[5:9], [[4, 4]]])
    Wt, Pt, _ = tie_case(d, False)
    Wz, Pz, _ = tie_case(d, True)
    Wd, Pd = dyadic_tie_case(d)
    return {
        "single": (W, base[3:4], "exp", AGGS),
        "ordered-exp": (W, ordered_pairs(d), "exp", ("max", "lse")),
        "ordered-inv": (sparse_w(d, 0.7, seed=4), ordered_pairs(d), "inv", ("max", "lse")),
        "diagonal": (W, diag, "exp", AGGS),
        "tiled": (W, tiled, "exp", AGGS),
        "ties-log": (Wt, Pt, "log", ("max",)),
        "ties-binom": (Wt * np.sqrt(0.4 / 0.8), Pt, "binom", ("max",)),
        "allzero-log": (Wz, Pz, "log", ("max", "lse")),
        "allzero-binom": (Wz * np.sqrt(0.4 / 0.8), Pz, "binom", ("max",)),
        "dyadic-log": (Wd, Pd, "log", ("max",)),
        "dyadic-binom": (Wd, Pd, "binom", ("max",)),
    }


# the cases that are about ties: name -> the least number of exact ties the restatement must see
TIE_CASES = {"tiled": 2, "ties-log": 2, "ties-binom": 2, "allzero-log": 2, "allzero-binom": 2,
             "dyadic-log": 2, "dyadic-binom": 2}


_REF = {}


def reference_ld(key, W, pairs, seq, agg, K_log=None):
    """pst_value_grad_ld computed once per `key` (a hashable name of the case) and shared,
    read-only, among the tests that need it."""
    if key not in _REF:
        v, g = pst_value_grad_ld(W, pairs, seq, agg, K_log)
        g.setflags(write=False)
        _REF[key] = (v, g)
    return _REF[key]
