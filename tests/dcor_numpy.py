"""Plain-numpy restatement of csrc/dcor.hip (tests/test_dcor_cpu.py, tests/test_gpu_dcor.py):
distance covariance of two columns without an n x n matrix ("dCor without the n^2 sum").

Row sums from the sorted column, S = sum_ab |x_a - x_b| |y_a - y_b| by x-blocks and y-bins of edge m
(terms (a) and (b) summed pair by pair within a block or bin, term (c) from the K x K cell sums of
1, x, y, xy and their inclusive 2-D prefix tables), the reference's biased statistic and the
bias-corrected one, the Philox-argsort device permutations and the chi-square p-value.  Vectorised:
O(n m) values in blocks, nothing n x n."""
import numpy as np

from tests.indep_numpy import philox4x32_10


def block_edge(n):
    """The library's rule: the power of two in [64, 1024] with m^2 >= n, else 1024."""
    m = 64
    while m < 1024 and m * m < n:
        m *= 2
    return m


def column_prep(x):
    """Per column: centred values, the stable argsort (-0.0 equal to +0.0), positions, row sums
    a_r. = sum_b |x_r - x_b|, and dvar^2 in both forms."""
    x = np.asarray(x, dtype=np.float64) + 0.0  # (-0.0 + 0.0 = +0.0: one key for both zeros)
    n = len(x)
    order = np.argsort(x, kind="stable")
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    xc = x - x.mean()
    xs = xc[order]
    # the running sums in long double: a serial float64 cumsum of a column with many ties rounds
    # the same way at every step and drifts (2.5e-13 in stat^2 at n = 4097)
    inc = np.cumsum(xs.astype(np.longdouble))
    tot = float(inc[-1])
    pre = np.concatenate([[0.0], inc[:-1]])
    rs = np.empty(n)
    rs[order] = (xs * (2.0 * np.arange(n) - n) + (inc[-1] - 2.0 * pre)).astype(np.float64)
    add, sxx, txx = rs.sum(), 2.0 * n * (xc * xc).sum() - 2.0 * tot * tot, (rs * rs).sum()
    dvar_b = sxx / n**2 - 2.0 * txx / n**3 + add * add / n**4
    dvar_u = (sxx / (n * (n - 3)) - 2.0 * txx / (n * (n - 2) * (n - 3)) +
              add * add / (n * (n - 1) * (n - 2) * (n - 3))) if n >= 4 else 0.0
    return dict(n=n, xc=xc, order=order, pos=pos, rs=rs, add=add, dvar_b=dvar_b, dvar_u=dvar_u,
                zero=bool(x.max() == x.min()))


def _within(key, x, y, other, m):
    """sum over ordered pairs (r, r') with key_r // m == key_r' // m (key a permutation of [0, n))
    of |dx| |dy|, restricted to other_r != other_r' when `other` is given."""
    n = len(key)
    K = -(-n // m)
    o = np.argsort(key, kind="stable")
    pad = K * m - n

    def grid(v, fill):
        return np.concatenate([v[o], np.full(pad, fill, dtype=v.dtype)]).reshape(K, m)

    X, Y = grid(x, 0.0), grid(y, 0.0)
    valid = grid(np.ones(n, dtype=bool), False)
    O = None if other is None else grid(other, -1)
    tot = 0.0
    step = max(1, (1 << 22) // (m * m))
    for k0 in range(0, K, step):
        sl = slice(k0, k0 + step)
        t = np.abs(X[sl, :, None] - X[sl, None, :]) * np.abs(Y[sl, :, None] - Y[sl, None, :])
        keep = valid[sl, :, None] & valid[sl, None, :]
        if O is not None:
            keep &= O[sl, :, None] != O[sl, None, :]
        tot += (t * keep).sum()
    return tot


def s_blocks(cx, cy, perm=None, m=0):
    """S = sum over ordered pairs of |x_r - x_r'| |y'_r - y'_r'| with y'_r = y[perm_r], by the
    decomposition with block edge m (0: the rule)."""
    n = cx["n"]
    m = m or block_edge(n)
    K = -(-n // m)
    pi = np.arange(n) if perm is None else np.asarray(perm, dtype=np.int64)
    x, y = cx["xc"], cy["xc"][pi]
    px, py = cx["pos"], cy["pos"][pi]
    blk, bn = px // m, py // m
    ab = _within(px, x, y, None, m) + _within(py, x, y, blk, m)
    M = np.zeros((4, K, K))
    for w, v in enumerate((np.ones(n), x, y, x * y)):
        np.add.at(M[w], (blk, bn), v)
    C = np.zeros((4, K + 1, K + 1))  # C[w, b, c] = sum over blocks < b and bins < c
    C[:, 1:, 1:] = M.cumsum(1).cumsum(2)
    ll = C[:, blk, bn]
    lg = C[:, blk, K] - C[:, blk, bn + 1]
    gl = C[:, K, bn] - C[:, blk + 1, bn]
    gg = C[:, K, K] [:, None] - C[:, blk + 1, K] - C[:, K, bn + 1] + C[:, blk + 1, bn + 1]
    g = ll + gg - lg - gl
    c = (x * y * g[0] - x * g[2] - y * g[1] + g[3]).sum()
    return ab + c


def dcov2(cx, cy, perm=None, m=0, unbiased=False):
    n = cx["n"]
    pi = np.arange(n) if perm is None else np.asarray(perm, dtype=np.int64)
    S = s_blocks(cx, cy, perm, m)
    T = (cx["rs"] * cy["rs"][pi]).sum()
    gg = cx["add"] * cy["add"]
    if unbiased:
        return S / (n * (n - 3)) - 2.0 * T / (n * (n - 2) * (n - 3)) + gg / (n * (n - 1) * (n - 2) * (n - 3))
    return S / n**2 - 2.0 * T / n**3 + gg / n**4


def stat_of(v, cx, cy, unbiased=False):
    """The returned statistic of the value v = dcov^2 or dcov^2_U."""
    if cx["zero"] or cy["zero"]:
        return 0.0
    vx, vy = (cx["dvar_u"], cy["dvar_u"]) if unbiased else (cx["dvar_b"], cy["dvar_b"])
    if vx <= 0 or vy <= 0:
        return 0.0
    return v / np.sqrt(vx * vy) if unbiased else np.sqrt(max(v, 0.0)) / np.sqrt(np.sqrt(vx * vy))


def r2_of(v, cx, cy, unbiased=False):
    """stat^2 for the biased form (R^2 = dcov^2 / sqrt(dvar_x^2 dvar_y^2)), R_U for the other: the
    quantity the 1e-12 bars are on."""
    vx, vy = (cx["dvar_u"], cy["dvar_u"]) if unbiased else (cx["dvar_b"], cy["dvar_b"])
    if cx["zero"] or cy["zero"] or vx <= 0 or vy <= 0:
        return 0.0
    return v / np.sqrt(vx * vy)


def dcor_null(X, pairs, perms=None, m=0, unbiased=False, prep=None):
    """(stat, ge, null, values): `mi_tests.dcor_null` for explicit perms (len(pairs), P, n) or none;
    values (len(pairs), P + 1) are the raw dcov^2 the count orders by."""
    X = np.asarray(X, dtype=np.float64)
    prep = prep if prep is not None else {}
    for v in set(np.asarray(pairs).ravel().tolist()):
        if v not in prep:
            prep[v] = column_prep(X[:, v])
    P = 0 if perms is None else perms.shape[1]
    stat, ge = np.zeros(len(pairs)), np.zeros(len(pairs), dtype=np.int64)
    null, vals = np.zeros((len(pairs), P)), np.zeros((len(pairs), P + 1))
    for q, (i, j) in enumerate(np.asarray(pairs).tolist()):
        cx, cy = prep[i], prep[j]
        if cx["zero"] or cy["zero"]:
            ge[q] = P
            continue
        vals[q, 0] = dcov2(cx, cy, None, m, unbiased)
        for p in range(P):
            vals[q, 1 + p] = dcov2(cx, cy, perms[q, p], m, unbiased)
        stat[q] = stat_of(vals[q, 0], cx, cy, unbiased)
        null[q] = [stat_of(v, cx, cy, unbiased) for v in vals[q, 1:]]
        ge[q] = int((vals[q, 1:] >= vals[q, 0]).sum())
    return stat, ge, null, vals


def philox_perms(seed, q, P, n):
    """The device permutations of pair q of a call, (P, n): pi = the stable argsort over a of
    (o0 << 32) | o1, o = Philox4x32-10(counter (q, p, a, 0), key (seed & 0xffffffff, seed >> 32))."""
    p, a = np.meshgrid(np.arange(P), np.arange(n), indexing="ij")
    o0, o1, _, _ = philox4x32_10(np.full_like(a, q), p, a, np.zeros_like(a), seed & 0xFFFFFFFF,
                                 (seed >> 32) & 0xFFFFFFFF)
    return np.argsort((o0 << np.uint64(32)) | o1, axis=1, kind="stable").astype(np.int32)


def chi2_pvalue(n, r_u):
    """Shen, Panda and Vogelstein: p = P(chi2_1 > n R_U + 1)."""
    from scipy import stats
    return stats.chi2.sf(n * np.asarray(r_u) + 1.0, 1)


# --- the reference's formulas by brute force (mi_tests.py:68-101) and U-centring ------------------
def brute_values(x, y):
    """(dcov^2, dvar_x^2, dvar_y^2) from the double-centred n x n distance matrices."""
    n = len(x)
    a, b = np.abs(x[:, None] - x[None, :]), np.abs(y[:, None] - y[None, :])
    A = a - a.mean(1, keepdims=True) - a.mean(0, keepdims=True) + a.mean()
    B = b - b.mean(1, keepdims=True) - b.mean(0, keepdims=True) + b.mean()
    return (A * B).sum() / n**2, (A * A).sum() / n**2, (B * B).sum() / n**2


def brute_values_u(x, y):
    """The same from the U-centred matrices (Szekely and Rizzo 2014), n >= 4."""
    n = len(x)

    def U(a):
        A = a - a.sum(1, keepdims=True) / (n - 2) - a.sum(0, keepdims=True) / (n - 2) + a.sum() / ((n - 1) * (n - 2))
        np.fill_diagonal(A, 0.0)
        return A

    A, B = U(np.abs(x[:, None] - x[None, :])), U(np.abs(y[:, None] - y[None, :]))
    return (A * B).sum() / (n * (n - 3)), (A * A).sum() / (n * (n - 3)), (B * B).sum() / (n * (n - 3))


def make_columns(kind, n, seed=0):
    """The data kinds of the dCor tests: (x, y)."""
    rng = np.random.default_rng(seed)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    if kind == "continuous":
        y = 0.5 * x + y
    elif kind == "rounded":
        x, y = np.round(2.0 * x), np.round(1.5 * y + x)
    elif kind == "binary":
        x, y = (x > 0).astype(float), (y + 0.5 * x > 0).astype(float)
    elif kind == "constant":
        y = np.full(n, 1.5)
    elif kind == "equal":
        y = x.copy()
    elif kind == "affine":
        y = 3.0 - 2.0 * x
    elif kind == "zeros":  # +0.0 and -0.0 mixed with a few other values
        x = np.where(x > 0.3, 0.0, np.where(x < -0.3, -0.0, np.round(x, 1)))
        y = y + x
    elif kind == "shifted":
        x, y = x + 1e3, np.sin(3.0 * x) + 0.2 * y
    else:
        raise ValueError(kind)
    return x, y


KINDS = ("continuous", "rounded", "binary", "constant", "equal", "affine", "zeros", "shifted")


def kind_matrices(n, seed=0):
    """Two n x 5 matrices whose columns cover the data kinds: continuous, rounded to integers, 0/1,
    constant, a copy (y = x); and 3 - 2 x, +0.0 / -0.0 mixed, shifted by 10^3, sin(3 x) + noise."""
    rng = np.random.default_rng(seed)
    x, z, w, u = (rng.standard_normal(n) for _ in range(4))
    A = np.column_stack([x, np.round(1.5 * z + x), (w > 0).astype(float), np.full(n, 1.5), x.copy()])
    zeros = np.where(u > 0.3, 0.0, np.where(u < -0.3, -0.0, np.round(u, 1)))
    B = np.column_stack([x, 3.0 - 2.0 * x, zeros, 0.3 * x + w + 1e3, np.sin(3.0 * x) + 0.2 * z])
    return [np.ascontiguousarray(A), np.ascontiguousarray(B)]


ALL_PAIRS_5 = [(i, j) for i in range(5) for j in range(i + 1, 5)]

# the n = 16384 case against the n^2 kernel: three columns, explicit permutations from this seed
BIG_N, BIG_P, BIG_SEED = 16384, 4, 11
BIG_PAIRS = [(0, 1), (0, 2), (1, 2)]


def big_case():
    rng = np.random.default_rng(BIG_SEED)
    x, y, z = (rng.standard_normal(BIG_N) for _ in range(3))
    X = np.ascontiguousarray(np.column_stack([x, 0.05 * x + y, np.sin(3.0 * x) + z]))
    perms = np.array([[rng.permutation(BIG_N) for _ in range(BIG_P)] for _ in BIG_PAIRS], dtype=np.int32)
    return X, perms


# chi-square cases: n, and seeds of independent pairs for which the restatement gives p > 0.05
CHI2_N, CHI2_SEEDS = 2000, (1, 2, 3)


def chi2_case(seed):
    """n x 3: x, an independent y, sin(3 x) + small noise."""
    rng = np.random.default_rng(seed)
    x, y, z = (rng.standard_normal(CHI2_N) for _ in range(3))
    return np.ascontiguousarray(np.column_stack([x, y, np.sin(3.0 * x) + 0.1 * z]))
