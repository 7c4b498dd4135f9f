"""Plain-numpy restatements for the independence-test suites (tests/test_indep_cpu.py,
tests/test_gpu_indep.py): the two identities csrc/indep.hip evaluates, the numpy permutation
stream, and the Philox4x32-10 device permutations ("Independence tests")."""
import numpy as np

CASES = ("c5", "c97", "c200", "c257", "c1000", "c96")
STATS = ("hsic", "dcor")


def median_sigma2(x):
    D2 = (x[:, None] - x[None, :]) ** 2
    med = np.median(D2[np.triu_indices(len(x), k=1)])
    return med if med > 0 else 1.0


def _centre(K):
    return K - K.mean(axis=1, keepdims=True) - K.mean(axis=0, keepdims=True) + K.mean()


def numpy_perms(seed, m, P, n):
    """(m, P, n): rng.permutation(n), P times per pair in pair order, from one default_rng(seed)."""
    rng = np.random.default_rng(seed)
    return np.array([[rng.permutation(n) for _ in range(P)] for _ in range(m)], dtype=np.int64).reshape(m, P, n)


def perm_guard(perms):
    n = perms.shape[-1]
    return (perms.astype(np.int64) * np.arange(1, n + 1, dtype=np.int64)).sum(axis=-1)


def pair_values(kind, x, y, perms):
    """(P + 1,) statistics of (x, y) and of (x, y[perm]) by the identities:
    HSIC = (1/n^2) sum Kc[a,b] exp(-(y_a - y_b)^2 / (2 sigma_y^2)) with Kc the centred Gram of x;
    dcov^2 = (1/n^2) sum Ax[a,b] |y_a - y_b| with Ax the centred distance matrix of x.
    A zero-range column gives zeros (the reference's centred matrix is exactly 0)."""
    n = len(x)
    ys = [y] + [y[p] for p in perms]
    if np.ptp(x) == 0 or np.ptp(y) == 0:
        return np.zeros(len(ys))
    if kind == "hsic":
        Kc = _centre(np.exp(-(x[:, None] - x[None, :]) ** 2 / (2.0 * median_sigma2(x))))
        s2 = median_sigma2(y)
        return np.array([(Kc * np.exp(-(v[:, None] - v[None, :]) ** 2 / (2.0 * s2))).sum() / (n * n) for v in ys])
    Ax = _centre(np.abs(x[:, None] - x[None, :]))
    Ay = _centre(np.abs(y[:, None] - y[None, :]))
    dvx, dvy = (Ax * Ax).sum() / (n * n), (Ay * Ay).sum() / (n * n)
    dcov2 = np.array([(Ax * np.abs(v[:, None] - v[None, :])).sum() / (n * n) for v in ys])
    if dvx <= 0 or dvy <= 0:
        return np.zeros(len(ys))
    return np.sqrt(np.maximum(dcov2, 0.0)) / np.sqrt(np.sqrt(dvx * dvy))


M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of 32-bit words held in uint64; returns the four output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for r in range(10):
        if r:
            k0, k1 = (k0 + w0) & M32, (k1 + w1) & M32
        p0, p1 = m0 * c0, m1 * c2
        hi0, lo0, hi1, lo1 = p0 >> s32, p0 & M32, p1 >> s32, p1 & M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    return c0, c1, c2, c3


def philox_perms(seed, m, P, n):
    """The device permutations: pi for (pair q, permutation p) = stable argsort over a of the key
    (((o0 << 32) | o1) & ~0x3fff) | a, o = Philox4x32-10(counter (q, p, a, 0), key (seed & 0xffffffff,
    seed >> 32))."""
    q, p, a = np.meshgrid(np.arange(m), np.arange(P), np.arange(n), indexing="ij")
    o0, o1, _, _ = philox4x32_10(q, p, a, np.zeros_like(a), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    key = (((o0 << np.uint64(32)) | o1) & ~np.uint64(0x3FFF)) | a.astype(np.uint64)
    return np.argsort(key, axis=2, kind="stable").astype(np.int32)
