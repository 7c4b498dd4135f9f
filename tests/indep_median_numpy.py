"""Plain-numpy restatement of the device median of csrc/indep.hip (`indep_median_kernel`), step for
step: sort the column, count the sorted-order differences <= t by one binary search per row,
bisect t over the bit pattern of the non-negative doubles, square, and take numpy's rule for an
even count (tests/test_indep_median_cpu.py, tests/test_gpu_indep_device.py)."""
import numpy as np

INF_BITS = 0x7FF0000000000000


def _from_bits(b):
    return np.array([b], dtype=np.uint64).view(np.float64)[0]


def prefix_lengths(xs, t):
    """Per row a of the sorted column: #{b > a : fl(xs[b] - xs[a]) <= t}, by binary search (the
    differences are non-decreasing in b)."""
    n = len(xs)
    a = np.arange(n - 1)
    lo, hi = a + 1, np.full(n - 1, n)
    while True:
        act = lo < hi
        if not act.any():
            return lo - (a + 1)
        mid = (lo + hi) >> 1
        with np.errstate(over="ignore"):
            le = xs[np.minimum(mid, n - 1)] - xs[a] <= t
        lo = np.where(act & le, mid + 1, lo)
        hi = np.where(act & ~le, mid, hi)


def count_le(xs, t):
    return int(prefix_lengths(xs, t).sum())


def kth_difference(xs, k):
    """The k-th smallest (from 0) sorted-order difference: the smallest non-negative double t with
    count_le(t) >= k + 1."""
    lo, hi = 0, INF_BITS
    while lo < hi:
        mid = lo + ((hi - lo) >> 1)
        if count_le(xs, _from_bits(mid)) >= k + 1:
            hi = mid
        else:
            lo = mid + 1
    return _from_bits(lo)


def select_median(x):
    """np.median of the squared differences of all pairs of entries of x, without forming them."""
    xs = np.sort(np.asarray(x, dtype=np.float64).ravel())
    n = len(xs)
    M = n * (n - 1) // 2
    with np.errstate(over="ignore", under="ignore"):
        if M & 1:
            v = kth_difference(xs, M // 2)
            return v * v
        v = kth_difference(xs, M // 2 - 1)
        p = prefix_lengths(xs, v)
        w = v
        if int(p.sum()) <= M // 2:  # the next element is the smallest difference above v
            a = np.arange(n - 1)
            nxt = a + 1 + p
            ok = nxt < n
            w = (xs[nxt[ok]] - xs[a[ok]]).min()
        return (v * v + w * w) / 2.0


def select_sigma2(x):
    med = select_median(x)
    return float(med) if med > 0 else 1.0


def columns(n, seed=0):
    """name -> column of length n: the data families of the median tests."""
    rng = np.random.default_rng(seed + n)
    z = rng.standard_normal(n)
    two = np.where(rng.random(n) < 0.5, -1.5, 2.25)
    pm0 = np.where(np.arange(n) % 2 == 0, 0.0, -0.0)
    return {
        "normal": z,
        "tied": np.round(2.0 * z) / 2.0,          # ties at the median
        "tiny": z * 1e-160,                       # squares underflow to subnormals and 0
        "lognormal": np.exp(3.0 * z),
        "constant": np.full(n, 3.0),              # median 0 -> 1.0
        "signed_zero": pm0,                       # +0.0 and -0.0 only
        "two_valued": two,
    }
