"""The selection csrc/indep.hip's median kernel performs, restated in numpy
(tests/indep_median_numpy.py), equals np.median of the reference's off-diagonal squared differences
(tests/indep_numpy.py::median_sigma2, notreks/mi_tests.py:39-44) bit for bit.  No GPU: this pins the
algorithm; tests/test_gpu_indep_device.py pins the kernel to `mi_tests.median_sigma2`."""
import numpy as np
import pytest

from tests import indep_median_numpy as imn
from tests import indep_numpy as inp
from midagma_amd import mi_tests as mi

SIZES = (2, 3, 4, 5, 6, 7, 64, 65, 97, 257, 1000)
KINDS = ("normal", "tied", "tiny", "lognormal", "constant", "signed_zero", "two_valued")


def _reference_median(x):
    D2 = (x[:, None] - x[None, :]) ** 2
    return np.median(D2[np.triu_indices(len(x), k=1)])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_selection_equals_numpy_median(kind, n):
    x = imn.columns(n)[kind]
    got, want = imn.select_median(x), _reference_median(x)
    assert np.array([got]).tobytes() == np.array([want]).tobytes()
    assert imn.select_sigma2(x) == inp.median_sigma2(x) == mi.median_sigma2(x)


def test_constant_column_gives_one():
    assert imn.select_median(np.full(7, 3.0)) == 0.0 and imn.select_sigma2(np.full(7, 3.0)) == 1.0


def test_even_count_takes_the_next_difference_when_the_lower_middle_is_unique():
    # n = 4: M = 6, differences 1 1 2 3 4 5 -> squares 1 1 4 9 16 25, median (4 + 9) / 2
    x = np.array([0.0, 1.0, 2.0, 5.0])
    assert sorted(abs(a - b) for i, a in enumerate(x) for b in x[i + 1:]) == [1, 1, 2, 3, 4, 5]
    assert imn.select_median(x) == 6.5 == _reference_median(x)
    # ... and the same element again when it is tied: 0 1 1 1 1 2 -> (1 + 1) / 2
    y = np.array([0.0, 1.0, 1.0, 2.0])
    assert imn.select_median(y) == 1.0 == _reference_median(y)


def test_new_entries_refuse_bad_arguments_before_any_device():
    from midagma_amd import _lib
    L = _lib.load()
    assert L.midagma_indep_set_data_dev(None, None, 10, 2, 2, None) == _lib.E_ARG
    assert L.midagma_indep_median_bandwidths(None, None, 0, None) == _lib.E_ARG
    assert L.midagma_indep_bandwidth_profile(None, None) == _lib.E_ARG
    assert b"null handle" in L.midagma_indep_last_error(None) or b"bad arguments" in L.midagma_indep_last_error(None)
    X = np.random.default_rng(0).standard_normal((10, 3))
    with pytest.raises(ValueError, match="bandwidths"):
        mi.permutation_null(X, [(0, 1)], bandwidths="gpu")


def test_prefix_counts_are_the_brute_force_counts():
    xs = np.sort(imn.columns(97)["lognormal"])
    diffs = np.concatenate([xs[a + 1:] - xs[a] for a in range(len(xs) - 1)])
    for t in (0.0, np.median(diffs), diffs.max(), np.inf):
        assert imn.count_le(xs, t) == int((diffs <= t).sum())
    # the monotonicity the binary search relies on
    assert all((np.diff(xs[a + 1:] - xs[a]) >= 0).all() for a in range(len(xs) - 1))
