"""The device permutations of the dCor and HSIC engines come from one place (csrc/coltest.h:
perm_keys_kernel and PermSort): the two engines make the same permutations for the same seed, pair
and count, and the inverse is one.  n = 257 is the first n with a second workgroup of the keys
kernel."""
import numpy as np
import pytest

from midagma_amd.solver import HipDcor, HipHsic

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [5, 257])
def test_dcor_and_hsic_make_the_same_device_permutations(n):
    X = np.random.default_rng(n).standard_normal((n, 2))
    seed, q, P = 0xFEDCBA9876543210, 3, 4
    dc, hs = HipDcor(X), HipHsic(X)
    try:
        pd, inv = dc.device_perms(q, P, seed, inverse=True)
        plain = dc.device_perms(q, P, seed)
        ph = hs.device_perms(q, P, seed)
    finally:
        dc.close()
        hs.close()
    rows = np.tile(np.arange(n, dtype=np.int32), (P, 1))
    assert pd.shape == ph.shape == (P, n) and pd.dtype == ph.dtype == np.int32
    assert np.array_equal(np.sort(pd, axis=1), rows)  # every row is a permutation
    assert np.array_equal(pd, ph) and np.array_equal(pd, plain)
    assert np.array_equal(np.take_along_axis(inv, pd, 1), rows) and np.array_equal(np.take_along_axis(pd, inv, 1), rows)
