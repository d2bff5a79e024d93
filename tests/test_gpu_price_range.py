"""acl_price's range test (csrc/common.h): the fast path is taken for
kPriceHiLo <= high dword of x < kPriceHiHi, one unsigned compare, where it
was 1e-6 < x < 1e60. Both constants lie inside the old interval, so the
admitted set is a subset of the old one and every x that newly fails takes the
IEEE expression, which is the reference.

On the GPU, through the acl_price test hook: the fast result equals getPrice's
float, (float)(1.0 / (sqrt(x) + 1e-8)) with IEEE operations, bit for bit, on
+-64 ulp around 1e-6, 1e60 and the two doubles the constants stand for, on the
values the test must reject (0, -0, the smallest subnormal, DBL_MIN, inf, -1,
NaN) and on 2^16 log-uniform samples. On the host: where the constants lie."""
import ctypes as ct

import numpy as np
import pytest

# csrc/common.h kPriceHiLo, kPriceHiHi
HI_LO, HI_HI = 0x3EB0C6F8, 0x4C63E9E4


def _dbl(hi):
    """The double whose high dword is hi and whose low dword is 0."""
    return np.array([hi << 32], np.uint64).view(np.float64)[0]


def _ieee(x):
    with np.errstate(all="ignore"):
        return (1.0 / (np.sqrt(np.asarray(x, np.float64)) + 1e-8)).astype(np.float32)


def _around(v, k=64):
    """The 2 k + 1 doubles within k ulp of v > 0 (bit patterns are ordered)."""
    c = int(np.array([v], np.float64).view(np.uint64)[0])
    return np.arange(c - k, c + k + 1, dtype=np.uint64).view(np.float64)


def _admitted(x):
    """The new range test, restated on the host."""
    hi = (np.asarray(x, np.float64).view(np.uint64) >> np.uint64(32)).astype(np.uint32)
    return (hi - np.uint32(HI_LO)) < np.uint32(HI_HI - HI_LO)


def _inputs():
    rng = np.random.RandomState(23)
    special = np.array([0.0, -0.0, 5e-324, np.finfo(np.float64).tiny, np.inf, -1.0, np.nan])
    return np.concatenate([_around(1e-6), _around(1e60), _around(_dbl(HI_LO)),
                           _around(_dbl(HI_HI)), special,
                           10.0 ** rng.uniform(-12, 70, 1 << 16)])


def _sweep(x):
    import torch
    from aclswarm_amd import _lib as L
    dev = torch.device("cuda:0")
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float64)).to(dev)
    fast = torch.empty(len(x), dtype=torch.float32, device=dev)
    ieee = torch.empty(len(x), dtype=torch.float32, device=dev)
    rc = L.lib().acl_internal_price_sweep(ct.c_void_p(xd.data_ptr()), ct.c_void_p(fast.data_ptr()),
                                          ct.c_void_p(ieee.data_ptr()), len(x))
    assert rc == 0
    return fast.cpu().numpy(), ieee.cpu().numpy()


@pytest.mark.gpu
def test_price_range_edges_bit_equal(cuda):
    x = _inputs()
    fast, ieee_gpu = _sweep(x)
    want = _ieee(x)
    for got in (ieee_gpu, fast):  # (the device's IEEE expression is the host's)
        nan = np.isnan(want)
        assert (np.isnan(got) == nan).all()
        bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)) & ~nan)
        assert bad.size == 0, (bad.size, x[bad[:5]], got[bad[:5]], want[bad[:5]])


def test_constants_lie_inside_the_old_interval():
    lo, hi = _dbl(HI_LO), _dbl(HI_HI)
    assert 1e-6 < lo < hi < 1e60
    # the nearest such words: one less at the low end is not above 1e-6, one
    # more at the high end admits doubles above 1e60
    assert _dbl(HI_LO - 1) <= 1e-6 and _dbl(HI_HI + 1) > 1e60


def test_admitted_set_is_a_subset_of_the_old_one():
    x = _inputs()
    new = _admitted(x)
    with np.errstate(invalid="ignore"):
        old = (x > 1e-6) & (x < 1e60)
    assert not (new & ~old).any()
    assert new.any() and (old & ~new).any()  # (the sweep reaches both sides of each edge)
    # the edges of the admitted set, exactly
    lo, hi = _dbl(HI_LO), _dbl(HI_HI)
    assert _admitted([lo])[0] and not _admitted([np.nextafter(lo, 0.0)])[0]
    assert not _admitted([hi])[0] and _admitted([np.nextafter(hi, 0.0)])[0]
    # what must fail: the sign bit, NaN, inf, zero, subnormals
    rej = np.array([0.0, -0.0, 5e-324, np.finfo(np.float64).tiny, np.inf, -np.inf, -1.0, -1e-3,
                    np.nan, -np.nan, 2.2e-308 / 4])
    assert not _admitted(rej).any()
