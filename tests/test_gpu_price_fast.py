"""acl_price's fast path (csrc/common.h: the hardware reciprocal square root,
one Newton step, the IEEE expression near float rounding midpoints and
outside the range) against getPrice's float, (float)(1.0 / (sqrt(x) + 1e-8))
with IEEE operations, evaluated on the host in numpy: bit for bit, through
the acl_price test hook.

Inputs: 2^20 log-uniform x in [1e-12, 1e70]; the edges of the fast path's
range (0, the smallest subnormal, 1e-6 and 1e60 with their neighbours, inf,
NaN); and x built so that the exact price lies 1, 100, 1000 and 5000 ulps of a
double on either side of a float rounding midpoint -- inside and outside the
window in which the fast path yields to the IEEE expression -- or as close to
one as a double x gets. The built inputs are found on the host in exact
arithmetic, and the tests without the gpu mark check on the host that they
lie where they should and that the IEEE expression puts the two sides on the
two neighbouring floats."""
import ctypes as ct
from decimal import Decimal, getcontext

import numpy as np
import pytest

OFFSETS = (1, 100, 1000, 5000)
getcontext().prec = 60
_C = Decimal(1e-8)  # the double constant, exactly


def _ieee(x):
    """getPrice's float with IEEE double operations (numpy: sqrt, the sum and
    the quotient each correctly rounded), then one rounding to f32."""
    with np.errstate(all="ignore"):
        return (1.0 / (np.sqrt(np.asarray(x, np.float64)) + 1e-8)).astype(np.float32)


def _exact_y(x):
    return 1 / (Decimal(float(x)).sqrt() + _C)


def _offset_ulps(x, mid):
    """The exact price of x less the midpoint, in ulps of the double mid."""
    return float((_exact_y(x) - Decimal(float(mid))) / Decimal(float(np.spacing(mid))))


_built = {}


def _midpoint_inputs():
    """{(float index, signed offset): (x, mid, lower float)}: for 48 floats f
    over [1e-3, 1e3] (and both ends of a binade) and the midpoint m of f and
    the next float, the double x whose exact price is nearest to m + k ulp(m),
    searched among the neighbours of the rounded solution."""
    if _built:
        return _built
    rng = np.random.RandomState(11)
    fs = list((10.0 ** rng.uniform(-3, 3, 46)).astype(np.float32))
    fs += [np.float32(1.0), np.nextafter(np.float32(2.0), np.float32(0))]
    for i, f in enumerate(fs):
        up = np.nextafter(f, np.float32(np.inf))
        mid = (np.float64(f) + np.float64(up)) / 2  # exact: 25 significant bits
        for k in (0,) + OFFSETS + tuple(-o for o in OFFSETS):
            yt = Decimal(float(mid)) + k * Decimal(float(np.spacing(mid)))
            x0 = np.float64((1 / yt - _C) ** 2)
            cand = [x0]
            for _ in range(6):
                cand = [np.nextafter(cand[0], 0.0)] + cand + [np.nextafter(cand[-1], np.inf)]
            x = min(cand, key=lambda c: abs(_offset_ulps(c, mid) - k))
            _built[(i, k)] = (float(x), float(mid), f)
    return _built


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


def _assert_bit_equal(x, got, want):
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all()
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)) & ~nan)
    assert bad.size == 0, (bad.size, x[bad[:5]], got[bad[:5]], want[bad[:5]])


def _edges():
    e = [0.0, 5e-324, np.inf, np.nan]
    for v in (1e-6, 1e60):
        e += [np.nextafter(v, 0.0), v, np.nextafter(v, np.inf)]
    return np.array(e)


@pytest.mark.gpu
def test_price_sweep_and_edges_bit_equal(cuda):
    rng = np.random.RandomState(17)
    x = np.concatenate([10.0 ** rng.uniform(-12, 70, 1 << 20), _edges()])
    fast, ieee_gpu = _sweep(x)
    want = _ieee(x)
    _assert_bit_equal(x, ieee_gpu, want)  # (the device's IEEE expression is the host's)
    _assert_bit_equal(x, fast, want)


@pytest.mark.gpu
def test_price_near_float_midpoints_bit_equal(cuda):
    x = np.array([v[0] for v in _midpoint_inputs().values()])
    fast, _ = _sweep(x)
    _assert_bit_equal(x, fast, _ieee(x))


@pytest.mark.gpu
def test_rsq_start_within_the_error_acl_price_assumes(cuda):
    """The one-step fast path is derived for a start within 2^-23 relative
    (the comment above acl_price): the raw instruction, on a sample of the
    fast path's range and every binade edge."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "scripts"))
    import rsq_f64_error as R
    x, _ = R.inputs(1 << 16, seed=3)
    err = R.rel_error(x, R.rsq_gpu(x))
    print("largest relative error of v_rsq_f64: %.4e" % err.max())
    assert err.max() <= 2.0 ** -23


def test_built_inputs_lie_at_their_offsets():
    for (i, k), (x, mid, f) in _midpoint_inputs().items():
        # a step of x moves the exact price by 1/4 to 1 ulp of the midpoint
        assert abs(_offset_ulps(x, mid) - k) <= 0.5, (i, k, x)
        assert 1e-6 < x < 1e60


def test_ieee_expression_lands_on_both_sides():
    """Below the midpoint the IEEE expression gives the lower float, above it
    the next one. Its three roundings are worth up to 1.5 ulp, so at 1 ulp
    (and at 0) it may land on either: there both floats must occur over the
    set."""
    B = _midpoint_inputs()
    n = len(B) // (2 * len(OFFSETS) + 1)
    seen = {-1: set(), 0: set(), 1: set()}
    for i in range(n):
        f = B[(i, 1)][2]
        up = np.nextafter(f, np.float32(np.inf))
        for k in OFFSETS[1:]:
            assert _ieee(B[(i, -k)][0]) == f, (i, -k)
            assert _ieee(B[(i, k)][0]) == up, (i, k)
        for k in seen:
            got = _ieee(B[(i, k)][0])
            assert got in (f, up)
            seen[k].add(bool(got == up))
    assert seen[0] == {False, True}
    assert False in seen[-1] and True in seen[1]


def test_edges_take_the_ieee_values():
    got = _ieee(_edges())
    assert got[0] == np.float32(1e8) and got[1] == np.float32(1e8)
    assert got[2] == 0 and np.isnan(got[3])
