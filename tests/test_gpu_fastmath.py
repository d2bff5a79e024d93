"""The default build's control fast-math on the device (csrc/common.h:
sqrt_nr1, its split sqrt_nr1_step / sqrt_nr1_edge, acl_atan_b and
acl_atan_b_vote) through the acl_internal_fastmath_sweep hook, against
np.sqrt / np.arctan on np.longdouble (63-bit mantissa) and, at the few hundred
boundary points, mpmath at 40 digits. tests/test_fastmath.py checks a numpy
model of the atan with an exact quotient; this is the device code itself: the
v_rcp_f64 start and its Newton step, the constants built in s[98:99], the row
index from float bits, the vote branch.

Bars. sqrt: 1.5 e0^2 + 4 u relative with e0 = 2^-23, the start error of
v_rsq_f64 that test_rsq_start_within_the_error_acl_price_assumes asserts (one
Goldschmidt step maps a start error e to 1.5 e^2; four roundings follow the
start): 2.2e-14. atan: the project's own figure, 1e-14 relative
(control_dev.h, ACL_GAIN_FASTMATH). The vote forms and the recombined sqrt
must have the bits of the plain ones."""
import ctypes as ct

import numpy as np
import pytest

LD = np.longdouble
U = 2.0 ** -53
SQRT_BAR = 1.5 * (2.0 ** -23) ** 2 + 4 * U
ATAN_BAR = 1e-14
INACTIVE = 0x7FF8DEAD0000BEEF  # what the hook writes for a lane with act = 0
HALF_PI_BITS = 0x3FF921FB54442D18


def _guard():
    assert np.finfo(LD).nmant >= 63, "np.longdouble is no wider than double here"


def _neighbours(v, n):
    out, lo, hi = [v], v, v
    for _ in range(n):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return out


def sqrt_inputs():
    rng = np.random.RandomState(23)
    lo, hi = np.log2(2.3e-308), np.log2(1.7e308)
    x = [2.0 ** rng.uniform(lo, hi, 1 << 18)]
    p4 = []
    for e in range(-511, 512):
        p4 += _neighbours(4.0 ** e, 1)
    p4 = np.array(p4)
    x.append(p4[(p4 >= 2.3e-308) & (p4 <= 1.7e308)])
    return np.concatenate(x)


SQRT_EDGES = np.array([0.0, -0.0, np.inf, np.nan, -1.0, -1e-300, -1e300, -np.inf])
SQRT_SUBNORMAL = np.array([5e-324, 1e-310])

ROW_BOUNDARIES = [2.0 ** e * (1 + j / 4) for e in range(-4, 4) for j in range(4)] + [16.0]


def rounds_up_points():
    """For each row boundary b (a float): a double below b whose float is b,
    so its row is picked as b's."""
    return np.array([b * (1 - 2.0 ** -26) for b in ROW_BOUNDARIES])


def atan_boundary_inputs():
    pts = []
    for b in ROW_BOUNDARIES:
        pts += _neighbours(b, 3)
    pts += list(rounds_up_points())
    pts += [1e200, 5e-324, 1e-310, 2.2250738585072014e-308, 1e300, 1e-300]
    pts = np.array(pts)
    return np.concatenate([pts, -pts])


def atan_sweep_inputs():
    rng = np.random.RandomState(29)
    mag = 10.0 ** rng.uniform(-300, 300, 1 << 18)
    return np.concatenate([mag * rng.choice([-1.0, 1.0], mag.size),
                           rng.uniform(-20, 20, 1 << 17)])


def row_of(x):
    """acl_atan_b's row index (the float bits of |x|)."""
    with np.errstate(over="ignore"):
        bits = np.abs(np.asarray(x, np.float64)).astype(np.float32).view(np.uint32)
    return np.clip((bits >> 21).astype(np.int64) - (123 << 2) + 1, 0, 33)


def _sweep(x, act=None):
    import torch
    from aclswarm_amd import _lib as L
    dev = torch.device("cuda:0")
    x = np.ascontiguousarray(x, np.float64)
    a = np.ones(len(x), np.int32) if act is None else np.ascontiguousarray(act, np.int32)
    xd, ad = torch.from_numpy(x).to(dev), torch.from_numpy(a).to(dev)
    out = torch.zeros(4 * len(x), dtype=torch.float64, device=dev)
    rc = L.lib().acl_internal_fastmath_sweep(ct.c_void_p(xd.data_ptr()),
                                             ct.c_void_p(ad.data_ptr()),
                                             ct.c_void_p(out.data_ptr()), len(x))
    assert rc == 0
    return out.cpu().numpy().reshape(4, len(x))


def _same_bits(a, b):
    """Bit-equal, NaN against NaN counting as equal."""
    both_nan = np.isnan(a) & np.isnan(b)
    return (a.view(np.uint64) == b.view(np.uint64)) | both_nan


def _rel(got, ref):
    return np.abs(got.astype(LD) - ref) / np.abs(ref)


@pytest.mark.gpu
def test_sqrt_nr1_against_longdouble(cuda):
    _guard()
    x = sqrt_inputs()
    out = _sweep(x)
    rel = _rel(out[0], np.sqrt(x.astype(LD)))
    worst = float(rel.max())
    print("sqrt_nr1: largest relative error %.4e at x = %r (bar %.4e, %d points)"
          % (worst, x[int(rel.argmax())], SQRT_BAR, x.size))
    assert worst <= SQRT_BAR
    assert _same_bits(out[0], out[1]).all()


@pytest.mark.gpu
def test_sqrt_nr1_edges_and_split_form(cuda):
    """+-0 and +inf come back as themselves (the sign of zero kept), NaN and
    negative arguments as NaN; the recombined form has the same bits. A
    subnormal argument is outside what the comments promise: nothing
    non-finite or negative may come out. (What does come out on the MI355X:
    the hardware honours fp64 subnormals, sqrt_nr1(5e-324) is
    2.2227587494850775e-162, the exact root, and sqrt_nr1(1e-310) is
    9.999999999999984e-156, two ulps below it.)"""
    x = np.concatenate([SQRT_EDGES, SQRT_SUBNORMAL])
    out = _sweep(x)
    s = out[0]
    assert s[0] == 0 and not np.signbit(s[0])
    assert s[1] == 0 and np.signbit(s[1])
    assert s[2] == np.inf
    assert np.isnan(s[3:8]).all(), s[3:8]
    assert _same_bits(out[0], out[1]).all()
    sub = s[8:]
    print("sqrt_nr1 of the subnormals %r: %r (exact %r)" % (list(SQRT_SUBNORMAL), list(sub),
                                                           list(np.sqrt(SQRT_SUBNORMAL))))
    assert np.isfinite(sub).all() and (sub >= 0).all() and not np.signbit(sub).any()


def _atan_reference_mp(x):
    import mpmath
    mpmath.mp.dps = 40
    return [mpmath.atan(mpmath.mpf(float(v))) for v in x]


@pytest.mark.gpu
def test_atan_b_sweep_against_longdouble(cuda):
    _guard()
    x = atan_sweep_inputs()
    out = _sweep(x)
    rel = _rel(out[2], np.arctan(x.astype(LD)))
    worst = float(rel.max())
    print("acl_atan_b: largest relative error %.4e at x = %r (bar %.1e, %d points)"
          % (worst, x[int(rel.argmax())], ATAN_BAR, x.size))
    assert worst <= ATAN_BAR
    assert (np.signbit(out[2]) == np.signbit(x)).all()
    # the vote form with every lane active
    assert _same_bits(out[2], out[3]).all()


@pytest.mark.gpu
def test_atan_b_row_boundaries_and_edges(cuda):
    import mpmath
    x = atan_boundary_inputs()
    out = _sweep(x)
    ref = _atan_reference_mp(x)
    worst, at = 0.0, None
    for v, got, r in zip(x, out[2], ref):
        e = float(abs(mpmath.mpf(float(got)) - r) / abs(r))
        if e > worst:
            worst, at = e, v
    print("acl_atan_b at the row boundaries: largest relative error %.4e at x = %r "
          "(bar %.1e, %d points)" % (worst, at, ATAN_BAR, x.size))
    assert worst <= ATAN_BAR
    assert _same_bits(out[2], out[3]).all()
    e = np.array([0.0, -0.0, np.inf, -np.inf, np.nan])
    o = _sweep(e)
    for p in (2, 3):
        a = o[p]
        assert a[0] == 0 and not np.signbit(a[0]) and a[1] == 0 and np.signbit(a[1])
        assert a[2:4].view(np.uint64).tolist() == [HALF_PI_BITS, HALF_PI_BITS | (1 << 63)]
        assert np.isnan(a[4])


def vote_case():
    """24 waves of x from the sweep and the boundary points, infinities by
    wave (w % 4: none; one lane; every lane; one lane that the second and
    third patterns leave inactive), and the three activity patterns."""
    W = 24
    rng = np.random.RandomState(31)
    pool = np.concatenate([atan_boundary_inputs(), atan_sweep_inputs()[:4096]])
    x = rng.choice(pool, 64 * W).reshape(W, 64)
    lane = np.arange(64)
    third = np.ones((W, 64), np.int32)
    third[:, lane % 3 == 2] = 0
    single = np.zeros((W, 64), np.int32)
    for w in range(W):
        single[w, (5 * w) % 64] = 1
        sign = -1.0 if w & 4 else 1.0
        if w % 4 == 1:
            x[w, (7 * w) % 64] = sign * np.inf
        elif w % 4 == 2:
            x[w, :] = np.where(lane & 1, -np.inf, np.inf)
        elif w % 4 == 3:
            cand = [q for q in range(64) if q % 3 == 2 and q != (5 * w) % 64]
            x[w, cand[w % len(cand)]] = sign * np.inf
    return x.ravel(), [np.ones(64 * W, np.int32), third.ravel(), single.ravel()]


@pytest.mark.gpu
def test_atan_b_vote_under_partial_exec_masks(cuda):
    x, patterns = vote_case()
    for act in patterns:
        out = _sweep(x, act)
        on = act != 0
        assert _same_bits(out[3][on], out[2][on]).all()
        assert (out[3][~on].view(np.uint64) == np.uint64(INACTIVE)).all()
        inf = np.isinf(x)
        want = np.where(x[inf] > 0, np.uint64(HALF_PI_BITS), np.uint64(HALF_PI_BITS | (1 << 63)))
        assert (out[2][inf].view(np.uint64) == want).all()
        fin = on & np.isfinite(x)
        assert np.isfinite(out[3][fin]).all()


def test_boundary_inputs_land_in_the_rows_they_are_meant_for():
    b = np.array(ROW_BOUNDARIES)
    assert (row_of(b) == np.arange(1, 34)).all()
    below = rounds_up_points()
    assert (below < b).all() and (below.astype(np.float32) == b.astype(np.float32)).all()
    assert (row_of(below) == row_of(b)).all()          # the next row, by its float
    assert (row_of(np.nextafter(b, 0) * (1 - 2.0 ** -20)) == np.arange(0, 33)).all()
    assert row_of(1e200) == 33  # (its float is inf)
    assert row_of(5e-324) == 0 and row_of(0.0) == 0 and row_of(np.nan) == 33


def test_vote_case_places_the_infinities():
    x, (full, third, single) = vote_case()
    x = x.reshape(24, 64)
    third, single = third.reshape(24, 64), single.reshape(24, 64)
    inf = np.isinf(x)
    assert (inf.sum(1)[0::4] == 0).all() and (inf.sum(1)[1::4] == 1).all()
    assert (inf.sum(1)[2::4] == 64).all() and (inf.sum(1)[3::4] == 1).all()
    # in the waves of the fourth kind the infinity sits in an inactive lane only
    assert not (inf[3::4] & (third[3::4] != 0)).any()
    assert not (inf[3::4] & (single[3::4] != 0)).any()
    assert (single.sum(1) == 1).all() and full.all()
    # some waves of the second pattern have an active infinity, others none
    act_inf = (inf & (third != 0)).any(1)
    assert act_inf.any() and not act_inf.all()


def test_bars():
    assert 2.1e-14 < SQRT_BAR < 2.2e-14
