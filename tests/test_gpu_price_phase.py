"""The price phase and the START bids of the fused solve (auction_kernel,
phase 2) against the CPU restatement: whole solves at n = 5, 20, 64, 65, 100
and 128 -- one and two vehicle chunks, kAB / n task classes per vehicle from
1 to 25, and the first size with the separate alignment launch -- B = 3
swarms each.

The phase has two loop bodies, chosen per wave by a bound on the inputs
(every coordinate and alignment entry finite and below 1e100: no price can be
NaN, so the body tests none). The cases reach both bodies, with the decision
margin on and off: finite inputs; a NaN and an inf in
q; a non-finite formation coordinate; a coordinate of 1e150, which fails the
bound while every price is finite (NONFINITE must stay clear); vehicles at one
point (a squared distance of exactly 0: the IEEE expression); a row whose two
best prices are equal bit for bit (START takes the first task).

The tests without the gpu mark assert on the oracle alone that each
construction reaches its edge."""
import copy

import numpy as np
import pytest

import helpers as H
import pyoracle as O

NS = [5, 20, 64, 65, 100, 128]
CASES = ["finite", "q_nan", "q_inf", "p_nonfinite", "huge", "same_point", "tie"]
B = 3

FLAG_NONFINITE, FLAG_CA_ACTIVE, FLAG_FRAGILE = 0x08, 0x20, 0x40


def _graph(rng, n):
    """Complete minus one random neighbour per row (the bench's shape)."""
    a = np.ones((n, n), np.uint8)
    for i in range(n):
        j = (i + 1 + rng.randint(0, n - 1)) % n
        a[i, j] = a[j, i] = 0
    np.fill_diagonal(a, 0)
    return a


_cases = {}


def _inputs(case, n):
    """(points, adjs, gains, fidx, q, vel, P_in) of a case, built once."""
    key = (case, n)
    if key in _cases:
        return _cases[key]
    rng = np.random.RandomState(9100 + 17 * CASES.index(case) + n)
    side = 4.5 * np.sqrt(n)
    adj = _graph(rng, n)
    p = H.random_positions(rng, n, side)
    q = np.stack([H.random_positions(rng, n, side) for _ in range(B)])
    vel = rng.normal(0, 0.2, (B, n, 3))
    P_in = np.stack([H.random_perm(rng, n) if b % 2 else np.arange(n, dtype=np.uint16)
                     for b in range(B)])
    pts, fidx = [p], np.zeros(B, np.int32)
    if case == "q_nan":
        q[1, n // 2, 1] = np.nan  # (swarms 0 and 2 stay finite)
    elif case == "q_inf":
        q[1, n // 3, 0] = np.inf
        q[2, n - 1, 2] = -np.inf
    elif case == "p_nonfinite":
        p2 = p.copy()
        p[n // 3, 0] = np.inf
        p2[n - 1, 2] = np.nan
        pts, fidx = [p, p2], np.array([0, 1, 0], np.int32)
    elif case == "huge":
        # z enters no alignment: the distances to it are 1e150, their squares
        # finite, the prices 0 after the f32 rounding
        p2 = p.copy()
        p2[n // 2, 2] = -1e150
        pts, fidx = [p, p2], np.array([0, 1, 0], np.int32)
        q[0, n // 4, 2] = 1e150
    elif case == "same_point":
        q[0, n - 1] = q[0, 0]                  # two vehicles at one point
        P_in[1] = np.arange(n, dtype=np.uint16)
        q[1] = p.copy()                        # every vehicle on its own point
        # all points and all vehicles at the origin of xy: every mean is 0,
        # the alignments are the identity and every squared distance is 0
        p2 = np.tile(np.array([[0.0, 0.0, 1.0]]), (n, 1))
        q[2] = p2.copy()
        pts, fidx = [p, p2], np.array([0, 0, 1], np.int32)
    elif case == "tie":
        # two formation points at one place: every vehicle's two prices are
        # one computation; the pair is some row's best (asserted below)
        # (moving a point moves the alignments: the pair is checked again)
        done = False
        for b in range(B):
            C = O.prices(q[b], p, adj, P_in[b])[0]
            for v in range(n):
                j1 = int(C[v].argmax())
                if j1 == n - 1 or done:
                    continue
                keep = p[n - 1].copy()
                p[n - 1] = p[j1]
                C2 = O.prices(q[b], p, adj, P_in[b])[0]
                done = (C2.argmax(1) == j1).any()
                if not done:
                    p[n - 1] = keep
    gains = [H.synth_gains(rng, adj) for _ in pts]
    _cases[key] = (pts, [adj] * len(pts), gains, fidx, q, vel, P_in)
    return _cases[key]


_refs = {}


def _reference(case, n):
    """The oracle's outputs of a case, computed once and shared, never modified."""
    key = (case, n)
    if key not in _refs:
        pts, adjs, gains, fidx, q, vel, P_in = _inputs(case, n)
        _refs[key] = [O.solve(q[b], vel[b], pts[fidx[b]], adjs[fidx[b]], gains[fidx[b]], P_in[b])
                      for b in range(B)]
    return _refs[key]


def _prices(case, n, b):
    pts, adjs, gains, fidx, q, vel, P_in = _inputs(case, n)
    return O.prices(q[b], pts[fidx[b]], adjs[fidx[b]], P_in[b])[0]


def _expected(ref, margin, control):
    """The reference as a call without the margin / without the control stage
    reports it (tests/test_gpu_cbaa_columns.py)."""
    out = copy.deepcopy(ref)
    for r in out:
        fl = int(r["status"]["flags"])
        if not margin:
            fl &= ~FLAG_FRAGILE
            r["status"]["margin"] = -1.0
        if not control:
            fl &= ~FLAG_CA_ACTIVE
        r["status"]["flags"] = fl
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("case", CASES)
def test_price_phase_vs_oracle(cuda, case, n):
    from test_gpu_parity import _compare, _gpu_solve
    args = _inputs(case, n)
    ref = _reference(case, n)
    # the commands are compared on finite, separated inputs only (elsewhere
    # they are non-finite or out of range on both sides)
    control = case in ("finite", "tie")
    outs = {}
    for margin in (True, False):
        gpu = _gpu_solve(*args, do_control=control, margin=margin)
        _compare(gpu, _expected(ref, margin, control), check_control=control)
        outs[margin] = gpu
    # the same outcome in both modes, bit for bit, but the margin fields
    for k in ("who", "P_out") + (("u", "u_safe", "ca_flag") if control else ()):
        np.testing.assert_array_equal(outs[True][k].view(np.uint8), outs[False][k].view(np.uint8),
                                      err_msg=k)
    for k in ("eff_rounds", "rounds", "n_invalid"):
        np.testing.assert_array_equal(outs[True]["status"][k], outs[False]["status"][k])
    keep = np.uint32(0xFFFFFFFF ^ FLAG_FRAGILE)
    np.testing.assert_array_equal(outs[True]["status"]["flags"] & keep,
                                  outs[False]["status"]["flags"] & keep)
    if case == "huge":
        assert not (outs[True]["status"]["flags"] & FLAG_NONFINITE).any()
        assert not (outs[False]["status"]["flags"] & FLAG_NONFINITE).any()


@pytest.mark.parametrize("n", NS)
def test_nonfinite_cases_set_the_flag_where_built(n):
    nf = lambda case: [bool(int(r["status"]["flags"]) & FLAG_NONFINITE) for r in _reference(case, n)]
    assert nf("finite") == [False, False, False]
    assert nf("q_nan") == [False, True, False]
    # (an infinite z is an infinite distance, price 0: no alignment reads z)
    assert nf("q_inf") == [False, True, False]
    assert nf("p_nonfinite") == [True, True, True]


@pytest.mark.parametrize("n", NS)
def test_huge_coordinates_keep_every_price_finite(n):
    pts, adjs, gains, fidx, q, vel, P_in = _inputs("huge", n)
    assert np.abs(q[0]).max() >= 1e100 and np.abs(pts[1]).max() >= 1e100
    for b in range(2):
        C = _prices("huge", n, b)
        assert np.isfinite(C).all() and (C == 0).any()
    assert not any(int(r["status"]["flags"]) & FLAG_NONFINITE for r in _reference("huge", n))


@pytest.mark.parametrize("n", NS)
def test_same_point_reaches_distance_zero(n):
    """A squared distance of exactly 0 is the price f32(1 / 1e-8)."""
    top = np.float32(1.0 / 1e-8)
    pts, adjs, gains, fidx, q, vel, P_in = _inputs("same_point", n)
    assert (q[0, n - 1] == q[0, 0]).all()
    assert _prices("same_point", n, 1).max() == top  # below the fast path's cut
    C, Rt = O.prices(q[2], pts[1], adjs[1], P_in[2])
    assert (Rt == np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0])).all()  # so x is 0 exactly
    assert (C == top).all()


@pytest.mark.parametrize("n", NS)
def test_tie_is_a_rows_best_pair(n):
    """Some row's largest price is held by two tasks, bit for bit; the START
    select (the first of the largest) is the lower task."""
    found = False
    for b in range(B):
        C = _prices("tie", n, b)
        assert np.isfinite(C).all()
        for v in range(n):
            j = int(C[v].argmax())
            same = np.flatnonzero(C[v].view(np.uint32) == C[v, j].view(np.uint32))
            if C[v, j] > 0 and same.size >= 2:
                assert j == same[0]
                found = True
    assert found
