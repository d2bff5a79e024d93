"""The fused solve (auction_kernel + pair_gain_fused) after three pieces of
work the result does not need were taken out of it:

* the padded rows of the control phase's point table sit far away instead of
  being masked out of the collision candidate test tile by tile
  (csrc/pair_fused.h, ACL_FUSED_FARPAD);
* the instantiations without the decision margin (skip_margin) track no
  runner-up price and run no second START pass (csrc/auction.hip,
  ACL_START_LEAN);
* first_who reads one lane per vehicle chunk and selects on the scalar unit
  (ACL_FIRST_WHO_RL).

Padding: n = 8, 16 (no padding), 9 (two row blocks, padded, not packed), 17,
20 (three row blocks: packed, with the odd tile out), 21, 23 (padded, not
packed), 65, 100 (the bench's 13 blocks) and 128; four swarms in one call --
generator-style positions, a vehicle exactly at the origin (where the padded
rows used to sit), two vehicles closer than d_avoid_thresh that hold the last
two formation rows (the last column block, and the last row block where it
has two real rows), and a swarm with a NaN and an inf coordinate. The fused
path (5-entry records) is compared with the oracle and with the stand-alone
path (9-plane records of the same gains: gain_kernel / ca_pair_kernel).

The tests without the gpu mark assert on the oracle alone that each
construction reaches its edge."""
import copy

import numpy as np
import pytest

import helpers as H
import pyoracle as O

U_RTOL = 1e-5  # tests/test_gpu_parity.py, tests/test_gpu_fused.py
FLAG_NONFINITE, FLAG_CA_ACTIVE, FLAG_FRAGILE = 0x08, 0x20, 0x40

NS_PAD = [8, 16, 9, 17, 20, 21, 23, 65, 100, 128]
S_GEN, S_ORIGIN, S_CLOSE, S_NONFIN = range(4)

_cache = {}


def _once(key, make):
    """Inputs and references are built once, shared and never modified."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _graph(rng, n):
    """Complete minus one random neighbour per row (the bench's shape)."""
    a = np.ones((n, n), np.uint8)
    for i in range(n):
        j = (i + 1 + rng.randint(0, n - 1)) % n
        a[i, j] = a[j, i] = 0
    np.fill_diagonal(a, 0)
    return a


def _solve(points, adjs, gains, fidx, q, vel, P_in, planes=5, margin=True, control=True):
    import torch
    from aclswarm_amd import engine
    dev = torch.device("cuda:0")
    T = engine.FormationTable.from_host(points, adjs, gains, device=dev, planes=planes)
    out = engine.solve(
        T, torch.from_numpy(np.asarray(fidx, np.int32)).to(dev),
        torch.from_numpy(np.ascontiguousarray(q)).to(dev),
        torch.from_numpy(np.ascontiguousarray(vel)).to(dev),
        torch.from_numpy(np.asarray(P_in, np.uint16).view(np.int16)).to(dev),
        do_control=control, want_who=True, want_gate_margin=control, margin=margin)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["P_out"] = res["P_out"].view(np.uint16)
    res["who"] = res["who"].view(np.uint16)
    res["status"] = np.ascontiguousarray(res["status"]).view(O.STATUS_DTYPE).reshape(-1)
    return res


def _compare_auction(gpu, refs, swarms, margin=True):
    """Tables, assignments, flags, round counts and the margin, bit for bit."""
    for b in swarms:
        r, st = refs[b], gpu["status"][b]
        np.testing.assert_array_equal(gpu["who"][b], r["who"], err_msg=f"who swarm {b}")
        np.testing.assert_array_equal(gpu["P_out"][b], r["P_out"], err_msg=f"P_out swarm {b}")
        fl = int(r["status"]["flags"])
        want = float(r["status"]["margin"])
        if not margin:
            fl, want = fl & ~FLAG_FRAGILE, -1.0
        assert int(st["flags"]) == fl, (b, st, r["status"])
        for k in ("eff_rounds", "rounds", "n_invalid"):
            assert int(st[k]) == int(r["status"][k]), (b, k, st, r["status"])
        assert np.float32(st["margin"]) == np.float32(want), (b, st["margin"], want)


def _compare_control(gpu, refs, swarms):
    """Collision flags and counts exact; commands within U_RTOL of max(|u|, 1)
    where the reference is finite, NaN / inf where it is (the same sign)."""
    for b in swarms:
        r = refs[b]
        assert int(gpu["status"][b]["n_ca"]) == int(r["status"]["n_ca"]), b
        np.testing.assert_array_equal(gpu["ca_flag"][b], r["ca"], err_msg=f"ca swarm {b}")
        for key in ("u", "u_safe"):
            g, x = gpu[key][b], r[key]
            np.testing.assert_array_equal(np.isnan(g), np.isnan(x), err_msg=f"{key} NaN swarm {b}")
            inf = np.isinf(x)
            np.testing.assert_array_equal(np.isinf(g), inf, err_msg=f"{key} inf swarm {b}")
            np.testing.assert_array_equal(g[inf], x[inf], err_msg=f"{key} inf sign swarm {b}")
            fin = np.isfinite(x)
            err = np.abs(g[fin] - x[fin]) / np.maximum(np.abs(x[fin]), 1.0)
            assert err.size == 0 or err.max() <= U_RTOL, (b, key, err.max())


# ---- padding ------------------------------------------------------------------

def _pad_inputs(n):
    def make():
        rng = np.random.RandomState(7700 + n)
        side = 4.5 * np.sqrt(n)
        adj = _graph(rng, n)
        p = np.c_[H.random_positions(rng, n, side)[:, :2], rng.uniform(0.5, 2.5, n)]
        # S_CLOSE's formation: its last two points 0.51 apart. Its vehicles sit
        # next to their own points under the identity, so every vehicle keeps
        # its point (asserted on the oracle below) and the vehicles of rows
        # n - 2 and n - 1 are closer than d_avoid_thresh = 1.5
        p2 = p.copy()
        p2[n - 1] = p2[n - 2] + np.array([0.4, 0.3, 0.1])
        q = np.stack([np.c_[H.random_positions(rng, n, side)[:, :2], rng.uniform(0.5, 2.5, n)]
                      for _ in range(4)])
        P_in = np.stack([H.random_perm(rng, n) if b % 2 else np.arange(n, dtype=np.uint16)
                         for b in range(4)])
        q[S_ORIGIN, n // 2] = 0.0
        q[S_CLOSE] = p2 + rng.normal(0, 1e-3, (n, 3))
        P_in[S_CLOSE] = np.arange(n, dtype=np.uint16)
        q[S_NONFIN, n // 2, 1] = np.nan
        q[S_NONFIN, n // 3, 0] = np.inf
        vel = rng.normal(0, 0.2, (4, n, 3))
        fidx = np.array([0, 0, 1, 0], np.int32)
        gains = [H.synth_gains(rng, adj) for _ in range(2)]
        return [p, p2], [adj, adj], gains, fidx, q, vel, P_in
    return _once(("pad", n), make)


def _pad_ref(n):
    def make():
        pts, adjs, gains, fidx, q, vel, P_in = _pad_inputs(n)
        return [O.solve(q[b], vel[b], pts[fidx[b]], adjs[fidx[b]], gains[fidx[b]], P_in[b])
                for b in range(4)]
    return _once(("pad_ref", n), make)


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS_PAD)
def test_far_padding_vs_oracle_and_standalone(cuda, n):
    args = _pad_inputs(n)
    ref = _pad_ref(n)
    fused = _solve(*args, planes=5)
    _compare_auction(fused, ref, range(4))
    _compare_control(fused, ref, range(4))
    for b in (S_GEN, S_ORIGIN, S_CLOSE):
        gm, rg = float(fused["gate_margin"][b]), ref[b]["gate_margin"]
        assert (gm == rg) if not np.isfinite(rg) else abs(gm - rg) <= 1e-10, (b, gm, rg)
    # the stand-alone path on the same gains as general 9-plane records
    alone = _solve(*args, planes=9)
    for k in ("P_out", "who", "ca_flag", "status"):
        np.testing.assert_array_equal(fused[k], alone[k], err_msg=k)
    for k in ("u", "u_safe"):
        g, x = fused[k], alone[k]
        fin = np.isfinite(x)
        assert np.isfinite(g[fin]).all(), k  # finite wherever the reference path is
        np.testing.assert_array_equal(np.isnan(g), np.isnan(x), err_msg=k)
        np.testing.assert_array_equal(g[np.isinf(x)], x[np.isinf(x)], err_msg=k)
        err = np.abs(g[fin] - x[fin]) / np.maximum(np.abs(x[fin]), 1.0)
        assert err.max() <= U_RTOL, (k, err.max())


@pytest.mark.parametrize("n", NS_PAD)
def test_padding_cases_reach_their_edges(n):
    pts, adjs, gains, fidx, q, vel, P_in = _pad_inputs(n)
    ref = _pad_ref(n)
    thr = O.default_safety().d_avoid_thresh
    assert (q[S_ORIGIN, n // 2] == 0.0).all()
    # generator positions are separated: nobody is close, nothing is flagged
    assert int(ref[S_GEN]["status"]["n_ca"]) == 0 and not ref[S_GEN]["ca"].any()
    # the close pair holds the last two formation rows, and only it is close
    P = ref[S_CLOSE]["P_out"]
    assert (P == np.arange(n)).all()
    d = np.hypot(*(q[S_CLOSE, n - 1, :2] - q[S_CLOSE, n - 2, :2]))
    assert d < thr  # (the first collision test passes for both; whether the
    # avoidance then changes a command depends on where the command points)
    # the non-finite swarm: flagged, and finite commands elsewhere in the batch
    assert int(ref[S_NONFIN]["status"]["flags"]) & FLAG_NONFINITE
    for b in (S_GEN, S_ORIGIN, S_CLOSE):
        assert np.isfinite(ref[b]["u"]).all() and np.isfinite(ref[b]["u_safe"]).all()


# ---- the START bids without the decision margin ----------------------------------

NS_START = [5, 20, 64, 65, 100]
M_TIE0, M_TIE1, M_TIE2, M_LONE, M_NANQ = range(5)


def _start_inputs(n):
    """The `tie` swarms of tests/test_gpu_price_phase.py (two formation points
    at one place: a row's two best prices are one computation, START takes
    the lower task), a swarm in which one vehicle has a single positive price
    (it and one formation point at z = 1e150: every other distance of either
    is 1e150, a price of 0 in f32 -- its START select has no runner-up), and a
    swarm with a NaN in q (the price loop's general body)."""
    def make():
        from test_gpu_price_phase import _inputs
        pts, adjs, gains, fidx, q, vel, P_in = _inputs("tie", n)
        rng = np.random.RandomState(7900 + n)
        p, adj = pts[0], adjs[0]
        w, j = n // 3, n // 2
        p_lone = p.copy()
        p_lone[j, 2] = 1e150
        q_lone = q[0].copy()
        q_lone[w, 2] = 1e150
        q_nan = q[0].copy()
        q_nan[n // 2, 1] = np.nan
        q5 = np.concatenate([q, q_lone[None], q_nan[None]])
        vel5 = np.concatenate([vel, rng.normal(0, 0.2, (2, n, 3))])
        P5 = np.concatenate([P_in, P_in[:1], P_in[:1]])
        f5 = np.array([0, 0, 0, 1, 0], np.int32)
        return [p, p_lone], [adj, adj], [gains[0], gains[0]], f5, q5, vel5, P5
    return _once(("start", n), make)


def _start_ref(n):
    def make():
        pts, adjs, gains, fidx, q, vel, P_in = _start_inputs(n)
        return [O.solve(q[b], vel[b], pts[fidx[b]], adjs[fidx[b]], gains[fidx[b]], P_in[b])
                for b in range(5)]
    return _once(("start_ref", n), make)


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS_START)
def test_margin_off_start_same_bits(cuda, n):
    args = _start_inputs(n)
    ref = _start_ref(n)
    on = _solve(*args, margin=True)
    off = _solve(*args, margin=False)
    _compare_auction(on, ref, range(5), margin=True)
    _compare_auction(off, ref, range(5), margin=False)
    for k in ("P_out", "who", "u", "u_safe", "ca_flag", "gate_margin"):
        np.testing.assert_array_equal(on[k].view(np.uint8), off[k].view(np.uint8), err_msg=k)
    for k in ("eff_rounds", "rounds", "n_invalid", "n_ca"):
        np.testing.assert_array_equal(on["status"][k], off["status"][k], err_msg=k)
    keep = np.uint32(0xFFFFFFFF ^ FLAG_FRAGILE)
    np.testing.assert_array_equal(on["status"]["flags"] & keep, off["status"]["flags"])
    assert (off["status"]["margin"] == -1.0).all()


@pytest.mark.parametrize("n", NS_START)
def test_start_cases_reach_their_edges(n):
    pts, adjs, gains, fidx, q, vel, P_in = _start_inputs(n)
    ref = _start_ref(n)
    # a row whose largest price is held by two tasks, bit for bit
    found = False
    for b in (M_TIE0, M_TIE1, M_TIE2):
        C = O.prices(q[b], pts[0], adjs[0], P_in[b])[0]
        for v in range(n):
            same = np.flatnonzero(C[v].view(np.uint32) == C[v].max().view(np.uint32))
            found |= bool(C[v].max() > 0 and same.size >= 2)
    assert found
    # one vehicle with exactly one positive price: its winner, no runner-up
    C = O.prices(q[M_LONE], pts[1], adjs[1], P_in[M_LONE])[0]
    assert np.isfinite(C).all()
    w, j = n // 3, n // 2
    assert (C[w] > 0).sum() == 1 and C[w, j] > 0
    assert not int(ref[M_LONE]["status"]["flags"]) & FLAG_NONFINITE
    assert int(ref[M_NANQ]["status"]["flags"]) & FLAG_NONFINITE


# ---- first_who: a level held under two `who`s -----------------------------------

# (n, first holder): lane 0, lane 63 (the last of chunk 0; at n = 65 the second
# holder is then vehicle 64, the only lane of chunk 1) and vehicle 64 (the
# first of chunk 1). At n = 65 vehicle 64 is the last vehicle and cannot be the
# first of two holders.
WHO_CASES = [(65, 0), (65, 63), (100, 0), (100, 63), (100, 64)]


def _force_tie_at(q, p, adj, P_in, v, w):
    """tests/test_gpu_cbaa_columns.py's _force_tie for a given pair v < w, not
    adjacent: w is moved (in place) until its START bid goes to v's task at
    v's price, bit for bit in f32. False when the construction fails."""
    from test_gpu_cbaa_columns import _price_rows
    C, Rt = O.prices(q, p, adj, P_in)
    j = int(C[v].argmax())
    target = C[v, j]
    assert target > 0 and not adj[v, w]
    d = 1.0 / float(target) - 1e-8
    r = [x for x in {w, int(P_in[w]), int(np.flatnonzero(P_in == w)[0])}
         if np.array_equal(_price_rows(q[[w]], p, Rt[[x]])[0], C[w])][0]
    for _ in range(3):  # the image of task j moves with w: fixed-point steps
        Rw = O.prices(q, p, adj, P_in)[1][r]
        a = np.array([(Rw[0] * p[j, 0] + Rw[1] * p[j, 1]) + Rw[4],
                      (Rw[2] * p[j, 0] + Rw[3] * p[j, 1]) + Rw[5], p[j, 2]])
        q[w] = a + np.array([d, 0.0, 0.0])
    lo, hi = 0.5 * d, 2.0 * d
    for _ in range(100):
        mid = 0.5 * (lo + hi)
        q[w] = a + np.array([mid, 0.0, 0.0])
        Cw = O.prices(q, p, adj, P_in)[0]
        if Cw[w, j] == target:
            break
        if Cw[w, j] > target:
            lo = mid
        else:
            hi = mid
    return bool(Cw[w, j] == target and int(Cw[w].argmax()) == j and np.array_equal(Cw[v], C[v]))


def _who_inputs(n, v):
    """One swarm whose vehicles v and n - 1 (not adjacent) place their START
    bids on one task at bit-equal prices: that column's top level is held under
    two `who`s in round 1, the first holder in lane v & 63 of chunk v >> 6."""
    def make():
        w = n - 1
        for seed in range(50):
            rng = np.random.RandomState(8100 + 977 * seed + 7 * n + v)
            side = 4.5 * np.sqrt(n)
            adj = _graph(rng, n)
            adj[v, w] = adj[w, v] = 0
            p = H.random_positions(rng, n, side)
            q = H.random_positions(rng, n, side)
            P_in = np.arange(n, dtype=np.uint16) if seed % 2 else H.random_perm(rng, n)
            if _force_tie_at(q, p, adj, P_in, v, w):
                vel = rng.normal(0, 0.2, (1, n, 3))
                return ([p], [adj], [H.synth_gains(rng, adj)], np.zeros(1, np.int32), q[None], vel,
                        P_in[None])
        raise AssertionError("no tie constructed")
    return _once(("who", n, v), make)


def _who_ref(n, v):
    def make():
        pts, adjs, gains, fidx, q, vel, P_in = _who_inputs(n, v)
        return [O.solve(q[0], vel[0], pts[0], adjs[0], gains[0], P_in[0])]
    return _once(("who_ref", n, v), make)


@pytest.mark.gpu
@pytest.mark.parametrize("n,v", WHO_CASES)
def test_first_who_two_holders_vs_oracle(cuda, n, v):
    args = _who_inputs(n, v)
    ref = _who_ref(n, v)
    for margin in (True, False):
        gpu = _solve(*args, margin=margin)
        _compare_auction(gpu, ref, [0], margin=margin)
        _compare_control(gpu, ref, [0])


@pytest.mark.parametrize("n,v", WHO_CASES)
def test_two_holders_sit_where_the_case_wants_them(n, v):
    pts, adjs, gains, fidx, q, vel, P_in = _who_inputs(n, v)
    C = O.prices(q[0], pts[0], adjs[0], P_in[0])[0]
    w = n - 1
    best = C.argmax(1)
    assert best[v] == best[w] and not adjs[0][v, w] and C[v, best[v]] > 0
    assert C[v, best[v]].view(np.uint32) == C[w, best[w]].view(np.uint32)
    # v is the first holder: no lower vehicle bids that task at that price
    top = C[np.arange(n), best]
    first = [x for x in range(n) if best[x] == best[v]
             and top[x].view(np.uint32) == top[v].view(np.uint32)]
    assert first[0] == v and first[-1] == w
