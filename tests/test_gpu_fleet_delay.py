"""GPU parity of acl_fleet_delay_auction_batch (the fleet auction with
per-link message latency: a publication log per vehicle, delivery by due
tick) against the plain-Python restatement tests/fleet_delay_oracle.py,
teacher-forced with the call's own alignments as tests/test_gpu_fleet_auction.py
does; against the existing entry on the same GPU at latency 1; and against
acl_solve_batch's one-call consensus for clean auctions.

Bar: everything bit for bit after every call (integer bookkeeping and
float32 compare-and-copy; latency only moves bids between ticks)."""
import numpy as np
import pytest

import fleet_auction_oracle as FO
import fleet_delay_cases as DC
import test_gpu_fleet_auction as G  # its helpers: tensors, device state, the Rt check

pytestmark = pytest.mark.gpu


def _fleet(cases, lat=None, queue_cap=None, max_iter=0, latency=True):
    """The cases as the swarms of one engine.FleetAuction; lat: [B][n][n]
    (default: every case's own matrix); latency=False: the existing entry."""
    from aclswarm_amd import engine
    scs = [c.sc for c in cases]
    kw = {}
    if latency:
        lat = np.stack([c.lat for c in cases]) if lat is None else lat
        kw = dict(latency=G._t(lat, np.uint8),
                  max_latency=max(int(lat.max()), max(c.max_lat for c in cases)))
    return engine.FleetAuction(G._table(scs), G._t(np.arange(len(scs)), np.int32),
                               Pt=G._u16(np.stack([G._rows(sc) for sc in scs])),
                               queue_cap=queue_cap, max_iter=max_iter, **kw)


def _calls(cases, delays=None):
    """The fleet's calls [(ticks, {swarm: window})]. Window k of swarm b goes
    into slot delays[b] + k and runs to quiescence within the budget. If a
    case cuts its first window short (the restart case: wticks[0] ticks, its
    second window in the very next call), the fleet's first call is that
    short, slot 0 is calls 0 + 1 for everybody else (whose window carries on
    in call 1 without a command: a chunk boundary with bids in flight) and
    slot s >= 1 is call s + 1."""
    delays = delays or [0] * len(cases)
    short = [c.wticks[0] for c in cases if c.wticks[0] is not None]
    budget = max(c.budget for c in cases)
    at = {}
    for b, c in enumerate(cases):
        for k in range(len(c.sc.windows)):
            if c.wticks[0] is not None:
                assert delays[b] == 0 and c.wticks[0] == short[0]
                ci = k
            else:
                slot = delays[b] + k
                ci = slot if not short or slot == 0 else slot + 1
            at.setdefault(ci, {})[b] = k
    return [(short[0] if short and ci == 0 else budget, at.get(ci, {}))
            for ci in range(max(at) + 1)], budget


def _commands(cases, issue, fleets):
    B, n = len(cases), cases[0].n
    cmd = np.zeros((B, n), np.uint8)
    q = np.zeros((B, n, 3))
    for b, k in issue.items():
        cmd[b] = cases[b].sc.cmd(k, fleets[b])
        q[b] = cases[b].sc.windows[k][1]
    return cmd, q


def _run_parity(cases, delays=None, queue_cap=None, hist_of=None, max_iter=0):
    """After every call every swarm is compared with its restatement (state,
    outputs, queue_len, status); every full call must end QUIESCENT. Returns
    (fa, fleets, oracle history of swarm hist_of, device history)."""
    scs = [c.sc for c in cases]
    fa = _fleet(cases, queue_cap=queue_cap, max_iter=max_iter)
    fleets = [DC.DO.DelayFleet(c.sc.p, c.sc.adj, c.lat, Pt=c.sc.Pt, queue_cap=queue_cap,
                               max_iter=max_iter) for c in cases]
    calls, budget = _calls(cases, delays)
    oh, gh = [], []
    for ci, (ticks, issue) in enumerate(calls):
        cmd, q = _commands(cases, issue, fleets)
        rows_before = np.stack([fl.Pt.copy() for fl in fleets])
        hist = fa.run(ticks, q=G._t(q, np.float64), cmd=G._t(cmd, np.uint8),
                      history=hist_of is not None)
        got = G._state(fa)
        st = fa.status()
        G._check_rt(fa, scs, cmd, q, rows_before, got["Rt"])
        for b, c in enumerate(cases):
            h = [] if b == hist_of else None
            exp = fleets[b].run(ticks, q=q[b], cmd=cmd[b], Rt=got["Rt"][b], hist=h)
            G._assert_swarm(got, b, fleets[b], st, exp, f"{c.name} (swarm {b}) call {ci}")
            assert ticks < budget or exp["flags"] & FO.QUIESCENT, (c.name, ci, exp)
            if h is not None:
                oh += h
                gh.append({k: v.cpu().numpy()[:, b] for k, v in hist.items()})
    return fa, fleets, oh, gh


def _n13_cases():
    """B = 8 at n = 13, each swarm with its own matrix (1..5; the restart
    case: every link at 5): the stale sequence in three phases, both
    asymmetric-row fleets (the draw under which rows13 stalls, the one under
    which rows13_stall finishes), a clean ring, the restart-while-busy case
    and rows13 under another draw."""
    cases = [DC.draw("stale13"), DC.draw("stale13", 33), DC.rows13_stalls(),
             DC.rows13_stall_finishes(), DC.draw("ring13"), DC.restart_busy(),
             DC.draw("stale13", 34), DC.draw("rows13")]
    return cases, [0, 1, 0, 2, 1, 0, 2, 0]


def test_parity_n13_random_latencies():
    cases, delays = _n13_cases()
    fa, fleets, oh, gh = _run_parity(cases, delays=delays, hist_of=1)
    # what the cases are for (also asserted on the CPU side)
    assert fleets[0].n_thrown.sum() > 0
    assert fleets[2].n_thrown.sum() == 7 and fleets[2].open.all()
    assert (fleets[3].done_tick.min(), fleets[3].done_tick.max()) == (117, 122)
    assert not fleets[3].open.any() and fleets[3].n_thrown.sum() == 0
    assert ((fleets[4].vflags & FO.V_ADOPTED) != 0).all() and fleets[4].n_thrown.sum() == 0
    np.testing.assert_array_equal(fleets[5].n_thrown, cases[5].sc.adj.sum(axis=1))
    assert fleets[5].invalid.all()
    hb = np.concatenate([g["biditer"] for g in gh])
    ho = np.concatenate([g["open"] for g in gh])
    np.testing.assert_array_equal(hb, np.stack([h[0] for h in oh]))
    np.testing.assert_array_equal(ho, np.stack([h[1] for h in oh]))
    assert hb.max() == 2 * 13 - 1 and ho.any() and not ho.all()


class _Flags:
    """What a window's command callable reads of a fleet (flush_flagged)."""

    def __init__(self, invalid):
        self.invalid = invalid


def test_all_ones_latency_equals_the_existing_entry():
    """The same swarms and calls with every link at 1 tick, beside
    engine.FleetAuction without latency on the same GPU: all state arrays,
    outputs, statuses and histories equal after every call."""
    cases, delays = _n13_cases()
    n = 13
    ones = np.ones((len(cases), n, n), np.uint8)
    new, old = _fleet(cases, lat=ones), _fleet(cases, latency=False)
    assert new.max_latency == 5 and old.latency is None  # (a ring longer than it needs)
    calls, _ = _calls(cases, delays)
    for ci, (ticks, issue) in enumerate(calls):
        inv = old.invalid.cpu().numpy()
        cmd, q = _commands(cases, issue, [_Flags(inv[b]) for b in range(len(cases))])
        hs = [fa.run(ticks, q=G._t(q, np.float64), cmd=G._t(cmd, np.uint8), history=True)
              for fa in (new, old)]
        sn, so = G._state(new), G._state(old)
        for k in so:
            np.testing.assert_array_equal(sn[k], so[k], err_msg=f"call {ci}: {k}")
        np.testing.assert_array_equal(new.status(), old.status())
        for k in ("biditer", "open"):
            np.testing.assert_array_equal(hs[0][k].cpu().numpy(), hs[1][k].cpu().numpy())
    st = old.status()
    assert (st["flags"] == FO.QUIESCENT).all() and st["ticks_run"].max() > 0
    assert (so["vflags"] & FO.V_CONSENSUS).any() and so["n_thrown"].sum() > 0


def test_log_ring_wraps_with_max_lat_2():
    """lat in {1, 2}, max_lat = 2: a ring of 4 entries per vehicle, reused
    every other tick through 26 iterations."""
    cases = [DC.wrap(), DC.wrap("rows13", 22), DC.wrap("stale13", 23)]
    fa, fleets, _, _ = _run_parity(cases)
    assert fa.max_latency == 2
    assert (fleets[0].n_tally == 26).all() and not fleets[0].open.any()


def test_largest_ring_uniform_64():
    """Every link at 64 ticks (a ring of 128 entries, two header loads per
    sender) on swarm6: 787 ticks."""
    fa, fleets, _, _ = _run_parity([DC.uniform64()])
    assert fa.status()["ticks_run"][0] == 787 and (fleets[0].vflags == 0x0D).all()


@pytest.mark.parametrize("n", [64, 65, 128])
def test_chord_ring_at_wavefront_boundaries(n):
    """One slot, two slots with the mask-word boundary, and the size limit,
    B = 2 under 1..4 draws. Parity with the restatement runs at a reduced
    max_iter (DC.RING_ITERS: the restatement takes 11 s per swarm for the 2 n
    iterations of n = 128); the full auction of the same swarms on the
    device then ends in acl_solve_batch's tables."""
    cases = [DC.ring_case(n, b) for b in range(2)]
    _run_parity(cases, max_iter=DC.RING_ITERS[n])
    fa = _fleet(cases)  # (the restatement: 577, 576 / 521, 585 / 1026, 1027 ticks)
    q = np.stack([c.sc.windows[0][1] for c in cases])
    fa.run(1500, q=G._t(q, np.float64), cmd=G._t(np.ones((2, n)), np.uint8))
    got, st = G._state(fa), fa.status()
    ident = np.arange(n, dtype=np.uint16)
    for b, c in enumerate(cases):
        who, Rt = G._solve_who(c.sc.p, c.sc.adj, q[b], ident)
        np.testing.assert_array_equal(got["Rt"][b].view(np.uint64), Rt.view(np.uint64))
        np.testing.assert_array_equal(got["final_who"][b], who)
        assert (got["vflags"][b] & FO.V_CONSENSUS).all() and not got["n_thrown"][b].any()
        assert not got["open"][b].any() and (got["n_tally"][b] == 2 * n).all()
        assert st["flags"][b] == FO.QUIESCENT and 2 * n < st["ticks_run"][b] < 1500
        assert got["done_tick"][b].max() <= st["ticks_run"][b] - 1


def test_chunked_calls_equal_one_call():
    """ticks split 1 + 2 + the rest with cmd == NULL equals one call, with
    bids in flight across both boundaries (latencies up to 5); the workspace
    (queues, buckets, publication logs) ends byte for byte the same."""
    import torch
    cases = [DC.uniform("ring13", 5), DC.draw("rows13"), DC.draw("stale13")]
    cmd = G._t(np.stack([c.sc.cmd(0, None) for c in cases]), np.uint8)
    q = G._t(np.stack([c.sc.windows[0][1] for c in cases]), np.float64)
    ticks = DC.BUDGET
    one, parts = _fleet(cases), _fleet(cases)
    h1 = one.run(ticks, q=q, cmd=cmd, history=True)
    s1, st1 = G._state(one), one.status().copy()
    hp = [parts.run(1, q=q, cmd=cmd, history=True)]
    assert not (parts.status()["flags"] & FO.QUIESCENT).any()
    hp.append(parts.run(2, history=True))
    assert not (parts.status()["flags"] & FO.QUIESCENT).any()
    hp.append(parts.run(ticks - 3, history=True))
    sp, stp = G._state(parts), parts.status().copy()
    for k in s1:
        np.testing.assert_array_equal(s1[k], sp[k], err_msg=k)
    np.testing.assert_array_equal(one.ws.cpu().numpy(), parts.ws.cpu().numpy())
    for k in ("biditer", "open"):
        np.testing.assert_array_equal(h1[k].cpu().numpy(),
                                      torch.cat([h[k] for h in hp]).cpu().numpy(), err_msg=k)
    assert (st1["flags"] == FO.QUIESCENT).all() and (stp["flags"] == FO.QUIESCENT).all()
    assert st1["ticks_run"].tolist() == [157, 134, 29]
    assert (stp["ticks_run"] == st1["ticks_run"] - 3).all()
    parts.run(5)
    sq, stq = G._state(parts), parts.status()
    for k in sp:
        np.testing.assert_array_equal(sq[k], sp[k], err_msg=k)
    assert (stq["ticks_run"] == 0).all() and (stq["flags"] == FO.QUIESCENT).all()


def test_bad_latency_leaves_the_swarm_untouched():
    """B = 3: swarm 0 has an entry of 0, swarm 2 one above max_lat; both get
    ACL_FLEET_BAD_INPUT and are untouched. Swarm 1 (whose diagonal holds 0
    and 255: ignored) runs as it does alone."""
    base = DC.draw("ring13")
    n = base.n
    fb = _fleet([base] * 3)
    assert fb.max_latency == 5
    lat = np.stack([base.lat] * 3)
    lat[0, 3, 7] = 0
    lat[2, 5, 1] = 6
    lat[1, np.arange(n), np.arange(n)] = [0, 255] * 6 + [0]
    fb.latency.copy_(G._t(lat, np.uint8))  # (the constructor would refuse the 6)
    before = G._state(fb)
    q = G._t(np.stack([base.sc.windows[0][1]] * 3), np.float64)
    fb.run(base.budget, q=q, cmd=G._t(np.ones((3, n)), np.uint8))
    after, st = G._state(fb), fb.status().copy()
    assert not fb.ws.cpu().numpy()[:fb.ws.numel() // 3].any()  # swarm 0's workspace: untouched
    alone = _fleet([base])
    alone.run(base.budget, q=q[:1], cmd=G._t(np.ones((1, n)), np.uint8))
    ref = G._state(alone)
    for b in (0, 2):
        assert tuple(st[b]) == (0, 0, 0, 0x4)
        for k in before:
            np.testing.assert_array_equal(after[k][b], before[k][b], err_msg=k)
    for k in ref:
        np.testing.assert_array_equal(after[k][1], ref[k][0], err_msg=k)
    assert st[1] == alone.status()[0]
    assert st[1]["flags"] == FO.QUIESCENT and st[1]["ticks_run"] == 119


def test_overflow_with_a_small_queue():
    """queue_cap = 2 on swarm6 under a 1..2 draw: bids are dropped and
    flagged exactly as in the restatement with the same capacity."""
    fa, fleets, _, _ = _run_parity([DC.overflow6()], queue_cap=2)
    st = fa.status()
    assert st["flags"][0] == FO.QUIESCENT | FO.OVERFLOW and st["ticks_run"][0] == 8
    assert ((fleets[0].vflags & FO.V_OVERFLOW) != 0).tolist() == [0, 0, 0, 1, 0, 1]
    assert (fleets[0].queue_len() <= 2).all()
