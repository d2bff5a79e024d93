"""GPU parity of acl_fleet_auction_batch (the message-level CBAA of whole
fleets: queues, buckets and ticks on the device) against the plain-Python
restatement tests/fleet_auction_oracle.py, teacher-forced with the call's own
alignments (whose bits are checked against acl_vehicle_start_batch), and
against acl_solve_batch's one-call consensus for clean auctions.

Bar: everything bit for bit -- the protocol is integer bookkeeping and
float32 compare-and-copy; the prices are the f64 getPrice in the reference's
operation order from an alignment with acl_vehicle_start_batch's bits."""
import ctypes as ct
import functools

import numpy as np
import pytest

import fleet_auction_cases as C
import fleet_auction_oracle as FO
import helpers as H

pytestmark = pytest.mark.gpu

OUT_KEYS = C.STATE_KEYS + ("queue_len",)


def _dev():
    import torch
    return torch.device("cuda:0")


def _t(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dt)).to(_dev())


def _u16(a):
    return _t(np.ascontiguousarray(a, np.uint16).view(np.int16), np.int16)


def _table(scs):
    from aclswarm_amd import engine
    return engine.FormationTable.from_host([sc.p for sc in scs], [sc.adj for sc in scs], None,
                                           device=_dev())


def _rows(sc):
    return np.tile(np.arange(sc.n), (sc.n, 1)) if sc.Pt is None else np.asarray(sc.Pt)


def _fleet(scs, queue_cap=None, fidx=None, max_iter=0):
    from aclswarm_amd import engine
    T = _table(scs)
    fidx = np.arange(len(scs)) if fidx is None else fidx
    return engine.FleetAuction(T, _t(fidx, np.int32), Pt=_u16(np.stack([_rows(sc) for sc in scs])),
                               queue_cap=queue_cap, max_iter=max_iter)


def _state(fa):
    import torch
    torch.cuda.synchronize()
    d = {k: getattr(fa, k).cpu().numpy() for k in OUT_KEYS}
    d["Pt"] = d["Pt"].view(np.uint16).astype(np.int64)
    d["Rt"] = fa.Rt.cpu().numpy()
    return d


def _assert_swarm(got, b, fl, st_got, st_exp, what):
    exp = C.snapshot_state(fl)
    for k in OUT_KEYS:
        g, e = got[k][b], exp[k]
        if k.endswith("price"):
            g, e = g.view(np.uint32), np.ascontiguousarray(e, np.float32).view(np.uint32)
        np.testing.assert_array_equal(g, e, err_msg=f"{what}: {k}")
    assert {k: int(st_got[k][b]) for k in st_exp} == st_exp, what


def _check_rt(fa, scs, cmd, q, rows_before, Rt):
    """The Rt the call wrote for every started vehicle has the bits of
    engine.vehicle_start for the same row and snapshot."""
    import torch
    from aclswarm_amd import engine
    n = scs[0].n
    ks = [(b, v) for b in range(len(scs)) for v in range(n)
          if cmd[b, v] == FO.START and sorted(rows_before[b, v].tolist()) == list(range(n))]
    if not ks:
        return
    bs = np.array([b for b, _ in ks])
    vs = np.array([v for _, v in ks])
    out = engine.vehicle_start(fa.table, _t(fa.fidx.cpu().numpy()[bs], np.int32),
                               _t(vs, np.int32), _t(q, np.float64), _u16(rows_before[bs, vs]),
                               qidx=_t(bs, np.int32), want_bid=False)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(Rt[bs, vs].view(np.uint64),
                                  out["Rt"].cpu().numpy().view(np.uint64))
    assert not out["flags"].cpu().numpy().any()


def _run_parity(scs, delays=None, queue_cap=None, hist_of=None, check_rt=True):
    """The scenarios as the swarms of one fleet, scenario b's window k in call
    delays[b] + k (no command in its other calls); after every call every
    swarm is compared with its restatement. Returns (fa, fleets, oracle
    history of scenario hist_of, device history)."""
    B, n = len(scs), scs[0].n
    delays = delays or [0] * B
    ncalls = max(d + len(sc.windows) for d, sc in zip(delays, scs))
    ticks = max(sc.ticks for sc in scs)
    fa = _fleet(scs, queue_cap=queue_cap)
    fleets = [FO.Fleet(sc.p, sc.adj, Pt=sc.Pt, queue_cap=queue_cap) for sc in scs]
    oh, gh = [], []
    for c in range(ncalls):
        cmd = np.zeros((B, n), np.uint8)
        q = np.zeros((B, n, 3))
        for b, sc in enumerate(scs):
            k = c - delays[b]
            if 0 <= k < len(sc.windows):
                cmd[b] = sc.cmd(k, fleets[b])
                q[b] = sc.windows[k][1]
        rows_before = np.stack([fl.Pt.copy() for fl in fleets])
        hist = fa.run(ticks, q=_t(q, np.float64), cmd=_t(cmd, np.uint8),
                      history=hist_of is not None)
        got = _state(fa)
        st = fa.status()
        if check_rt:
            _check_rt(fa, scs, cmd, q, rows_before, got["Rt"])
        for b, sc in enumerate(scs):
            h = [] if b == hist_of else None
            exp = fleets[b].run(ticks, q=q[b], cmd=cmd[b], Rt=got["Rt"][b], hist=h)
            _assert_swarm(got, b, fleets[b], st, exp, f"{sc.name} (swarm {b}) call {c}")
            assert exp["flags"] & FO.QUIESCENT  # every window runs to its end
            if h is not None:
                oh += h
                gh.append({k: v.cpu().numpy()[:, b] for k, v in hist.items()})
    return fa, fleets, oh, gh


def test_parity_n13_swarms_in_different_phases():
    """B = 8 swarms of one call at n = 13: the four-window stale-START
    sequence in four different phases, the two random-row fleets (one
    finishes, one stalls on thrown bids), a clean ring and a second stale
    sequence; the history of swarm 1 too."""
    scs = [C.stale_start(13)] * 4 + [C.random_rows(13), C.random_rows(13, C.ROWS_STALL_SEED),
                                     C.clean_ring(13), C.stale_start(13, seed=12, silent=7)]
    fa, fleets, oh, gh = _run_parity(scs, delays=[0, 1, 2, 3, 0, 2, 1, 0], hist_of=1)
    # what the scenarios are for (also asserted on the CPU side)
    assert fleets[0].n_thrown.sum() > 0 and not fleets[0].invalid.any()
    assert (fleets[4].done_tick.min(), fleets[4].done_tick.max()) == (74, 77)
    assert fleets[5].n_thrown.sum() > 0 and fleets[5].open.all()
    hb = np.concatenate([g["biditer"] for g in gh])
    ho = np.concatenate([g["open"] for g in gh])
    np.testing.assert_array_equal(hb, np.stack([h[0] for h in oh]))
    np.testing.assert_array_equal(ho, np.stack([h[1] for h in oh]))
    assert hb.max() == 2 * 13 - 1 and ho.any() and not ho.all()


def test_parity_stale_start_n40():
    scs = [C.stale_start(40), C.stale_start(40, seed=12, silent=20)]
    fa, fleets, _, _ = _run_parity(scs, delays=[0, 1])
    assert fleets[0].n_thrown.sum() > 0 and not fleets[0].invalid.any()
    assert ((fleets[0].vflags & FO.V_INVALID) != 0).all()  # window 2


def test_parity_two_rings_and_swarm6():
    """The two-ring case (vehicle 2 silent: only its ring stalls) in B = 8
    swarms with other silent vehicles and seeds; swarm6 from q0 over its
    three formations."""
    scs = [C.rings12(silent=s, seed=5 + s) for s in (2, 2, 0, 7, 11, 5, 6, 3)]
    scs[1] = C.rings12()
    fa, fleets, _, _ = _run_parity(scs)
    st = fa.status()
    assert st["n_open"][1] == 5 and st["flags"][1] == FO.QUIESCENT
    assert fleets[1].open.tolist() == [1, 1, 0, 1, 1, 1] + [0] * 6
    assert ((fleets[1].vflags[6:] & FO.V_CONSENSUS) != 0).all()
    pts, adj, _, q0 = H.swarm6()
    s6 = [C.Scenario(f"swarm6/{f}", pts[f], adj[f], [(np.ones(6, np.uint8), q0)])
          for f in range(3)]
    fa, fleets, _, _ = _run_parity(s6)
    assert fa.status()["ticks_run"][0] == 36 and (fleets[0].vflags == 0x0D).all()


def _solve_who(p, adj, q, P):
    """acl_solve_batch's one-call consensus tables who [n][n] (-1: nobody)."""
    import torch
    from aclswarm_amd import engine
    n = p.shape[0]
    dev = _dev()
    T = engine.FormationTable.from_host([p], [adj], None, device=dev)
    out = engine.solve(T, torch.zeros(1, dtype=torch.int32, device=dev), _t(q[None], np.float64),
                       torch.zeros((1, n, 3), dtype=torch.float64, device=dev),
                       _t(P[None].view(np.int16), np.int16), do_control=False, want_who=True,
                       want_align=True, early_exit=False)
    torch.cuda.synchronize()
    who = out["who"].cpu().numpy().view(np.uint16)[0].astype(np.int32)
    return np.where(who == 0xFFFF, -1, who), out["align_Rt"].cpu().numpy()[0]


def _clean_vs_solve(cases):
    """cases: [(p, adj, q, P)] of one n, the swarms of one fleet call; every
    vehicle's final_who equals its acl_solve_batch table."""
    n = cases[0][0].shape[0]
    scs = []
    for i, (p, adj, q, P) in enumerate(cases):
        Pt = np.empty(n, np.int64)
        Pt[P] = np.arange(n)
        scs.append(C.Scenario(f"clean{n}/{i}", p, adj, [(np.ones(n, np.uint8), q)],
                              Pt=np.tile(Pt, (n, 1))))
    fa = _fleet(scs)
    ticks = max(sc.ticks for sc in scs)
    fa.run(ticks, q=_t(np.stack([c[2] for c in cases]), np.float64),
           cmd=_t(np.ones((len(cases), n)), np.uint8))
    got = _state(fa)
    st = fa.status()
    for b, (p, adj, q, P) in enumerate(cases):
        who, Rt = _solve_who(p, adj, q, P)
        np.testing.assert_array_equal(got["Rt"][b].view(np.uint64), Rt.view(np.uint64))
        np.testing.assert_array_equal(got["final_who"][b], who)
        assert (got["vflags"][b] & FO.V_CONSENSUS).all() and not got["n_thrown"][b].any()
        assert not got["open"][b].any() and (got["n_tally"][b] == 2 * n).all()
        assert st["flags"][b] == FO.QUIESCENT and 0 < st["ticks_run"][b] <= 2 * n * C.d_max(adj)
        assert got["done_tick"][b].max() == st["ticks_run"][b] - 1
    return st


@pytest.mark.parametrize("name", ["simform20_nc", "simform100_nc"])
def test_clean_run_equals_solve_batch_simform(name):
    Pf, Af = H.simform(name)
    n = Pf.shape[2]
    cases = []
    for b in range(2):
        rng = np.random.RandomState(b + 5)
        q = H.random_positions(rng, n, 20.0 if n <= 20 else 45.0)
        cases.append((Pf[b, 0], Af[b].astype(np.uint8), q, H.random_perm(rng, n)))
    _clean_vs_solve(cases)


@pytest.mark.parametrize("n", [64, 65, 128])
def test_clean_run_equals_solve_batch_chord_ring(n):
    """The wavefront boundary and the size limit; 2 n 3 ticks."""
    cases = []
    for b in range(2):
        rng = np.random.RandomState(100 * n + b)
        cases.append((C.points(rng, n), C.chord_ring(n), C.snapshot(rng, n),
                      H.random_perm(rng, n)))
    st = _clean_vs_solve(cases)
    assert (st["ticks_run"] == 2 * n * 3).all()


def test_n129_is_rejected():
    from aclswarm_amd import _lib as L
    from aclswarm_amd import engine
    import torch
    n = 129
    T = engine.FormationTable.from_host([np.zeros((n, 3))], [C.chord_ring(n)], None,
                                        device=_dev())
    with pytest.raises(ValueError):
        engine.FleetAuction(T, torch.zeros(1, dtype=torch.int32, device=_dev()))
    a = L.FleetAuctionArgs()
    a.B, a.ticks, a.queue_cap = 1, 1, 4
    F = T.struct()
    assert L.lib().acl_fleet_auction_batch(ct.byref(F), ct.byref(a), None) == 1  # INVALID_ARG
    assert b"n out of range" in L.lib().acl_last_error()


@functools.lru_cache(maxsize=None)
def _chunk_scs():
    return (C.clean_ring(13), C.random_rows(13), C.stale_start(13))


def test_chunked_calls_equal_one_call():
    """ticks split 1 + 7 + the rest with cmd == NULL equals one call; a call
    after quiescence changes nothing and reports QUIESCENT with ticks_run 0."""
    import torch
    scs = _chunk_scs()
    B, n = len(scs), 13
    cmd = _t(np.stack([sc.cmd(0, None) for sc in scs]), np.uint8)
    q = _t(np.stack([sc.windows[0][1] for sc in scs]), np.float64)
    ticks = max(sc.ticks for sc in scs)
    one, parts = _fleet(scs), _fleet(scs)
    h1 = one.run(ticks, q=q, cmd=cmd, history=True)
    s1, st1 = _state(one), one.status().copy()
    hp = [parts.run(1, q=q, cmd=cmd, history=True), parts.run(7, history=True),
          parts.run(ticks - 8, history=True)]
    sp, stp = _state(parts), parts.status().copy()
    for k in s1:
        np.testing.assert_array_equal(s1[k], sp[k], err_msg=k)
    np.testing.assert_array_equal(one.ws.cpu().numpy(), parts.ws.cpu().numpy())
    for k in ("biditer", "open"):
        np.testing.assert_array_equal(h1[k].cpu().numpy(),
                                      torch.cat([h[k] for h in hp]).cpu().numpy(), err_msg=k)
    assert (st1["flags"] == FO.QUIESCENT).all() and (stp["flags"] == FO.QUIESCENT).all()
    assert (st1["n_open"] == stp["n_open"]).all() and (st1["n_queued"] == stp["n_queued"]).all()
    assert st1["ticks_run"].tolist() == [78, 78, 11]
    assert (stp["ticks_run"] == np.maximum(st1["ticks_run"] - 8, 0)).all()
    parts.run(5)
    sq, stq = _state(parts), parts.status()
    for k in sp:
        np.testing.assert_array_equal(sq[k], sp[k], err_msg=k)
    assert (stq["ticks_run"] == 0).all() and (stq["flags"] == FO.QUIESCENT).all()
    assert (stq["n_open"] == stp["n_open"]).all()


def test_overflow_with_a_small_queue():
    """queue_cap = 2 on swarm6: bids are dropped and flagged exactly as in
    the restatement with the same capacity, and every swarm of the call
    equals its own run alone."""
    pts, adj, _, q0 = H.swarm6()
    scs = [C.Scenario(f"swarm6/{f}", pts[f], adj[f], [(np.ones(6, np.uint8), q0)])
           for f in range(3)]
    fa, fleets, _, _ = _run_parity(scs, queue_cap=2)
    st = fa.status().copy()
    assert st["flags"][0] & FO.OVERFLOW and (fleets[0].vflags & FO.V_OVERFLOW).any()
    assert (fleets[0].queue_len() <= 2).all()
    both = _state(fa)
    for b, sc in enumerate(scs):
        alone = _fleet([sc], queue_cap=2)
        alone.run(sc.ticks, q=_t(q0[None], np.float64), cmd=_t(np.ones((1, 6)), np.uint8))
        sa = _state(alone)
        for k in sa:
            np.testing.assert_array_equal(sa[k][0], both[k][b], err_msg=f"{sc.name}: {k}")
        assert alone.status()[0] == st[b]


def test_bad_row_and_bad_fidx():
    """A non-permutation row with START: V_BAD_ROW, the vehicle stays closed
    and publishes nothing, so its neighbours stall at biditer 0. fidx out of
    range: ACL_FLEET_BAD_INPUT and the swarm's arrays untouched."""
    n = 13
    base = C.clean_ring(n)
    rows = np.tile(np.arange(n), (n, 1))
    rows[4, 9] = 2  # vehicle 4's own row names vehicle 2 twice
    bad = C.Scenario("badrow", base.p, base.adj, base.windows, Pt=rows)
    fa, fleets, _, _ = _run_parity([bad, base])
    fl = fleets[0]
    assert fl.vflags[4] == FO.V_BAD_ROW and not fl.open[4]
    nb = [v for v in range(n) if base.adj[v][4]]
    assert all(fl.open[v] and fl.biditer[v] == 0 for v in nb)
    assert not (fl.vflags & FO.V_CONSENSUS).any()
    assert ((fleets[1].vflags & FO.V_CONSENSUS) != 0).all()
    # fidx out of range on swarm 0 of a fresh fleet; swarm 1 runs as before
    fb = _fleet([base, base], fidx=np.array([7, 1]))
    before = _state(fb)
    q = _t(np.stack([base.windows[0][1]] * 2), np.float64)
    fb.run(base.ticks, q=q, cmd=_t(np.ones((2, n)), np.uint8))
    after, st = _state(fb), fb.status()
    assert tuple(st[0]) == (0, 0, 0, 0x4)
    for k in before:
        np.testing.assert_array_equal(after[k][0], before[k][0], err_msg=k)
    ref = _state(fa)
    for k in ref:
        np.testing.assert_array_equal(after[k][1], ref[k][1], err_msg=k)
    assert st[1]["flags"] == FO.QUIESCENT and st[1]["n_open"] == 0
