"""CPU suite of the fleet auction (acl_fleet_auction_batch): the plain-Python
restatement of the model (tests/fleet_auction_oracle.py) against
cbaa_step_oracle.lockstep and the message-level effects the model exists for,
the ABI's argument checks, and engine.FleetAuction's rejections -- none of it
needs a GPU. The GPU kernel is compared with the same restatement in
tests/test_gpu_fleet_auction.py."""
import ctypes as ct

import numpy as np
import pytest

import fleet_auction_cases as C
import fleet_auction_oracle as FO


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", ["swarm6", "ring13"])
def test_clean_run_equals_lockstep(name):
    """Every vehicle starts from one table: the final tables are lockstep's,
    nothing is thrown away, every vehicle adopts (just_received), and the
    auction takes at most 2 n d_max ticks."""
    sc, fl, recs = C.cpu_run(name)
    r, n = recs[0], sc.n
    s = r["state"]
    who, price = C.lockstep_tables(sc.p, sc.adj, r["q"], r["Rt"], r["rows"][0])
    np.testing.assert_array_equal(s["final_who"], who)
    np.testing.assert_array_equal(_bits(s["final_price"]), _bits(price))
    assert s["n_thrown"].sum() == 0
    want = FO.V_STARTED | FO.V_CONSENSUS | FO.V_ADOPTED
    assert (s["vflags"] == want).all() and not s["open"].any() and not s["invalid"].any()
    assert (s["Pt"] == who).all() and not s["just_received"].any()
    st = r["status"]
    assert st["flags"] == FO.QUIESCENT and st["n_open"] == 0
    assert 0 < st["ticks_run"] <= 2 * n * C.d_max(sc.adj)
    assert s["done_tick"].max() == st["ticks_run"] - 1
    assert (s["n_tally"] == 2 * n).all()


def test_stale_start_sequence():
    """Chord ring, n = 13. Window 1: vehicle 3 stays silent, its neighbours
    stall at biditer 0 and nobody reaches consensus. Window 2: everybody
    restarts; the new auction is seeded with the stalled one's START bids
    (bids_curr_ = bids_zero_, insert refuses the fresh bid), bids are thrown
    away, and the consensus differs from lockstep of the same price rows or
    is invalid. Window 3: the flagged vehicles flush. Window 4: a clean
    auction again."""
    sc, fl, recs = C.cpu_run("stale13")
    n = sc.n
    w1, w2, w3, w4 = recs
    s1 = w1["state"]
    assert w1["status"]["flags"] == FO.QUIESCENT
    assert not (s1["vflags"] & FO.V_CONSENSUS).any()
    nbrs3 = [v for v in range(n) if sc.adj[v][3]]
    assert nbrs3 and all(s1["open"][v] and s1["biditer"][v] == 0 for v in nbrs3)
    assert s1["open"].sum() == n - 1 and not s1["open"][3]

    s2 = w2["state"]
    who2, _ = C.lockstep_tables(sc.p, sc.adj, w2["q"], w2["Rt"], w2["rows"][0])
    assert ((s2["vflags"] & FO.V_CONSENSUS) != 0).all()
    assert s2["n_thrown"].sum() > 0
    wrong = [bool(s2["invalid"][v]) or (s2["final_who"][v] != who2[v]).any() for v in range(n)]
    assert any(wrong)

    assert (w3["cmd"] == np.where(s2["invalid"] != 0, FO.FLUSH, FO.NONE)).all()
    s3 = w3["state"]
    assert not s3["invalid"].any() and not s3["open"].any()
    assert (s3["queue_len"][w3["cmd"] == FO.FLUSH] == 0).all()

    s4 = w4["state"]
    who4, price4 = C.lockstep_tables(sc.p, sc.adj, w4["q"], w4["Rt"], w4["rows"][0])
    np.testing.assert_array_equal(s4["final_who"], who4)
    np.testing.assert_array_equal(_bits(s4["final_price"]), _bits(price4))
    assert not s4["invalid"].any() and not s4["open"].any()
    assert ((s4["vflags"] & FO.V_ADOPTED) != 0).all()


def test_two_rings_stall_only_the_silent_component():
    """Two disjoint rings of 6 (n = 12, identity rows), vehicle 2 silent: the
    ring 6..11 runs its auction to consensus while 0, 1, 3, 4, 5 stay open.
    The six vehicles of the finished ring hold a table that gives each of
    them its own task and leaves six of the twelve tasks without a bidder, so
    isValidAssignment (auctioneer.cpp:325-343) refuses it: they flag invalid
    rather than adopt (the model's rule for a table that is no permutation)."""
    sc, fl, recs = C.cpu_run("rings12")
    s, st = recs[0]["state"], recs[0]["status"]
    assert ((s["vflags"][6:] & FO.V_CONSENSUS) != 0).all()
    assert not (s["vflags"][:6] & FO.V_CONSENSUS).any()
    assert s["open"].tolist() == [1, 1, 0, 1, 1, 1] + [0] * 6
    assert st["n_open"] == 5 and st["flags"] == FO.QUIESCENT
    for v in range(6, 12):
        held = sorted(int(x) for x in s["final_who"][v] if x >= 0)
        assert held == list(range(6, 12))  # one task each, all agreed
        assert (s["final_who"][v] == s["final_who"][6]).all()
    assert (s["invalid"][6:] == 1).all() and not s["invalid"][:6].any()
    assert s["n_thrown"].sum() == 0


def test_asymmetric_rows_finish_or_stall():
    """Vehicles that each hold their own random row subscribe asymmetrically.
    With the committed seed the auction still completes (78 ticks, consensus
    at ticks 74-77); with another a sender runs two iterations ahead of a
    receiver it does not wait for, its bid is thrown away and the fleet
    stalls."""
    sc, fl, recs = C.cpu_run("rows13")
    s, st = recs[0]["state"], recs[0]["status"]
    fresh = sc.fleet()  # (the rows the auction started from: it ends with one adopted table)
    subs = [fresh.subscribed(v) for v in range(sc.n)]
    assert any((u in subs[w]) != (w in subs[u]) for w in range(sc.n) for u in range(sc.n))
    assert st["ticks_run"] == 78 and ((s["vflags"] & FO.V_CONSENSUS) != 0).all()
    assert (s["done_tick"].min(), s["done_tick"].max()) == (74, 77)
    sc2, fl2, recs2 = C.cpu_run("rows13_stall")
    s2, st2 = recs2[0]["state"], recs2[0]["status"]
    assert s2["n_thrown"].sum() > 0 and st2["n_open"] == sc2.n
    assert st2["flags"] == FO.QUIESCENT and not (s2["vflags"] & FO.V_CONSENSUS).any()


@pytest.mark.parametrize("name", ["swarm6", "ring13", "stale13", "rings12", "rows13",
                                  "rows13_stall"])
def test_queue_stays_below_default_capacity(name):
    """queue_cap = 4 n is never reached in the scenarios the parity tests
    run, so none of them runs into drops unnoticed."""
    sc, fl, recs = C.cpu_run(name)
    assert fl.cap == 4 * sc.n and 0 < fl.max_queue < fl.cap
    assert not any(r["status"]["flags"] & FO.OVERFLOW for r in recs)
    assert not any((r["state"]["vflags"] & FO.V_OVERFLOW).any() for r in recs)


def test_chunked_run_equals_one_run():
    """ticks = a then b equals a + b, and a run after quiescence is a no-op."""
    sc = C.swarm6()
    q = sc.windows[0][1]
    Rt = C.align_rt(sc.p, sc.adj, q, np.tile(np.arange(6), (6, 1)))
    one, parts = sc.fleet(), sc.fleet()
    st = one.run(sc.ticks, q=q, cmd=sc.cmd(0, one), Rt=Rt)
    parts.run(1, q=q, cmd=sc.cmd(0, parts), Rt=Rt)
    parts.run(7)
    parts.run(sc.ticks)
    for k in C.STATE_KEYS:
        np.testing.assert_array_equal(getattr(one, k), getattr(parts, k), err_msg=k)
    again = parts.run(5)
    assert again["ticks_run"] == 0 and again["flags"] == FO.QUIESCENT
    assert st["ticks_run"] == one.tick == parts.tick


def test_overflow_is_flagged_in_the_restatement():
    sc = C.swarm6(queue_cap=2)
    fl, recs = C.run_oracle(sc)
    assert recs[0]["status"]["flags"] & FO.OVERFLOW
    assert (recs[0]["state"]["vflags"] & FO.V_OVERFLOW).any() and fl.max_queue == 2


# ---- the ABI and engine.FleetAuction without a GPU ----

def test_abi_argument_errors_without_gpu():
    from aclswarm_amd import _lib as L
    lib = L.lib()
    assert ct.sizeof(L.FleetAuctionArgs) == 16 + 22 * 8 + 8
    assert L.FLEET_STATUS_DTYPE.itemsize == 16
    F = L.Formations(129, 1, 8, 8, None, None)
    a = L.FleetAuctionArgs()
    a.B, a.ticks, a.queue_cap = 1, 1, 4
    assert lib.acl_fleet_auction_batch(ct.byref(F), ct.byref(a), None) == 1  # INVALID_ARG
    assert b"n out of range [1, 128]" in lib.acl_last_error()
    F.n = 13
    assert lib.acl_fleet_auction_batch(ct.byref(F), ct.byref(a), None) == 1
    assert b"NULL" in lib.acl_last_error()
    a.queue_cap = 0
    assert lib.acl_fleet_auction_batch(ct.byref(F), ct.byref(a), None) == 1
    assert b"queue_cap" in lib.acl_last_error()
    a.queue_cap = 4
    for k, _ in L.FleetAuctionArgs._fields_[4:-1]:
        setattr(a, k, 8)  # never dereferenced: the calls below fail their checks
    a.hist_biditer = a.hist_open = None
    a.workspace_bytes = lib.acl_fleet_workspace_bytes(13, 1, 4) - 1
    assert lib.acl_fleet_auction_batch(ct.byref(F), ct.byref(a), None) == 1
    assert b"workspace_bytes" in lib.acl_last_error()
    a.workspace_bytes += 1
    a.ticks = 0
    assert lib.acl_fleet_auction_batch(ct.byref(F), ct.byref(a), None) == 1
    assert b"at least one tick" in lib.acl_last_error()
    a.B = 0
    assert lib.acl_fleet_auction_batch(ct.byref(F), ct.byref(a), None) == 0  # empty batch
    assert lib.acl_fleet_auction_batch(None, ct.byref(a), None) == 1


def test_workspace_bytes():
    """Per swarm: 16 + n (80 + 24) + 8 n^2 + 24 n^3 + n cap (8 + 8 n) bytes (the
    tick counter, per-vehicle bookkeeping and start position, one stale
    table, three buckets of n tables, cap queue entries); the sizes DESIGN
    quotes."""
    from aclswarm_amd import _lib as L
    lib = L.lib()

    def per_swarm(n, cap):
        return 16 + n * 104 + 8 * n * n + 24 * n ** 3 + n * cap * (8 + 8 * n)
    for n, B, cap in ((20, 1, 80), (100, 1, 400), (13, 8, 52), (128, 3, 512), (1, 1, 1)):
        assert lib.acl_fleet_workspace_bytes(n, B, cap) == B * per_swarm(n, cap)
    assert per_swarm(20, 80) == 466096 and per_swarm(100, 400) == 56410416
    assert lib.acl_fleet_workspace_bytes(129, 1, 4) == 0
    assert lib.acl_fleet_workspace_bytes(13, 1, 0) == 0


def _cpu_table(n):
    from aclswarm_amd import engine
    return engine.FormationTable.from_host([np.zeros((n, 3))], [C.chord_ring(n)], None,
                                           device="cpu")


def test_fleet_auction_rejections_without_gpu():
    """engine.FleetAuction raises ValueError before anything runs, one case
    per rule."""
    import torch
    from aclswarm_amd import engine
    n, B = 13, 2
    T = _cpu_table(n)
    fidx = torch.zeros(B, dtype=torch.int32)
    Pt = torch.arange(n, dtype=torch.int16).repeat(B, n, 1)
    bad = [
        dict(fidx=fidx.to(torch.int64)),                              # wrong dtype
        dict(fidx=fidx, Pt=Pt.to(torch.int32)),                       # wrong dtype
        dict(fidx=fidx, Pt=Pt[:, :, :-1].contiguous()),               # wrong shape
        dict(fidx=fidx.reshape(B, 1)),                                # wrong shape
        dict(fidx=torch.zeros(2 * B, dtype=torch.int32)[::2]),        # non-contiguous
        dict(fidx=fidx, Pt=Pt.transpose(1, 2)),                       # non-contiguous
        dict(fidx=torch.zeros(B, dtype=torch.int32, device="meta")),  # mixed devices
        dict(fidx=fidx, queue_cap=0),                                 # queue_cap < 1
        dict(fidx=fidx, max_iter=-1),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            engine.FleetAuction(T, **kw)
    with pytest.raises(ValueError, match="out of range"):             # n > 128
        engine.FleetAuction(_cpu_table(129), fidx)
    fa = engine.FleetAuction(T, fidx)
    assert fa.queue_cap == 4 * n and fa.ws is None
    assert (fa.Pt[1, 5] == torch.arange(n, dtype=torch.int16)).all()
    q = torch.zeros((B, n, 3), dtype=torch.float64)
    cmd = torch.ones((B, n), dtype=torch.uint8)
    bad_run = [
        dict(ticks=-1),
        dict(ticks=4, q=q.to(torch.float32), cmd=cmd),                # wrong dtype
        dict(ticks=4, q=q, cmd=cmd.to(torch.int32)),
        dict(ticks=4, q=q[:, :, :2].contiguous(), cmd=cmd),           # wrong shape
        dict(ticks=4, q=q, cmd=cmd[:1]),
        dict(ticks=4, q=q.transpose(0, 1).contiguous().transpose(0, 1), cmd=cmd),  # strides
        dict(ticks=4, q=q.to("meta"), cmd=cmd),                       # mixed devices
        dict(ticks=4, cmd=cmd),                                       # cmd without q
        dict(ticks=0, q=q, cmd=cmd),                                  # cmd needs a tick
        dict(ticks=4, q=q, cmd=cmd),                                  # not on a GPU
    ]
    for kw in bad_run:
        with pytest.raises(ValueError):
            fa.run(**kw)
    assert fa.ws is None  # nothing was allocated or launched
