"""CPU suite of the fleet auction with per-link message latency
(acl_fleet_delay_auction_batch): the plain-Python restatement of the model
(tests/fleet_delay_oracle.py) against today's restatement at latency 1 and
against cbaa_step_oracle.lockstep under random latencies, the effects latency
has on fleets with asymmetric subscriptions, chunked runs and a restart with
bids in flight; the ABI's argument checks and engine.FleetAuction's
rejections. None of it needs a GPU; the kernel is compared with the same
restatement in tests/test_gpu_fleet_delay.py."""
import ctypes as ct
import os
import subprocess

import numpy as np
import pytest

import fleet_auction_cases as C
import fleet_auction_oracle as FO
import fleet_delay_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", DC.NAMES)
def test_all_ones_latency_is_todays_model(name):
    """Every link at 1 tick: every state array, queue_len and every status
    dict (ticks_run included) of every window equal fleet_auction_oracle's."""
    sc, fl0, recs0 = C.cpu_run(name)
    case, fl, recs = DC.cpu_run("ones", name)
    assert len(recs) == len(recs0)
    for k, (r, r0) in enumerate(zip(recs, recs0)):
        assert r["status"] == r0["status"], (name, k)
        for key in C.STATE_KEYS + ("queue_len",):
            np.testing.assert_array_equal(r["state"][key], r0["state"][key],
                                          err_msg=f"{name} window {k}: {key}")
    assert fl.max_queue == fl0.max_queue and fl.tick == fl0.tick


# ticks_run of the clean auctions under lat_draw(n, seed) in 1..5, seeds
# DC.CLEAN_SEEDS (36 and 78 at latency 1)
CLEAN_TICKS = {"swarm6": (61, 52, 56), "ring13": (131, 131, 120)}


@pytest.mark.parametrize("name", ["swarm6", "ring13"])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_clean_auction_under_latency_equals_lockstep(name, k):
    """Every vehicle starts in one call from one row: latency moves the
    duration only. The final tables are lockstep's bit for bit, nothing is
    thrown away and everybody adopts.

    The duration: no vehicle publishes at its consensus, so the swarm is
    quiescent once the last vehicle is done AND the last bid anybody published
    (the iter 2n-1 bids, which senders that finished early leave behind) has
    passed its sender's slowest link: ticks_run - 1 is the later of
    done_tick.max() and max over senders of (last publication tick + reach).
    At latency 1 the second never exceeds the first; here it may."""
    case, fl, recs = DC.cpu_run("draw", name, DC.CLEAN_SEEDS[k])
    sc, r, n = case.sc, recs[0], case.n
    s, st = r["state"], r["status"]
    who, price = C.lockstep_tables(sc.p, sc.adj, r["q"], r["Rt"], r["rows"][0])
    np.testing.assert_array_equal(s["final_who"], who)
    np.testing.assert_array_equal(_bits(s["final_price"]), _bits(price))
    assert s["n_thrown"].sum() == 0
    want = FO.V_STARTED | FO.V_CONSENSUS | FO.V_ADOPTED
    assert (s["vflags"] == want).all() and not s["open"].any() and not s["invalid"].any()
    assert (s["n_tally"] == 2 * n).all()
    assert st["flags"] == FO.QUIESCENT and st["n_open"] == 0
    drained = int((fl.last_pub + fl.reach).max())
    assert st["ticks_run"] - 1 == max(int(s["done_tick"].max()), drained)
    assert st["ticks_run"] == CLEAN_TICKS[name][k]
    assert st["ticks_run"] > C.cpu_run(name)[2][0]["status"]["ticks_run"]
    assert fl.max_queue <= 3


def test_uniform_latency_3_on_ring13():
    """A uniform 3 ticks: 105 ticks instead of 78, and here the last
    consensus is the last tick (every bid of iteration 2n-1 is consumed)."""
    case, fl, recs = DC.cpu_run("uniform", "ring13", 3)
    st, s = recs[0]["status"], recs[0]["state"]
    assert st["ticks_run"] == 105 and st["n_queued"] == 0
    assert s["done_tick"].max() == 104 and s["n_thrown"].sum() == 0


# ticks_run of every window under lat_draw(n, DC.DRAW_SEED[name]) in 1..5
DRAW_TICKS = {"swarm6": [57], "ring13": [119], "stale13": [29, 121, 0, 121], "rings12": [99],
              "rows13": [134], "rows13_stall": [113]}


@pytest.mark.parametrize("name", DC.NAMES)
def test_random_draws_run_to_quiescence(name):
    """The draws the GPU parity tests run: every window ends QUIESCENT inside
    the budget (run_oracle asserts it) after the committed number of ticks."""
    case, fl, recs = DC.cpu_run("draw", name)
    assert [r["status"]["ticks_run"] for r in recs] == DRAW_TICKS[name]
    assert all(t < case.budget for t in DRAW_TICKS[name])
    assert case.lat.min() == 1 and case.lat.max() == 5 and case.max_lat == 5


def test_asymmetric_rows_flip_under_latency():
    """Whether a sender runs two iterations ahead of a receiver it does not
    wait for depends on the link delays. rows13 finishes at latency 1 (78
    ticks); under the committed draw 7 bids are thrown away and all 13
    vehicles stay open. rows13_stall stalls at latency 1; under its draw it
    finishes in 123 ticks with nothing thrown away."""
    assert C.cpu_run("rows13")[2][0]["status"]["n_open"] == 0
    case, fl, recs = DC.cpu_run("rows13_stalls")
    s, st = recs[0]["state"], recs[0]["status"]
    assert s["n_thrown"].sum() == 7 and st["n_open"] == 13 and st["ticks_run"] == 68
    assert st["flags"] == FO.QUIESCENT and not (s["vflags"] & FO.V_CONSENSUS).any()
    assert C.cpu_run("rows13_stall")[2][0]["status"]["n_open"] == 13
    case, fl, recs = DC.cpu_run("rows13_stall_finishes")
    s, st = recs[0]["state"], recs[0]["status"]
    assert s["n_thrown"].sum() == 0 and st["n_open"] == 0 and st["ticks_run"] == 123
    assert (s["done_tick"].min(), s["done_tick"].max()) == (117, 122)
    assert ((s["vflags"] & FO.V_CONSENSUS) != 0).all()


def test_log_ring_wrap_case_and_largest_ring():
    """max_lat = 2 (a log ring of 4 entries) on ring13 under a 1..2 draw, and
    a uniform 64 on swarm6: both clean auctions, 78 and 787 ticks."""
    case, fl, recs = DC.cpu_run("wrap")
    assert case.max_lat == 2 and set(np.unique(case.lat)) == {1, 2}
    assert recs[0]["status"]["ticks_run"] == 78 and fl.n_thrown.sum() == 0
    assert (fl.n_tally == 26).all()  # 26 publications per vehicle through 4 slots
    case, fl, recs = DC.cpu_run("uniform64")
    assert recs[0]["status"]["ticks_run"] == 787 and fl.done_tick.max() == 786
    assert ((fl.vflags & FO.V_ADOPTED) != 0).all()


def _same(a, b):
    for k in C.STATE_KEYS:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)
    np.testing.assert_array_equal(a.queue_len(), b.queue_len())
    assert a.tick == b.tick


def test_chunked_run_equals_one_run_with_bids_in_flight():
    """Every link at 5 ticks: after 1 tick and after 1 + 2 ticks the START
    bids (publication tick -1, due at tick 4) are still in flight; 1 + 2 +
    the rest equals one run."""
    case = DC.uniform("ring13", 5)
    sc = case.sc
    q = sc.windows[0][1]
    Rt = C.align_rt(sc.p, sc.adj, q, np.tile(np.arange(sc.n), (sc.n, 1)))
    one, parts = case.fleet(), case.fleet()
    st = one.run(case.budget, q=q, cmd=sc.cmd(0, one), Rt=Rt)
    a = parts.run(1, q=q, cmd=sc.cmd(0, parts), Rt=Rt)
    assert a["ticks_run"] == 1 and not a["flags"] & FO.QUIESCENT and all(parts.log)
    b = parts.run(2)
    assert b["ticks_run"] == 2 and not b["flags"] & FO.QUIESCENT and all(parts.log)
    assert not parts.queue_len().any()  # nothing has arrived yet
    c = parts.run(case.budget)
    _same(one, parts)
    assert st["flags"] == c["flags"] == FO.QUIESCENT
    assert st["ticks_run"] == 3 + c["ticks_run"]
    again = parts.run(5)
    assert again["ticks_run"] == 0 and again["flags"] == FO.QUIESCENT


def test_restart_while_first_bids_are_in_flight():
    """Every link at 5 ticks. Window 1 starts everybody and runs 3 ticks: the
    START bids (publication tick -1) are due at tick 4. Window 2 (first tick
    3) starts everybody again from another snapshot: those START bids have
    publication tick 2 and are due at tick 7. So every vehicle receives its
    neighbours' STALE START bids first, after its restart, and files them
    under iter 0 of the new auction: its first tally runs on them (ticks 4 to
    6, one neighbour's bid popped per tick, so a vehicle of degree 2 tallies
    at tick 5 and one of degree 3 at tick 6), and when the fresh START bids
    arrive at tick 7 every vehicle is at biditer 1 and throws them away:
    n_thrown is the vehicle's degree. The auction then runs on, seeded with
    prices of the wrong snapshot, and ends in tables that are not lockstep's
    of window 2 (here: every vehicle flags an invalid assignment)."""
    case = DC.restart_busy()
    sc, n = case.sc, case.n
    fl = case.fleet()
    fl.trace = []
    rows = np.tile(np.arange(n), (n, 1))
    q1, q2 = sc.windows[0][1], sc.windows[1][1]
    Rt1, Rt2 = C.align_rt(sc.p, sc.adj, q1, rows), C.align_rt(sc.p, sc.adj, q2, rows)
    a = fl.run(3, q=q1, cmd=sc.cmd(0, fl), Rt=Rt1)
    assert a == dict(ticks_run=3, n_open=n, n_queued=0, flags=0)
    assert all(len(x) == 1 and x[0][0] == -1 for x in fl.log) and not fl.trace
    stale = [x[0][2].copy() for x in fl.log]
    hist = []
    b = fl.run(case.budget, q=q2, cmd=sc.cmd(1, fl), Rt=Rt2, hist=hist)
    deg = sc.adj.sum(axis=1)
    first = [e for e in fl.trace if e[3] == -1]
    fresh = [e for e in fl.trace if e[3] == 2]
    assert len(first) == len(fresh) == deg.sum()
    assert {e[0] for e in first} == {4} and {e[0] for e in fresh} == {7}  # after the restart
    assert all(e[4] == 0 for e in first + fresh)
    # the first tally of the new auction ran before the fresh START bids arrived
    bi_at = {t: hist[t - 3][0] for t in (4, 5, 6)}
    assert (bi_at[4] == 0).all() and (bi_at[6] == 1).all()
    assert ((bi_at[5] == 1) == (deg == 2)).all()
    np.testing.assert_array_equal(fl.n_thrown, deg)
    assert fl.n_thrown.sum() > 0
    assert b["flags"] == FO.QUIESCENT and b["n_open"] == 0 and b["ticks_run"] == 154
    assert ((fl.vflags & FO.V_CONSENSUS) != 0).all()
    who2, _ = C.lockstep_tables(sc.p, sc.adj, q2, Rt2, rows[0])
    assert fl.invalid.all() and (fl.final_who != who2).any()
    assert any((stale[v] != 0).any() for v in range(n))


ALL_CASES = ([("ones", n) for n in DC.NAMES] + [("draw", n) for n in DC.NAMES] +
             [("draw", n, s) for n in ("swarm6", "ring13") for s in DC.CLEAN_SEEDS] +
             [("rows13_stalls",), ("rows13_stall_finishes",), ("wrap",), ("uniform64",),
              ("uniform", "ring13", 3), ("uniform", "ring13", 5), ("restart_busy",)] +
             [("ring_case", n, s) for n in (64, 65, 128) for s in (0, 1)])


@pytest.mark.parametrize("key", ALL_CASES, ids=lambda k: "-".join(str(x) for x in k))
def test_queue_stays_below_default_capacity(key):
    """queue_cap = 4 n is never reached in a committed case, so no parity
    case hides drops."""
    case, fl, recs = DC.cpu_run(*key)
    assert fl.cap == 4 * case.n and 0 < fl.max_queue < fl.cap
    assert not any(r["status"]["flags"] & FO.OVERFLOW for r in recs)
    assert not any((r["state"]["vflags"] & FO.V_OVERFLOW).any() for r in recs)


def test_overflow_is_flagged_in_the_restatement():
    case, fl, recs = DC.cpu_run("overflow6")
    st, s = recs[0]["status"], recs[0]["state"]
    assert st["flags"] == FO.QUIESCENT | FO.OVERFLOW and st["ticks_run"] == 8
    assert ((s["vflags"] & FO.V_OVERFLOW) != 0).tolist() == [0, 0, 0, 1, 0, 1]
    assert fl.max_queue == 2


# ---- the ABI and engine.FleetAuction without a GPU ----

_SIZE_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "aclswarm_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %d\n", sizeof(acl_fleet_delay_args_t),
         offsetof(acl_fleet_delay_args_t, base), offsetof(acl_fleet_delay_args_t, lat),
         offsetof(acl_fleet_delay_args_t, max_lat), ACL_ABI_VERSION);
  return 0;
}
"""


def test_struct_layout_matches_ctypes(tmp_path):
    from aclswarm_amd import _lib as L
    src = tmp_path / "size.c"
    src.write_text(_SIZE_C)
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe)])
    size, o_base, o_lat, o_max, abi = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert size == ct.sizeof(L.FleetDelayArgs) == ct.sizeof(L.FleetAuctionArgs) + 16
    assert (o_base, o_lat, o_max) == (L.FleetDelayArgs.base.offset, L.FleetDelayArgs.lat.offset,
                                      L.FleetDelayArgs.max_lat.offset)
    assert abi == L.ABI_VERSION == 11  # added symbols: the ABI version stays
    assert L.FLEET_MAX_LAT == 64


def test_workspace_bytes():
    """Per swarm: the existing layout without its stale table, plus per
    vehicle 16 bytes of log bookkeeping and 2 max_lat entries of 8 + 8 n."""
    from aclswarm_amd import _lib as L
    lib = L.lib()
    ws = lib.acl_fleet_delay_workspace_bytes
    assert ws(129, 1, 4, 1) == 0 and ws(13, 0, 4, 1) == 0 and ws(13, 1, 0, 1) == 0
    assert ws(13, 1, 4, 0) == 0 and ws(13, 1, 4, 65) == 0

    def per_swarm(n, cap, ml):
        return (16 + n * 104 + 24 * n ** 3 + n * cap * (8 + 8 * n)
                + n * (16 + 2 * ml * (8 + 8 * n)))
    for n, B, cap in ((20, 1, 80), (100, 1, 400), (13, 8, 52), (128, 3, 512), (1, 1, 1)):
        last = lib.acl_fleet_workspace_bytes(n, B, cap)
        assert last > 0
        for ml in (1, 2, 5, 64):
            cur = ws(n, B, cap, ml)
            assert cur == B * per_swarm(n, cap, ml)
            assert cur > last  # larger than the existing layout, and grows with max_lat
            last = cur


def test_abi_argument_errors_without_gpu():
    from aclswarm_amd import _lib as L
    lib = L.lib()
    call = lib.acl_fleet_delay_auction_batch
    name = b"acl_fleet_delay_auction_batch: "

    def fails(F, d, msg):
        assert call(ct.byref(F), ct.byref(d), None) == 1  # INVALID_ARG
        err = lib.acl_last_error()
        assert err.startswith(name) and msg in err, err

    F = L.Formations(129, 1, 8, 8, None, None)
    d = L.FleetDelayArgs()
    a = d.base
    a.B, a.ticks, a.queue_cap = 1, 1, 4
    d.max_lat = 3
    fails(F, d, b"n out of range [1, 128]")
    F.n = 13
    fails(F, d, b"required pointer is NULL")
    a.queue_cap = 0
    fails(F, d, b"queue_cap < 1")
    a.queue_cap = 4
    a.ticks = -1
    fails(F, d, b"ticks < 0")
    a.ticks = 1
    for k, _ in L.FleetAuctionArgs._fields_[4:-1]:
        setattr(a, k, 8)  # never dereferenced: the calls below fail their checks
    a.hist_biditer = a.hist_open = None
    a.workspace_bytes = lib.acl_fleet_delay_workspace_bytes(13, 1, 4, 3)
    fails(F, d, b"lat is NULL")
    d.lat = 8
    for bad in (0, -1, 65):
        d.max_lat = bad
        fails(F, d, b"max_lat out of range [1, 64]")
    d.max_lat = 3
    a.workspace_bytes -= 1
    fails(F, d, b"workspace_bytes is too small (acl_fleet_delay_workspace_bytes)")
    # a workspace of the existing layout is too small for any max_lat
    a.workspace_bytes = lib.acl_fleet_workspace_bytes(13, 1, 4)
    d.max_lat = 1
    fails(F, d, b"workspace_bytes is too small")
    d.max_lat = 3
    a.workspace_bytes = lib.acl_fleet_delay_workspace_bytes(13, 1, 4, 3)
    a.q = None
    fails(F, d, b"cmd is given and q is NULL")
    a.q = 8
    a.ticks = 0
    fails(F, d, b"at least one tick")
    F.n_formations = 0
    fails(F, d, b"formation table is empty")
    F.n_formations = 1
    a.B = 0
    assert call(ct.byref(F), ct.byref(d), None) == 0  # empty batch
    assert call(None, ct.byref(d), None) == 1 and call(ct.byref(F), None, None) == 1
    assert lib.acl_last_error() == name + b"null argument"


def _cpu_table(n):
    from aclswarm_amd import engine
    return engine.FormationTable.from_host([np.zeros((n, 3))], [C.chord_ring(n)], None,
                                           device="cpu")


def test_fleet_auction_latency_rejections_without_gpu():
    """engine.FleetAuction(latency=, max_latency=) raises ValueError before
    anything runs, one case per rule; a good latency picks the delay entry's
    workspace."""
    import torch
    from aclswarm_amd import _lib as L
    from aclswarm_amd import engine
    n, B = 13, 2
    T = _cpu_table(n)
    fidx = torch.zeros(B, dtype=torch.int32)
    lat = torch.full((B, n, n), 3, dtype=torch.uint8)
    bad = [
        dict(latency=0), dict(latency=65), dict(latency=-1),           # an int outside 1..64
        dict(latency=2.0), dict(latency=True),                         # no int, no tensor
        dict(latency=lat.to(torch.int32)),                             # wrong dtype
        dict(latency=lat[:, :, :-1].contiguous()),                     # wrong shape
        dict(latency=lat[0]),
        dict(latency=lat.transpose(1, 2)),                             # non-contiguous
        dict(latency=torch.full((B, n, n), 3, dtype=torch.uint8, device="meta")),  # device
        dict(latency=lat, max_latency=2),                              # below the largest entry
        dict(latency=lat, max_latency=65),                             # above 64
        dict(latency=3, max_latency=2),
        dict(latency=3, max_latency=4.5),
        dict(max_latency=4),                                           # without latency
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            engine.FleetAuction(T, fidx, **kw)
    lib = L.lib()
    plain = engine.FleetAuction(T, fidx)
    assert plain.latency is None and plain.max_latency is None
    assert plain.workspace_bytes() == lib.acl_fleet_workspace_bytes(n, B, 4 * n)
    fa = engine.FleetAuction(T, fidx, latency=3)
    assert fa.max_latency == 3 and fa.latency.dtype == torch.uint8
    assert tuple(fa.latency.shape) == (B, n, n) and (fa.latency == 3).all()
    assert fa.workspace_bytes() == lib.acl_fleet_delay_workspace_bytes(n, B, 4 * n, 3)
    lat[1, 2, 5] = 7
    fb = engine.FleetAuction(T, fidx, latency=lat)
    assert fb.max_latency == 7 and fb.latency is not lat
    assert engine.FleetAuction(T, fidx, latency=lat, max_latency=64).max_latency == 64
    q = torch.zeros((B, n, 3), dtype=torch.float64)
    cmd = torch.ones((B, n), dtype=torch.uint8)
    for kw in (dict(ticks=4, q=q, cmd=cmd), dict(ticks=0, q=q, cmd=cmd), dict(ticks=-1)):
        with pytest.raises(ValueError):  # (the last: not on a GPU)
            fa.run(**kw)
    assert fa.ws is None  # nothing was allocated or launched
