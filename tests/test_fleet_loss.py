"""CPU suite of the fleet auction with seeded per-link message loss
(acl_fleet_lossy_auction_batch): the plain-Python restatement of the model
(tests/fleet_loss_oracle.py) against the pinned hash table, against
fleet_delay_oracle.DelayFleet at loss 0, and on the cases
tests/fleet_loss_cases.py quotes: one lost bid that stalls a fleet and the
restart that recovers it, dead links, loss before capacity, chunked runs, a
matrix that changes between calls; the ABI's argument checks and the engine's
rejections. None of it needs a GPU; the kernel is compared with the same
restatement in tests/test_gpu_fleet_loss.py."""
import ctypes as ct
import json
import os
import subprocess

import numpy as np
import pytest

import fleet_auction_cases as C
import fleet_auction_oracle as FO
import fleet_delay_cases as DC
import fleet_loss_cases as LC
import fleet_loss_oracle as LO
import test_fleet_delay as TD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1, 2: the hash ----

def test_link_hash_is_the_pinned_table():
    """tests/golden/fleet_loss_hash.json was computed from the header's formula
    by a C program (uint32_t arithmetic); P = -1 is the START of a workspace's
    first call."""
    with open(os.path.join(ROOT, "tests", "golden", "fleet_loss_hash.json")) as f:
        rows = json.load(f)["rows"]
    assert len(rows) >= 8 and any(r[3] == -1 for r in rows)
    for seed, w, u, P, it, h in rows:
        assert LO.link_hash(seed, w, u, P, it) == h, (seed, w, u, P, it)


def test_drop_rate_within_five_sigma():
    """65 536 keys at threshold 16384 (p = 1/4): sigma = sqrt(N p (1 - p)) =
    110.9, so the count lies within 555 of 16 384 (it is 16 373)."""
    lost = sum(LO.is_lost(16384, 12345, k % 13, (k // 13) % 13, k // 169, (7 * k) % 27)
               for k in range(65536))
    print("lost", lost)
    assert abs(lost - 16384) <= 5 * np.sqrt(65536 * 0.25 * 0.75)
    assert lost == 16373
    # the two ends of the range
    assert not any(LO.is_lost(0, 1, 2, 3, P, 4) for P in range(-1, 2000))
    assert all(LO.is_lost(LO.DEAD, 1, 2, 3, P, 4) for P in range(-1, 2000))


# ---- 3: loss 0 is the delay model ----

@pytest.mark.parametrize("key", TD.ALL_CASES, ids=lambda k: "-".join(str(x) for x in k))
def test_loss_zero_equals_the_delay_restatement(key):
    """Every state array, queue_len and every status dict of every window,
    for two seeds; nothing is counted as lost."""
    case, fl0, recs0 = DC.cpu_run(*key)
    for seed in (0, 0xDEADBEEF):
        fl, recs = DC.run_oracle(LC.LossCase(case, 0, seed))
        assert len(recs) == len(recs0)
        for k, (r, r0) in enumerate(zip(recs, recs0)):
            assert r["status"] == r0["status"], (key, k)
            for name in C.STATE_KEYS + ("queue_len",):
                np.testing.assert_array_equal(r["state"][name], r0["state"][name],
                                              err_msg=f"{key} window {k}: {name}")
        assert fl.tick == fl0.tick and fl.max_queue == fl0.max_queue and not fl.n_lost.any()


# ---- 4: one lost bid; a restart recovers ----

def test_one_lost_bid_stalls_the_fleet_and_a_restart_recovers():
    case = DC.draw("ring13")
    sc, n = case.sc, case.n
    fl = LC.LossCase(case, 64, 1).fleet()
    fl.lost_trace = []
    rows = np.tile(np.arange(n), (n, 1))
    q1 = sc.windows[0][1]
    a = fl.run(case.budget, q=q1, cmd=sc.cmd(0, fl), Rt=C.align_rt(sc.p, sc.adj, q1, rows))
    assert a == dict(ticks_run=54, n_open=n, n_queued=0, flags=FO.QUIESCENT)
    assert fl.n_lost.sum() == 1 and fl.n_lost[8] == 1
    assert fl.lost_trace == [(30, 8, 9, 29, 7)]  # (tick, receiver, sender, publication tick, iter)
    assert fl.open.all() and not (fl.vflags & FO.V_CONSENSUS).any()
    # window 2: everybody starts again from a new snapshot, loss 0
    q2 = C.snapshot(np.random.RandomState(77), n)
    Rt2 = C.align_rt(sc.p, sc.adj, q2, rows)
    fl.loss[:] = 0
    b = fl.run(case.budget, q=q2, cmd=np.full(n, FO.START, np.uint8), Rt=Rt2)
    assert b["flags"] == FO.QUIESCENT and b["n_open"] == 0
    who, _ = C.lockstep_tables(sc.p, sc.adj, q2, Rt2, rows[0])
    np.testing.assert_array_equal(fl.final_who, who)
    assert fl.n_thrown.sum() == 0 and fl.n_lost.sum() == 1
    assert ((fl.vflags & FO.V_CONSENSUS) != 0).all()


# ---- 5: the mixed batches, and the condition on every parity batch ----

@pytest.mark.parametrize("name", ["swarm6", "ring13"])
def test_mixed_batch_figures(name):
    runs = LC.cpu_batch("item5", name)
    figs = [LC.figures(fl, recs) for fl, recs in runs]
    print(name, figs)
    assert [f[2] for f in figs] == LC.ITEM5_LOST[name]
    assert [f[1] for f in figs] == LC.ITEM5_OPEN[name]
    assert [f[0] for f in figs] == LC.ITEM5_TICKS[name]
    assert all(recs[0]["status"]["flags"] == FO.QUIESCENT for _, recs in runs)


PARITY_BATCHES = [("item5", "swarm6"), ("item5", "ring13"), ("rings", 64), ("rings", 65),
                  ("rings", 128), ("matrices13",), ("wrap13",)]


@pytest.mark.parametrize("key", PARITY_BATCHES, ids=lambda k: "-".join(str(x) for x in k))
def test_every_parity_batch_loses_and_keeps(key):
    """A swarm that finishes with nothing lost, one with n_lost > 0 and one
    with n_open > 0 in every batch the GPU tests compare; the committed
    figures; no queue reaches its capacity."""
    runs = LC.cpu_batch(*key)
    assert LC.batch_condition(runs), key
    figs = [LC.figures(fl, recs) for fl, recs in runs]
    print(key, figs)
    want = {"rings": LC.RING_FIGURES.get(key[-1]), "matrices13": LC.MATRIX_FIGURES,
            "wrap13": LC.WRAP_FIGURES}.get(key[0])
    if want is not None:
        assert figs == want
    for fl, recs in runs:
        assert 0 < fl.max_queue < fl.cap
        assert not any(r["status"]["flags"] & FO.OVERFLOW for r in recs)


def test_matrices13_draws_every_kind_of_link():
    lcs = LC.matrices13()
    vals = set()
    for lc in lcs:
        subs = [lc.fleet().subscribed(w) for w in range(lc.n)]
        vals |= {int(lc.loss[w][u]) for w in range(lc.n) for u in subs[w]}
    assert vals == {0, 256, 4096, LO.DEAD}
    assert len({lc.loss.tobytes() for lc in lcs}) == 8  # a matrix of its own per swarm


# ---- 6, 7: dead links; loss before capacity ----

def test_dead_link():
    """The receiver never tallies past START, n_lost counts every publication
    of the sender (all were due while it subscribed), and the sender goes on
    on its other links."""
    lc, u = LC.dead_link()
    w = LC.DEAD_W
    fl, recs = DC.run_oracle(lc)
    assert u in fl.subscribed(w) and u == 0
    assert fl.n_tally[w] == 0 and fl.biditer[w] == 0 and fl.open[w]
    assert fl.n_lost[w] == LC.publications(fl, u) == 2 and fl.n_lost.sum() == fl.n_lost[w]
    assert fl.n_tally[u] >= 1 and fl.n_tally.max() == 2  # u and others went on
    assert recs[0]["status"] == dict(ticks_run=14, n_open=6, n_queued=0, flags=FO.QUIESCENT)


def test_loss_comes_before_capacity():
    """overflow6 (queue_cap 2) drops bids at vehicles 3 and 5. With every link
    into 3 dead, 3 raises no V_OVERFLOW and takes no bid: what would have been
    appended or dropped is counted in n_lost; 5 still overflows."""
    _, fl0, _ = DC.cpu_run("overflow6")
    assert fl0.vflags[3] & FO.V_OVERFLOW
    fl, recs = DC.run_oracle(LC.dead_into_3())
    assert not fl.vflags[3] & FO.V_OVERFLOW and fl.vflags[5] & FO.V_OVERFLOW
    subs = sorted(fl.subscribed(3))
    assert subs == [0, 2, 4]
    assert fl.n_lost[3] == sum(LC.publications(fl, u) for u in subs) == 6
    assert fl.n_lost.sum() == 6 and fl.n_tally[3] == 0 and len(fl.queue[3]) == 0
    assert recs[0]["status"]["flags"] == FO.QUIESCENT | FO.OVERFLOW


# ---- 8, 9: chunking; loss and seed that change between calls ----

def _same(a, b):
    TD._same(a, b)
    np.testing.assert_array_equal(a.n_lost, b.n_lost)


def _start(lc):
    sc = lc.sc
    q = sc.windows[0][1]
    rows = np.tile(np.arange(sc.n), (sc.n, 1))
    return q, C.align_rt(sc.p, sc.adj, q, rows)


def test_chunked_run_equals_one_run():
    lc = LC.LossCase(DC.draw("ring13"), 1024, 3)
    q, Rt = _start(lc)
    one, parts = lc.fleet(), lc.fleet()
    st = one.run(lc.budget, q=q, cmd=lc.sc.cmd(0, one), Rt=Rt)
    assert st == dict(ticks_run=18, n_open=13, n_queued=0, flags=FO.QUIESCENT)
    assert one.n_lost.sum() == 3
    a = parts.run(5, q=q, cmd=lc.sc.cmd(0, parts), Rt=Rt)
    b = parts.run(lc.budget)
    assert (a["ticks_run"], b["ticks_run"]) == (5, 13) and b["flags"] == FO.QUIESCENT
    _same(one, parts)


def test_loss_and_seed_of_the_call_in_which_a_bid_is_due_decide():
    """Two calls with different matrices and seeds equal a restatement that is
    given each call's pair in turn: a lossy first call (a bid is lost at tick
    30 under loss 64, seed 1), then loss 0 with another seed -- and the
    reverse order loses a different bid."""
    case = DC.draw("ring13")
    lc = LC.LossCase(case, 64, 1)
    q, Rt = _start(lc)
    # the reference: one fleet whose attributes are replaced between its runs
    ref = lc.fleet()
    ref.run(40, q=q, cmd=lc.sc.cmd(0, ref), Rt=Rt)
    assert ref.n_lost.sum() == 1
    ref.loss, ref.seed = LO.loss_matrix(13, 2048), 99
    st = ref.run(case.budget)
    # a fresh restatement of each call on a copy of the state is the same thing:
    # the fleet holds no loss state, so replaying with the pairs in turn must agree
    again = LC.LossCase(case, 64, 1).fleet()
    again.run(40, q=q, cmd=lc.sc.cmd(0, again), Rt=Rt)
    again.loss, again.seed = LO.loss_matrix(13, 2048), 99
    assert again.run(case.budget) == st
    _same(ref, again)
    assert ref.n_lost.sum() > 1
    # the pair of the due tick decides: loss 0 first, then the lossy pair, differs
    other = LC.LossCase(case, 0, 99).fleet()
    other.run(40, q=q, cmd=lc.sc.cmd(0, other), Rt=Rt)
    assert other.n_lost.sum() == 0
    other.loss, other.seed = LO.loss_matrix(13, 64), 1
    other.run(case.budget)
    assert (other.n_lost != ref.n_lost).any()


# ---- 10: the ABI and the engine without a GPU ----

_SIZE_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "aclswarm_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu ", sizeof(acl_fleet_loss_t), offsetof(acl_fleet_loss_t, loss),
         offsetof(acl_fleet_loss_t, seed), offsetof(acl_fleet_loss_t, n_lost));
  printf("%zu %zu %zu ", sizeof(acl_fleet_lossy_args_t), offsetof(acl_fleet_lossy_args_t, delay),
         offsetof(acl_fleet_lossy_args_t, link));
  printf("%zu %zu %zu ", sizeof(acl_fleet_lossy_episode_args_t),
         offsetof(acl_fleet_lossy_episode_args_t, delay),
         offsetof(acl_fleet_lossy_episode_args_t, link));
  printf("%zu %zu %zu ", sizeof(acl_fleet_lossy_trial_args_t),
         offsetof(acl_fleet_lossy_trial_args_t, delay),
         offsetof(acl_fleet_lossy_trial_args_t, link));
  printf("%zu %zu %zu %d\n", sizeof(acl_fleet_delay_args_t),
         sizeof(acl_fleet_delay_episode_args_t), sizeof(acl_fleet_delay_trial_args_t),
         ACL_ABI_VERSION);
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
    v = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert v[:4] == [ct.sizeof(L.FleetLoss), L.FleetLoss.loss.offset, L.FleetLoss.seed.offset,
                     L.FleetLoss.n_lost.offset] == [24, 0, 8, 16]
    for k, (S, D) in enumerate(((L.FleetLossyArgs, L.FleetDelayArgs),
                                (L.FleetLossyEpisodeArgs, L.FleetDelayEpisodeArgs),
                                (L.FleetLossyTrialArgs, L.FleetDelayTrialArgs))):
        size, o_delay, o_link = v[4 + 3 * k: 7 + 3 * k]
        assert size == ct.sizeof(S) == ct.sizeof(D) + 24
        assert (o_delay, o_link) == (S.delay.offset, S.link.offset) == (0, ct.sizeof(D))
        assert v[13 + k] == ct.sizeof(D)  # no existing struct changed
    assert v[16] == L.ABI_VERSION == 11  # added symbols: the ABI version stays
    assert L.FLEET_LOSS_DEAD == 0xFFFF
    for s in ("acl_fleet_lossy_auction_batch", "acl_fleet_lossy_episode_batch",
              "acl_fleet_lossy_trial_batch"):
        assert s in L.EXPORTS and hasattr(L.lib(), s)


def _filled(a, fields):
    for k, _ in fields:
        setattr(a, k, 8)  # never dereferenced: the calls below fail their checks


def _loss_errors(fails, ok_args, link):
    """The three NULL checks, each alone, after everything of the delay entry."""
    link.loss = link.seed = link.n_lost = 8
    for k, msg in (("loss", b"loss is NULL"), ("seed", b"seed is NULL"),
                   ("n_lost", b"n_lost is NULL")):
        setattr(link, k, None)
        fails(msg)
        setattr(link, k, 8)


def test_auction_argument_errors_without_gpu():
    from aclswarm_amd import _lib as L
    lib = L.lib()
    call = lib.acl_fleet_lossy_auction_batch
    name = b"acl_fleet_lossy_auction_batch: "
    F = L.Formations(129, 1, 8, 8, None, None)
    lo = L.FleetLossyArgs()
    d, a = lo.delay, lo.delay.base

    def fails(msg):
        assert call(ct.byref(F), ct.byref(lo), None) == 1  # INVALID_ARG
        err = lib.acl_last_error()
        assert err.startswith(name) and msg in err, err

    a.B, a.ticks, a.queue_cap = 1, 1, 4
    d.max_lat = 3
    fails(b"n out of range [1, 128]")
    F.n = 13
    fails(b"required pointer is NULL")
    a.queue_cap = 0
    fails(b"queue_cap < 1")
    a.queue_cap = 4
    a.ticks = -1
    fails(b"ticks < 0")
    a.ticks = 1
    _filled(a, L.FleetAuctionArgs._fields_[4:-1])
    a.hist_biditer = a.hist_open = None
    a.workspace_bytes = lib.acl_fleet_delay_workspace_bytes(13, 1, 4, 3)
    fails(b"lat is NULL")
    d.lat = 8
    for bad in (0, -1, 65):
        d.max_lat = bad
        fails(b"max_lat out of range [1, 64]")
    d.max_lat = 3
    _loss_errors(fails, None, lo.link)
    a.workspace_bytes -= 1
    fails(b"workspace_bytes is too small (acl_fleet_delay_workspace_bytes)")
    a.workspace_bytes += 1
    a.q = None
    fails(b"cmd is given and q is NULL")
    a.q = 8
    a.ticks = 0
    fails(b"at least one tick")
    F.n_formations = 0
    fails(b"formation table is empty")
    F.n_formations = 1
    a.B = 0
    lo.link.loss = None
    assert call(ct.byref(F), ct.byref(lo), None) == 0  # empty batch
    assert call(None, ct.byref(lo), None) == 1 and call(ct.byref(F), None, None) == 1
    assert lib.acl_last_error() == name + b"null argument"


def test_episode_argument_errors_without_gpu():
    from aclswarm_amd import _lib as L
    lib = L.lib()
    call = lib.acl_fleet_lossy_episode_batch
    name = b"acl_fleet_lossy_episode_batch: "
    F = L.Formations(129, 1, 8, 8, None, None)
    lo = L.FleetLossyEpisodeArgs()
    d, a = lo.delay, lo.delay.base

    def fails(msg):
        assert call(ct.byref(F), ct.byref(lo), None) == 1
        err = lib.acl_last_error()
        assert err.startswith(name) and msg in err, err

    a.B, a.steps, a.ticks_per_step, a.queue_cap = 1, 1, 1, 4
    a.ep = L.default_episode_params()
    d.max_lat = 3
    fails(b"n out of range [1, 128]")
    F.n = 13
    fails(b"required pointer is NULL")
    a.ticks_per_step = 0
    fails(b"ticks_per_step < 1")
    a.ticks_per_step = 1
    a.queue_cap = 0
    fails(b"queue_cap < 1")
    a.queue_cap = 4
    a.ep.auction_latency = 1
    fails(b"auction_latency")
    a.ep.auction_latency = 0
    d.max_lat = 65
    fails(b"max_lat out of range [1, 64]")
    d.max_lat = 3
    _filled(a, [f for f in L.FleetEpisodeArgs._fields_ if f[1] is ct.c_void_p])
    for k in ("q_hist", "vel_hist", "u_hist", "ca_hist", "P_hist", "vflags_hist"):
        setattr(a, k, None)
    a.workspace_bytes = lib.acl_fleet_delay_episode_workspace_bytes(13, 1, 4, 3)
    fails(b"lat is NULL")
    d.lat = 8
    _loss_errors(fails, None, lo.link)
    a.workspace_bytes -= 1
    fails(b"workspace_bytes is too small (acl_fleet_delay_episode_workspace_bytes)")
    a.steps = 0
    assert call(ct.byref(F), ct.byref(lo), None) == 0  # nothing to fly
    assert call(ct.byref(F), None, None) == 1
    assert lib.acl_last_error() == name + b"null argument"


def test_trial_argument_errors_without_gpu():
    from aclswarm_amd import _lib as L
    lib = L.lib()
    call = lib.acl_fleet_lossy_trial_batch
    name = b"acl_fleet_lossy_trial_batch: "
    F = L.Formations(129, 1, 8, 8, None, None)
    lo = L.FleetLossyTrialArgs()
    d, a = lo.delay, lo.delay.base

    def fails(msg):
        assert call(ct.byref(F), ct.byref(lo), None) == 1
        err = lib.acl_last_error()
        assert err.startswith(name) and msg in err, err

    a.B, a.K, a.steps, a.ticks_per_step, a.queue_cap = 1, 1, 1, 1, 4
    a.tp = L.default_trial_params()
    d.max_lat = 3
    fails(b"n out of range [1, 128]")
    F.n = 13
    fails(b"required pointer is NULL")
    a.K = 0
    fails(b"K >= 1")
    a.K = 1
    a.ticks_per_step = 0
    fails(b"ticks_per_step < 1")
    a.ticks_per_step = 1
    a.tp.ep.assignment = 1
    fails(b"assignment")
    a.tp.ep.assignment = 0
    d.max_lat = 0
    fails(b"max_lat out of range [1, 64]")
    d.max_lat = 3
    _filled(a, [f for f in L.FleetTrialArgs._fields_ if f[1] is ct.c_void_p])
    for k in ("q_hist", "vel_hist", "u_hist", "ca_hist", "ctl_hist", "P_hist", "state_hist",
              "vflags_hist"):
        setattr(a, k, None)
    a.workspace_bytes = lib.acl_fleet_delay_trial_workspace_bytes(13, 1, 4, 3)
    fails(b"lat is NULL")
    d.lat = 8
    _loss_errors(fails, None, lo.link)
    a.workspace_bytes -= 1
    fails(b"workspace_bytes is too small (acl_fleet_delay_trial_workspace_bytes)")
    a.workspace_bytes += 1
    F.n_formations = 0
    fails(b"n_formations < 1")
    a.steps = 0
    assert call(ct.byref(F), ct.byref(lo), None) == 0
    assert call(ct.byref(F), None, None) == 1 and call(None, ct.byref(lo), None) == 1
    assert lib.acl_last_error() == name + b"null argument"


def _bad_loss_arguments(B, n):
    import torch
    loss = torch.full((B, n, n), 64, dtype=torch.int16)
    seed = torch.zeros(B, dtype=torch.int32)
    return [
        dict(loss=-1), dict(loss=65536),                                # an int outside 0..65535
        dict(loss=True), dict(loss=0.5), dict(loss=64.0),               # a bool, a float
        dict(loss=loss.to(torch.int32)), dict(loss=loss.to(torch.uint8)),  # wrong dtype
        dict(loss=loss[:, :, :-1].contiguous()), dict(loss=loss[0]),    # wrong shape
        dict(loss=loss.transpose(1, 2)),                                # non-contiguous
        dict(loss=torch.full((B, n, n), 64, dtype=torch.int16, device="meta")),  # device
        dict(loss_seed=3), dict(loss_seed=seed),                        # without loss
        dict(loss=64, loss_seed=-1), dict(loss=64, loss_seed=1 << 32),  # outside u32
        dict(loss=64, loss_seed=True), dict(loss=64, loss_seed=1.0),
        dict(loss=64, loss_seed=seed.to(torch.int64)),                  # wrong dtype
        dict(loss=64, loss_seed=torch.zeros(B + 1, dtype=torch.int32)),  # wrong shape
        dict(loss=64, loss_seed=torch.zeros(2 * B, dtype=torch.int32)[::2]),  # non-contiguous
        dict(loss=64, loss_seed=torch.zeros(B, dtype=torch.int32, device="meta")),
        dict(loss=64, latency=0),                                       # the latency checks stay
    ]


def test_fleet_auction_loss_rejections_without_gpu():
    """engine.FleetAuction(loss=, loss_seed=) raises ValueError before anything
    runs, one case per rule; a good loss picks the delay entry's workspace,
    with every link at 1 tick unless latency says otherwise; the attributes
    can be replaced, with the same checks."""
    import torch
    from aclswarm_amd import _lib as L
    from aclswarm_amd import engine
    n, B = 13, 3
    T = TD._cpu_table(n)
    fidx = torch.zeros(B, dtype=torch.int32)
    for kw in _bad_loss_arguments(B, n):
        with pytest.raises(ValueError):
            engine.FleetAuction(T, fidx, **kw)
    lib = L.lib()
    plain = engine.FleetAuction(T, fidx)
    assert plain.loss is None and plain.loss_seed is None and plain.n_lost is None
    with pytest.raises(ValueError):
        plain.loss = 64  # its workspace is not the delay layout
    fa = engine.FleetAuction(T, fidx, loss=64)
    assert fa.max_latency == 1 and (fa.latency == 1).all()
    assert fa.workspace_bytes() == lib.acl_fleet_delay_workspace_bytes(n, B, 4 * n, 1)
    assert fa.loss.dtype == torch.int16 and tuple(fa.loss.shape) == (B, n, n)
    assert (fa.loss == 64).all() and fa.loss_seed.tolist() == [0, 1, 2]
    assert fa.n_lost.dtype == torch.int32 and tuple(fa.n_lost.shape) == (B, n)
    assert not fa.n_lost.any()
    fb = engine.FleetAuction(T, fidx, latency=3, loss=0xFFFF, loss_seed=0xFFFFFFFE)
    assert fb.workspace_bytes() == lib.acl_fleet_delay_workspace_bytes(n, B, 4 * n, 3)
    assert (fb.loss.view(torch.int16).to(torch.int32) & 0xFFFF == 0xFFFF).all()
    assert (fb.loss_seed.to(torch.int64) & 0xFFFFFFFF).tolist() == [0xFFFFFFFE, 0xFFFFFFFF, 0]
    m = torch.full((B, n, n), 7, dtype=torch.int16)
    fb.loss = m
    assert fb.loss is not m and (fb.loss == 7).all()
    fb.loss_seed = torch.tensor([5, 6, 7], dtype=torch.int32)
    assert fb.loss_seed.tolist() == [5, 6, 7]
    for bad in (-1, 65536, 1.0, True, m.to(torch.int32), m[0]):
        with pytest.raises(ValueError):
            fb.loss = bad
    for bad in (-1, 1 << 32, 2.0, False, torch.zeros(B, dtype=torch.int64)):
        with pytest.raises(ValueError):
            fb.loss_seed = bad
    assert (fb.loss == 7).all() and fb.loss_seed.tolist() == [5, 6, 7]  # a refusal changes nothing
    fb.loss = None  # back to the delay entry on the same workspace
    assert fb.loss is None and fb.workspace_bytes() == \
        lib.acl_fleet_delay_workspace_bytes(n, B, 4 * n, 3)
    fb.loss = 16
    q = torch.zeros((B, n, 3), dtype=torch.float64)
    cmd = torch.ones((B, n), dtype=torch.uint8)
    with pytest.raises(ValueError):  # not on a GPU
        fb.run(4, q=q, cmd=cmd)
    assert fb.ws is None  # nothing was allocated or launched
