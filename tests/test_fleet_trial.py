"""CPU suite of the trials on the message-level auction
(acl_fleet_trial_batch): every case of tests/fleet_trial_cases.py on the
restatement alone (tests/fleet_trial_oracle.py), so that a case that stops
covering its edge fails here; the pin of the new model to the synchronous one
where they must agree; the ABI of the new structs and the rejections of
engine.FleetTrial without a GPU."""
import ctypes as ct
import os
import subprocess

import numpy as np
import pytest

import fleet_auction_cases as FA
import fleet_auction_oracle as FO
import fleet_trial_cases as K
import trial_oracle as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _first(recs, pred):
    return next((r["step"] for r in recs if pred(r)), -1)


def _commits(recs):
    return [r for r in recs if r["committed"]]


# ---- the pin: one clean auction per step is the synchronous trial ----

@pytest.mark.parametrize("name", ["sync6_two", "sync6_reassign"])
def test_sync6_equals_the_synchronous_trial_bit_for_bit(name):
    """ticks_per_step = 60 holds one clean auction of six vehicles on the
    complete graph (2 n (n - 1) ticks): every auction is over within its step,
    every vehicle adopts together, and the trial is trial_oracle.run_trial's:
    the supervisor's state after every step, the final q and vel and the
    record, bit for bit."""
    cs, ft, recs = K.cpu_run(name)
    t, q, vel, states = T.run_trial(cs.q, cs.vel, cs.fseq, cs.forms, cs.tp, cs.steps)
    assert [r["state"] for r in recs] == states
    assert ft.sup.state == T.COMPLETE and len(recs) < cs.steps
    np.testing.assert_array_equal(ft.q.view(np.uint64), q.view(np.uint64))
    np.testing.assert_array_equal(ft.vel.view(np.uint64), vel.view(np.uint64))
    a, b = ft.sup.record(), t.sup.record()
    np.testing.assert_array_equal(np.asarray(a.pop("dist")).view(np.uint64),
                                  np.asarray(b.pop("dist")).view(np.uint64))
    assert a == b
    assert ft.n_auctions == t.counts["auctions"] and ft.fst["n_restarted"] == 0
    assert ft.fst["n_invalid"] == 0 and not ft.fleet.n_thrown.any()


# ---- the cases ----

@pytest.mark.parametrize("name", ["interrupt6", "interrupt13"])
def test_a_formation_change_interrupts_a_running_auction(name):
    cs, ft, recs = K.cpu_run(name)
    first, second = _commits(recs)
    assert first["before"]["open"].sum() == 0 and first["before"]["queued"].sum() == 0
    # the second formation commits onto open auctioneers with queued bids ...
    assert second["before"]["open"].sum() >= 1 and second["before"]["queued"].sum() >= 1
    # ... which stay queued, and are thrown away in the new formation's auction
    thrown_at = recs[second["step"] - 1]["n_thrown"].sum()
    assert ft.fleet.n_thrown.sum() > thrown_at
    assert (ft.sup.state, ft.sup.last_state) == (T.COMPLETE, T.HOVERING)
    assert ft.sup.record()["assignments"] == [1, 1]
    # the interrupted auction delays the trial against the synchronous model
    t, _, _, states = T.run_trial(cs.q, cs.vel, cs.fseq, cs.forms, cs.tp, cs.steps)
    assert t.sup.state == T.COMPLETE and len(states) < len(recs)


def test_auctions_longer_than_the_period_never_finish():
    cs, ft, recs = K.cpu_run("restart13")
    assert 2 * 13 * 12 > cs.T * cs.tp["ep"]["auction_every"]  # ticks an auction needs / has
    cmds = [r for r in recs if r["cmd"] is not None]
    assert len(cmds) >= 3 and all((r["cmd"] == FO.START).all() for r in cmds)
    assert cmds[0]["before"]["open"].sum() == 0
    assert all(r["before"]["open"].all() for r in cmds[1:])  # every later START is a restart
    assert ft.fst["n_restarted"] == 13 * (len(cmds) - 1)
    assert ft.fst["n_consensus"] == 0 and ft.fst["n_adopted"] == 0
    assert not any(r["ctl_on"].any() for r in recs)
    assert (ft.sup.state, ft.sup.last_state) == (T.TERMINATE, T.WAITING)
    # the synchronous trial completes the same swarm
    t, _, _, _ = T.run_trial(cs.q, cs.vel, cs.fseq, cs.forms, cs.tp, 400)
    assert t.sup.state == T.COMPLETE


def test_controllers_start_vehicle_by_vehicle_and_the_supervisor_hears_vehicle_0():
    cs, ft, recs = K.cpu_run("stagger13_t2")
    ad = K.adoption_steps(recs)
    assert len(ad) >= 2 and sum(len(v) for v in ad.values()) == 13
    s_first = min(ad)
    s0 = next(s for s, v in ad.items() if 0 in v)
    assert s0 > s_first  # vehicle 0 is not in the first group
    for s, vs in ad.items():
        assert recs[s]["ctl_on"][vs].all()
    assert 0 < recs[s_first]["ctl_on"].sum() < 13 and recs[s_first]["per_vehicle"] == 1
    # WAITING -> FLYING at the first supervisor tick at or after vehicle 0's adoption
    every = cs.tp["ep"]["sample_every"]
    tick = s0 if s0 % every == 0 else s0 + every - s0 % every
    assert _first(recs, lambda r: r["state"] == T.FLYING) == tick
    assert all(r["state"] == T.WAITING for r in recs[s_first:tick])
    assert ft.sup.record()["assignments"] == [1]


def test_invalid_consensus_and_flush_alternate_vehicle_by_vehicle():
    cs, ft, recs = K.cpu_run("rings12_invalid")
    cmds = [r for r in recs if r["cmd"] is not None]
    assert len(cmds) >= 4
    for k, r in enumerate(cmds):
        assert (r["cmd"] == (FO.START if k % 2 == 0 else FO.FLUSH)).all()
    inv = [r["step"] for r in recs if (r["raised"] & FO.V_INVALID).any()]
    starts = [r["step"] for r in cmds[::2]]
    assert len(inv) >= 2 and all(a < b for a, b in zip(starts, inv))
    assert all(((r["raised"] & FO.V_INVALID) != 0).sum() in (0, 12) for r in recs)
    assert ft.fst["n_invalid"] == ft.fst["n_flushed"] == 12 * len(inv)
    assert ft.fst["n_adopted"] == 0 and not any(r["ctl_on"].any() for r in recs)
    assert (ft.sup.state, ft.sup.last_state) == (T.TERMINATE, T.WAITING)


def test_ring65_adoptions_spread_over_steps():
    cs, ft, recs = K.cpu_run("ring65")
    ad = K.adoption_steps(recs)
    assert len(ad) >= 2 and sum(len(v) for v in ad.values()) == 65
    assert any(64 in v for v in ad.values())  # the second wave's one live lane
    assert ft.sup.state == T.FLYING and ft.fst["n_restarted"] == 0


def test_near128_some_adopt_and_the_others_flag_invalid():
    cs, ft, recs = K.cpu_run("near128")
    ad = K.adoption_steps(recs)
    who = sorted(sum(ad.values(), []))
    assert 0 in who and 127 in who and 0 < len(who) < 128
    assert ft.fst["n_invalid"] == 128 - len(who) and ft.fst["n_consensus"] == 128
    assert (ft.fleet.invalid != 0).sum() == 128 - len(who)
    assert (ft.t.ctl_on.nonzero()[0] == who).all()
    assert ft.per_vehicle == 1 and any(v >= 64 for v in who)
    s0 = next(s for s, v in ad.items() if 0 in v)
    assert _first(recs, lambda r: r["state"] == T.FLYING) in (s0, s0 + 1)
    assert recs[-1]["state"] == T.FLYING


def test_interrupt128_commits_onto_open_queued_and_in_flight():
    cs, ft, recs = K.cpu_run("interrupt128")
    first, second = _commits(recs)
    assert second["step"] == K.INTERRUPT128_AT
    b = second["before"]
    assert b["open"].all() and b["queued"].sum() >= 1
    fly = np.array(b["inflight"])
    assert fly[:64].any() and fly[64:].any()  # both task slots' vehicles have a bid in flight
    assert ft.t.fidx == 1 and ft.fleet.n_thrown.sum() > recs[second["step"] - 1]["n_thrown"].sum()
    assert (ft.fleet.just_received == 1).all() and not ft.t.ctl_on.any()


# ---- the ABI ----

_LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "aclswarm_amd.h"
#define P(f) printf(#f " %zu\n", offsetof(acl_fleet_trial_args_t, f));
int main(void) {
  printf("sizeof %zu abi %d\n", sizeof(acl_fleet_trial_args_t), ACL_ABI_VERSION);
  P(B) P(K) P(step0) P(steps) P(ticks_per_step) P(max_iter) P(queue_cap) P(fseq) P(fidx) P(q)
  P(vel) P(P) P(ts) P(ctl_on) P(ring_u) P(ring_ca) P(posf) P(dist) P(t_conv) P(t_avoid)
  P(n_assign) P(Pt) P(open) P(invalid) P(just_received) P(biditer) P(price) P(who) P(Rt)
  P(final_price) P(final_who) P(done_tick) P(vflags) P(n_thrown) P(n_tally) P(queue_len)
  P(status) P(adopt_step) P(fst) P(q_hist) P(vel_hist) P(u_hist) P(ca_hist) P(ctl_hist)
  P(P_hist) P(state_hist) P(vflags_hist) P(workspace) P(workspace_bytes) P(cntrl) P(safety)
  P(tp)
  return 0;
}
"""


def test_struct_layout_matches_ctypes(tmp_path):
    from aclswarm_amd import _lib as L
    src = tmp_path / "layout.c"
    src.write_text(_LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split("\n")
    head = out[0].split()
    assert int(head[1]) == ct.sizeof(L.FleetTrialArgs)
    assert int(head[3]) == L.ABI_VERSION == 11  # an added symbol: the ABI version stays
    seen = []
    for line in out[1:]:
        if line:
            f, off = line.split()
            assert getattr(L.FleetTrialArgs, f).offset == int(off), f
            seen.append(f)
    assert seen == [f[0] for f in L.FleetTrialArgs._fields_]
    fixed = 7 * 4 + 4 + 41 * 8 + 8
    assert ct.sizeof(L.FleetTrialArgs) == fixed + ct.sizeof(L.CntrlGains) + \
        ct.sizeof(L.SafetyParams) + ct.sizeof(L.TrialParams)


def test_workspace_bytes():
    from aclswarm_amd import _lib as L
    lib = L.lib()
    for n, B, cap in ((13, 8, 52), (20, 4, 80), (128, 2, 512), (1, 1, 1)):
        need = lib.acl_fleet_trial_workspace_bytes(n, B, cap)
        # the fleet workspace, the control hand-off region, u and u_safe (f64),
        # ca and cmd (u8), the step's flags (i32)
        assert need >= lib.acl_fleet_workspace_bytes(n, B, cap) + \
            lib.acl_solve_workspace_bytes(n, B) + B * n * (48 + 2 + 4)
        assert need >= lib.acl_fleet_episode_workspace_bytes(n, B, cap)
    assert lib.acl_fleet_trial_workspace_bytes(129, 1, 4) == 0
    assert lib.acl_fleet_trial_workspace_bytes(13, 0, 4) == 0
    assert lib.acl_fleet_trial_workspace_bytes(13, 1, 0) == 0


@pytest.mark.parametrize("entry", ["init", "batch"])
def test_argument_errors_without_gpu(entry):
    from aclswarm_amd import _lib as L
    lib = L.lib()
    F = L.Formations(129, 1, 8, 8, None, None)
    a = L.FleetTrialArgs()
    a.B, a.K, a.steps, a.ticks_per_step, a.queue_cap = 1, 2, 1, 10, 4
    lib.acl_default_trial_params(ct.byref(a.tp))

    def call():
        if entry == "init":
            return lib.acl_fleet_trial_init(ct.byref(a), F.n, None)
        return lib.acl_fleet_trial_batch(ct.byref(F), ct.byref(a), None)

    def err():
        assert call() == 1  # INVALID_ARG
        return lib.acl_last_error()
    assert b"n out of range [1, 128]" in err()
    F.n = 0
    assert b"n out of range [1, 128]" in err()
    F.n = 13
    assert b"NULL" in err()
    a.K = 0
    assert b"K >= 1" in err()
    a.K = 2
    a.ticks_per_step = 0
    assert b"ticks_per_step" in err()
    a.ticks_per_step = 10
    a.queue_cap = 0
    assert b"queue_cap" in err()
    a.queue_cap = 4
    a.max_iter = -1
    assert b"max_iter" in err()
    a.max_iter = 0
    a.tp.ep.auction_latency = -1
    assert b"auction_latency" in err()
    a.tp.ep.auction_latency = 0
    a.tp.ep.assignment = 1
    assert b"assignment" in err()
    a.tp.ep.assignment = 0
    a.tp.settle_steps = -1
    assert b"settle_steps" in err()
    a.tp.settle_steps = 150
    ptrs = [k for k, t in L.FleetTrialArgs._fields_ if t is ct.c_void_p]
    assert len(ptrs) == 41
    optional = ("q_hist", "vel_hist", "u_hist", "ca_hist", "ctl_hist", "P_hist", "state_hist",
                "vflags_hist")
    for k in ptrs:
        setattr(a, k, None if k in optional else 8)  # never dereferenced: the calls fail
    for k in ptrs:
        if k in optional:
            continue
        setattr(a, k, None)
        assert b"NULL" in err(), k
        setattr(a, k, 8)
    a.workspace_bytes = lib.acl_fleet_trial_workspace_bytes(13, 1, 4) - 1
    assert b"workspace_bytes" in err()
    if entry == "batch":
        a.steps = 0
        assert call() == 0  # nothing to fly, before any pointer is looked at
        a.steps = 1
        assert lib.acl_fleet_trial_batch(None, ct.byref(a), None) == 1
        assert lib.acl_fleet_trial_batch(ct.byref(F), None, None) == 1
    else:
        assert lib.acl_fleet_trial_init(None, 13, None) == 1
    a.B = 0
    for k in ptrs:
        setattr(a, k, None)
    assert call() == 0  # empty batch


# ---- engine.FleetTrial without a GPU ----

def _cpu_table(n):
    from aclswarm_amd import engine
    return engine.FormationTable.from_host([np.zeros((n, 3))], [FA.chord_ring(n)], None,
                                           device="cpu")


def test_fleet_trial_rejections_without_gpu():
    """engine.FleetTrial raises ValueError before anything is allocated, one
    case per rule (CPU tensors: the last rule, a CUDA device, rejects what
    passes the others)."""
    import torch
    import aclswarm_amd
    from aclswarm_amd import _lib as L
    from aclswarm_amd import engine
    assert aclswarm_amd.FleetTrial is engine.FleetTrial
    n, B = 13, 2
    Tb = _cpu_table(n)
    fseq = torch.zeros((B, 2), dtype=torch.int32)
    q = torch.zeros((B, n, 3), dtype=torch.float64)
    lat = L.default_trial_params()
    lat.ep.auction_latency = -1
    cen = L.default_trial_params()
    cen.ep.assignment = 1
    bad = [
        (dict(q=q.numpy()), "q must be"),                                    # type
        (dict(q=q[0]), "q must be"),                                         # shape
        (dict(q=q[:0]), "empty"),
        (dict(q=q.to(torch.float32)), "q must be a contiguous"),             # dtype
        (dict(vel=q[:, :, :2].contiguous()), "vel must be a contiguous"),    # shape
        (dict(vel=q.transpose(0, 1).contiguous().transpose(0, 1)), "vel"),   # strides
        (dict(vel=None), "vel must be a torch tensor"),
        (dict(fseq=fseq.to(torch.int64)), "fseq"),                           # dtype
        (dict(fseq=fseq[:1]), "fseq"),                                       # shape
        (dict(fseq=fseq[:, :0]), "fseq"),                                    # K = 0
        (dict(fseq=fseq[:, 0]), "fseq"),                                     # rank
        (dict(fseq=torch.zeros((B, 2), dtype=torch.int32, device="meta")), "fseq"),  # devices
        (dict(queue_cap=0), "queue_cap"),
        (dict(max_iter=-1), "max_iter"),
        (dict(ticks_per_step=0), "ticks_per_step"),
        (dict(params=lat), "auction_latency"),
        (dict(params=cen), "assignment"),
        (dict(), "CUDA device"),                                             # not on a GPU
    ]
    for kw, msg in bad:
        args = dict(dict(fseq=fseq, q=q, vel=q), **kw)
        with pytest.raises(ValueError, match=msg):
            engine.FleetTrial(Tb, args.pop("fseq"), args.pop("q"), args.pop("vel"), **args)
    with pytest.raises(ValueError, match="out of range"):                    # n > 128
        engine.FleetTrial(_cpu_table(129), fseq, torch.zeros((B, 129, 3), dtype=torch.float64),
                          torch.zeros((B, 129, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="formation table is on"):           # the table's device
        m = dict(dtype=torch.float64, device="meta")
        engine.FleetTrial(Tb, torch.zeros((B, 2), dtype=torch.int32, device="meta"),
                          torch.zeros((B, n, 3), **m), torch.zeros((B, n, 3), **m))
