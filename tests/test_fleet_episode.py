"""CPU suite of the episodes on the message-level auction
(acl_fleet_episode_batch): the facts each shared case exists for, on the
plain-Python restatement alone (tests/fleet_episode_oracle.py), so that a case
which stops reaching its edge fails without a GPU; the ABI's struct sizes,
prototypes and argument checks; and engine.FleetEpisode's rejections. The GPU
loop is compared with the same restatement in tests/test_gpu_fleet_episode.py."""
import ctypes as ct

import numpy as np
import pytest

import fleet_auction_cases as C
import fleet_auction_oracle as FO
import fleet_episode_cases as K

CLEAN = FO.V_CONSENSUS | FO.V_ADOPTED
BAD = FO.V_CONSENSUS | FO.V_INVALID


def _raised(recs):
    """{step: sorted flag words raised by some vehicle}, steps without any left out."""
    return {r["step"]: sorted(set(int(x) for x in r["raised"] if x)) for r in recs
            if r["raised"].any()}


def test_ring13_adopts_in_step_7_and_restarts_at_12():
    cs, ep, recs = K.cpu_run("ring13")
    assert (recs[7]["done_tick"].min(), recs[7]["done_tick"].max()) == (72, 77)
    assert _raised(recs) == {0: [FO.V_STARTED], 7: [CLEAN], 12: [FO.V_STARTED], 19: [CLEAN],
                             24: [FO.V_STARTED]}
    assert K.adoption_steps(recs) == {7: 13, 19: 13}
    assert (ep.adopt_step == 19).all()
    assert not any(r["per_vehicle"] for r in recs)
    assert [r["status"]["ticks_run"] for r in recs[:13]] == [10] * 7 + [8] + [0] * 4 + [10]
    assert ep.fst["n_restarted"] == 0 and ep.fst["n_flushed"] == 0 and ep.fst["n_started"] == 39
    assert ep.sup.n_samples == 15  # the window (bufflen 5) filled: predicates evaluated


def test_ring13_two_ticks_per_step_flies_mixed_rows_for_two_steps():
    """What the synchronous episode cannot show: the vehicles adopt at
    different steps, and in between each flies its own row."""
    cs, ep, recs = K.cpu_run("ring13_t2")
    assert K.adoption_steps(recs) == {36: 5, 37: 4, 38: 4}
    assert [r["step"] for r in recs if r["per_vehicle"]] == [36, 37]
    assert sorted(set(ep.adopt_step.tolist())) == [36, 37, 38]
    assert (ep.fleet.done_tick.min(), ep.fleet.done_tick.max()) == (72, 77)
    assert (ep.fleet.Pt == ep.fleet.Pt[0]).all()  # one table again


def test_stale13_windows():
    cs, ep, recs = K.cpu_run("stale13")
    n = 13
    # step 0: vehicle 3 flushes, the other twelve stall (quiescent after 11 ticks)
    assert recs[0]["cmd"].tolist() == [FO.START] * 3 + [FO.FLUSH] + [FO.START] * 9
    assert [r["status"]["ticks_run"] for r in recs[:12]] == [10, 1] + [0] * 10
    assert recs[1]["status"]["flags"] & FO.QUIESCENT and recs[1]["open"].sum() == 12
    # step 12: all start, 12 of them restarts seeded with the stale START
    # bids; all reach consensus on an invalid table at ticks 83-88
    assert (recs[12]["cmd"] == FO.START).all() and recs[11]["open"].sum() == 12
    assert _raised(recs[12:24]) == {12: [FO.V_STARTED], 19: [BAD]}
    assert (recs[19]["done_tick"].min(), recs[19]["done_tick"].max()) == (83, 88)
    assert recs[19]["invalid"].all() and ep.fleet.n_thrown.sum() > 0
    # step 24: all 13 flush
    assert (recs[24]["cmd"] == FO.FLUSH).all() and not recs[24]["invalid"].any()
    assert not recs[24]["raised"].any() and recs[24]["status"]["ticks_run"] == 0
    # step 36: a clean auction, everybody adopts at relative ticks 72-77
    t0 = recs[35]["tick"]
    assert (recs[36]["cmd"] == FO.START).all() and t0 == 89
    assert _raised(recs[36:]) == {36: [FO.V_STARTED], 43: [CLEAN]}
    assert (ep.fleet.done_tick.min() - t0, ep.fleet.done_tick.max() - t0) == (72, 77)
    assert (ep.adopt_step == 43).all() and not any(r["per_vehicle"] for r in recs)
    f = ep.fst
    assert (f["n_restarted"], f["n_invalid"], f["n_flushed"]) == (12, 13, 14)
    assert (f["n_started"], f["n_consensus"], f["n_adopted"]) == (12 + 13 + 13, 26, 13)
    assert f["ticks_run"] == 11 + 78 + 78 and f["flags"] == 0


def test_rings12_components_go_their_own_ways():
    cs, ep, recs = K.cpu_run("rings12")
    # ring B (6..11) reaches consensus at tick 47 on a table six tasks short
    assert _raised(recs[:12]) == {0: [FO.V_STARTED], 4: [BAD]}
    assert recs[4]["done_tick"][6:].tolist() == [47] * 6
    assert recs[4]["invalid"].tolist() == [0] * 6 + [1] * 6
    assert not K.adoption_steps(recs)
    # ring A stalls on vehicle 2, which flushed
    assert recs[0]["cmd"][2] == FO.FLUSH
    assert recs[11]["open"].tolist() == [1, 1, 0, 1, 1, 1] + [0] * 6
    # step 12: ring B flushes, ring A restarts on its own
    assert recs[12]["cmd"].tolist() == [FO.START] * 6 + [FO.FLUSH] * 6
    assert recs[12]["open"].tolist() == [1] * 6 + [0] * 6
    f = ep.fst
    assert (f["n_started"], f["n_restarted"], f["n_flushed"]) == (11 + 6 + 6, 5, 1 + 6 + 6)
    assert f["n_adopted"] == 0 and f["n_invalid"] == 12


def test_ring65_adoptions_spread_over_three_steps():
    cs, ep, recs = K.cpu_run("ring65")
    assert (ep.fleet.done_tick.min(), ep.fleet.done_tick.max()) == (365, 389)
    assert sorted(K.adoption_steps(recs)) == [36, 37, 38]
    assert sum(K.adoption_steps(recs).values()) == 65
    assert [r["step"] for r in recs if r["per_vehicle"]] == [36, 37]
    assert ep.fst["ticks_run"] == 390


@pytest.mark.parametrize("name", ["odd_last128", "odd_last128_col"])
def test_odd_last128_flies_per_vehicle_rows_from_step_0(name):
    cs, ep, recs = K.cpu_run(name)
    n = 128
    rows = cs.Pt
    if name == "odd_last128":  # only the last row differs
        assert (rows[:127] == np.arange(n)).all() and (rows[127] != np.arange(n)).sum() == 2
    else:  # only the last two columns differ
        assert (rows[:, :126] == np.arange(126)).all() and (rows[:126] == np.arange(n)).all()
        assert rows[126:, 126:].tolist() == [[127, 126]] * 2
    assert all(r["per_vehicle"] for r in recs) and not K.adoption_steps(recs)
    assert ep.fst["ticks_run"] == 48 and ep.fst["n_invalid"] == n and ep.fleet.invalid.all()
    assert (ep.fleet.Pt == rows).all()
    # the odd rows matter to the controller: under the shared table the
    # vehicles that hold them would fly another command
    import episode_oracle as E
    shared = np.tile(np.arange(n), (n, 1)).astype(np.uint16)
    u1, _, _ = E.control_step(cs.q0, cs.vel0, cs.p, cs.adj, cs.gains, ep.P,
                              tables=rows.astype(np.uint16))
    u0, _, _ = E.control_step(cs.q0, cs.vel0, cs.p, cs.adj, cs.gains, np.arange(n), tables=shared)
    odd = [127] if name == "odd_last128" else [126, 127]
    for v in odd:
        assert np.abs(u1[v] - u0[v]).max() > 1e-3 * np.abs(u0[v]).max()


def test_chunk_boundaries_do_not_matter_to_the_restatement():
    """The restatement's fleet carries on from its stored state: the shared
    run equals a fresh one (determinism of the cases the GPU tests lean on)."""
    cs, ep, recs = K.cpu_run("ring13_t2")
    ep2 = cs.oracle()
    for s in range(cs.steps):
        r = ep2.step()
        np.testing.assert_array_equal(r["raised"], recs[s]["raised"])
    np.testing.assert_array_equal(ep2.q, ep.q)


# ---- the ABI and engine.FleetEpisode without a GPU ----

def test_abi_struct_sizes_and_workspace_bytes():
    from aclswarm_amd import _lib as L
    lib = L.lib()
    assert L.FLEET_EPISODE_STATUS_DTYPE.itemsize == 32
    fixed = 6 * 4 + 32 * 8 + 8
    assert ct.sizeof(L.FleetEpisodeArgs) == fixed + ct.sizeof(L.CntrlGains) + \
        ct.sizeof(L.SafetyParams) + ct.sizeof(L.EpisodeParams)
    assert L.FleetEpisodeArgs.ep.offset % 8 == 0
    for n, B, cap in ((13, 8, 52), (20, 4, 80), (128, 2, 512), (1, 1, 1)):
        need = lib.acl_fleet_episode_workspace_bytes(n, B, cap)
        assert need >= lib.acl_fleet_workspace_bytes(n, B, cap) + \
            lib.acl_solve_workspace_bytes(n, B)
        # ... plus u, u_safe (f64) and ca, cmd (u8), the step's flags (i32)
        assert need >= lib.acl_fleet_workspace_bytes(n, B, cap) + \
            lib.acl_solve_workspace_bytes(n, B) + B * n * (48 + 2 + 4)
    assert lib.acl_fleet_episode_workspace_bytes(129, 1, 4) == 0
    assert lib.acl_fleet_episode_workspace_bytes(13, 0, 4) == 0
    assert lib.acl_fleet_episode_workspace_bytes(13, 1, 0) == 0


def test_abi_argument_errors_without_gpu():
    from aclswarm_amd import _lib as L
    lib = L.lib()
    F = L.Formations(129, 1, 8, 8, None, None)
    a = L.FleetEpisodeArgs()
    a.B, a.steps, a.ticks_per_step, a.queue_cap = 1, 1, 10, 4
    lib.acl_default_episode_params(ct.byref(a.ep))

    def err():
        assert lib.acl_fleet_episode_batch(ct.byref(F), ct.byref(a), None) == 1  # INVALID_ARG
        return lib.acl_last_error()
    assert b"n out of range [1, 128]" in err()
    F.n = 0
    assert b"n out of range [1, 128]" in err()
    F.n = 13
    assert b"NULL" in err()
    a.ticks_per_step = 0
    assert b"ticks_per_step" in err()
    a.ticks_per_step = 10
    a.queue_cap = 0
    assert b"queue_cap" in err()
    a.queue_cap = 4
    a.ep.auction_latency = -1
    assert b"auction_latency" in err()
    a.ep.auction_latency = 0
    a.ep.assignment = 1
    assert b"assignment" in err()
    a.ep.assignment = 0
    ptrs = [k for k, t in L.FleetEpisodeArgs._fields_ if t is ct.c_void_p]
    assert len(ptrs) == 32
    optional = ("q_hist", "vel_hist", "u_hist", "ca_hist", "P_hist", "vflags_hist")
    for k in ptrs:
        setattr(a, k, None if k in optional else 8)  # never dereferenced: the calls fail
    for k in ptrs:
        if k in optional:
            continue
        setattr(a, k, None)
        assert b"NULL" in err(), k
        setattr(a, k, 8)
    a.workspace_bytes = lib.acl_fleet_episode_workspace_bytes(13, 1, 4) - 1
    assert b"workspace_bytes" in err()
    a.steps = 0
    assert lib.acl_fleet_episode_batch(ct.byref(F), ct.byref(a), None) == 0  # nothing to fly
    a.steps, a.B = 1, 0
    assert lib.acl_fleet_episode_batch(ct.byref(F), ct.byref(a), None) == 0  # empty batch
    assert lib.acl_fleet_episode_batch(None, ct.byref(a), None) == 1
    assert lib.acl_fleet_episode_batch(ct.byref(F), None, None) == 1


def _cpu_table(n):
    from aclswarm_amd import engine
    return engine.FormationTable.from_host([np.zeros((n, 3))], [C.chord_ring(n)], None,
                                           device="cpu")


def test_fleet_episode_rejections_without_gpu():
    """engine.FleetEpisode raises ValueError before anything runs, one case
    per rule (CPU tensors: the last rule, a CUDA device, rejects what passes
    the others)."""
    import torch
    import aclswarm_amd
    from aclswarm_amd import _lib as L
    from aclswarm_amd import engine
    assert aclswarm_amd.FleetEpisode is engine.FleetEpisode
    n, B = 13, 2
    T = _cpu_table(n)
    fidx = torch.zeros(B, dtype=torch.int32)
    q = torch.zeros((B, n, 3), dtype=torch.float64)
    Pt = torch.arange(n, dtype=torch.int16).repeat(B, n, 1)
    lat = L.default_episode_params()
    lat.auction_latency = -1
    cen = L.default_episode_params()
    cen.assignment = 1
    bad = [
        (dict(q=q.numpy()), "q must be"),                                    # type
        (dict(q=q[0]), "q must be"),                                         # shape
        (dict(q=q[:0]), "empty"),
        (dict(q=q.to(torch.float32)), "q must be a contiguous"),             # dtype
        (dict(vel=q[:, :, :2].contiguous()), "vel must be a contiguous"),    # shape
        (dict(vel=q.transpose(0, 1).contiguous().transpose(0, 1)), "vel"),   # strides
        (dict(vel=None), "vel must be a torch tensor"),
        (dict(fidx=fidx.to(torch.int64)), "fidx"),                           # dtype
        (dict(fidx=fidx[:1]), "fidx"),                                       # shape
        (dict(fidx=torch.zeros(B, dtype=torch.int32, device="meta")), "fidx"),  # devices
        (dict(Pt=Pt.to(torch.int32)), "Pt"),                                 # dtype
        (dict(Pt=Pt[:, :, :-1].contiguous()), "Pt"),                         # shape
        (dict(Pt=Pt.transpose(1, 2)), "Pt"),                                 # contiguity
        (dict(queue_cap=0), "queue_cap"),
        (dict(max_iter=-1), "max_iter"),
        (dict(ticks_per_step=0), "ticks_per_step"),
        (dict(params=lat), "auction_latency"),
        (dict(params=cen), "assignment"),
        (dict(), "CUDA device"),                                             # not on a GPU
    ]
    for kw, msg in bad:
        args = dict(dict(fidx=fidx, q=q, vel=q), **kw)
        with pytest.raises(ValueError, match=msg):
            engine.FleetEpisode(T, args.pop("fidx"), args.pop("q"), args.pop("vel"), **args)
    with pytest.raises(ValueError, match="out of range"):                    # n > 128
        engine.FleetEpisode(_cpu_table(129), fidx, torch.zeros((B, 129, 3), dtype=torch.float64),
                            torch.zeros((B, 129, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="formation table is on"):           # the table's device
        engine.FleetEpisode(T, fidx.to("meta"), q.to("meta"), q.to("meta"))
