"""CPU suite of fleet localization on real links
(acl_fleet_delay_localize_batch, acl_fleet_delay_est_episode_batch): the
plain-Python restatement (tests/fleet_delay_localize_oracle.py) on the figures
tests/fleet_delay_localize_cases.py quotes, its reductions and invariants, and
the ABI's argument checks. None of it needs a GPU; the kernel is compared with
the same restatement in tests/test_gpu_fleet_delay_localize.py."""
import ctypes as ct

import numpy as np
import pytest

import fleet_auction_cases as C
import fleet_delay_localize_cases as DC
import fleet_delay_localize_oracle as DG
import fleet_localize_cases as GC
import fleet_localize_oracle as GO
import fleet_loss_oracle as LO


def _same(a, b):
    np.testing.assert_array_equal(a.stamps(), b.stamps())
    np.testing.assert_array_equal(a.est().view(np.uint64), b.est().view(np.uint64))
    assert a.round == b.round and list(a.n_lost) == list(b.n_lost)


@pytest.mark.parametrize("d", [0, 1, 2, 3])
def test_reduction_3_a_hop_costs_d_plus_one_rounds(d):
    """chord_ring(13), diameter 6: everybody known after 6 (d + 1) rounds, and
    max_age 6 (d + 1) - 1 from then on."""
    rounds, age = DC.KNOWN_AFTER_AT[d]
    assert (rounds, age) == (6 * (d + 1), 6 * (d + 1) - 1)
    traj = GC.trajectory(13, rounds + 4, d)
    tr = DG.DelayedTrackers(C.chord_ring(13), tlat=d)
    st = tr.run(rounds - 1, traj[:rounds - 1])
    print(d, st)
    assert st["n_unknown"] > 0
    st = tr.run(1, traj[rounds - 1:rounds])
    print(d, st)
    assert st == dict(rounds_run=1, n_unknown=0, max_age=age, flags=0)
    st = tr.run(4, traj[rounds:])
    assert st["n_unknown"] == 0 and st["max_age"] == age
    # a neighbour's entry is d rounds old, and holds what it sensed then
    ages = tr.round - tr.stamps()
    adj = C.chord_ring(13)
    assert (ages[adj != 0] == d).all() and (np.diag(ages) == 0).all()
    w, u = np.argwhere(adj != 0)[0]
    np.testing.assert_array_equal(tr.est()[w, u], traj[rounds + 3 - d, u])


def test_reduction_1_latency_zero_is_the_existing_model_under_loss():
    traj = GC.trajectory(13, 24, 2)
    a = GO.Trackers(C.chord_ring(13), loss=4096, seed=3)
    b = DG.DelayedTrackers(C.chord_ring(13), loss=4096, seed=3, tlat=0, max_tlat=3)
    assert a.run(24, traj) == b.run(24, traj)
    _same(a, b)
    assert sum(a.n_lost) > 0 and sum(b.n_missed) == 0


def _drawn(seed=0):
    return DG.DelayedTrackers(C.chord_ring(13), loss=4096, seed=5, tlat=DC.tlat_draw(13, 11, 3),
                              max_tlat=3, feed_loss=DC.feed_draw(13, 12))


def test_reduction_2_rounds_a_then_b_equals_a_plus_b():
    traj = GC.trajectory(13, 24, 4)
    a, b = _drawn(), _drawn()
    sa = a.run(24, traj)
    b.run(5, traj[:5])
    sb = b.run(19, traj[5:])
    _same(a, b)
    assert dict(sa, rounds_run=19) == sb and a.n_missed == b.n_missed
    assert sum(a.n_lost) > 0 and 0 < sum(a.n_missed) < 24 * 13
    assert set(DC.feed_draw(13, 12).tolist()) == set(DC.FEED_THRS)


def test_result_is_independent_of_the_visiting_order():
    traj = GC.trajectory(13, 12, 6)
    a, b = _drawn(), _drawn()
    rng = np.random.RandomState(0)
    b.order = lambda w, senders: [senders[k] for k in rng.permutation(len(senders))]
    assert a.run(12, traj) == b.run(12, traj)
    _same(a, b)
    assert a.n_missed == b.n_missed


def test_a_dead_feed_is_never_known_to_anybody():
    n, v, rounds = 13, 4, 30
    feed = np.zeros(n, np.int64)
    feed[v] = LO.DEAD
    tr = DG.DelayedTrackers(C.chord_ring(n), tlat=1, feed_loss=feed)
    st = tr.run(rounds, GC.trajectory(n, rounds, 8))
    assert st["n_unknown"] == n and (tr.stamps()[:, v] == 0).all()
    assert tr.n_missed == [rounds if w == v else 0 for w in range(n)]
    assert tr.stamps()[v, v] == 0 and not tr.est()[:, v].any()
    # it still hears, publishes and relays: everybody else is known to everybody
    assert (np.delete(tr.stamps(), v, axis=1) > 0).all()


def test_a_table_from_before_the_log_is_neither_delivered_nor_counted():
    """Three rounds of the existing model, then latency 2 on a fresh log with
    every link dead: the first two rounds have nothing to lose."""
    n = 13
    traj = GC.trajectory(n, 8, 9)
    tr = DG.DelayedTrackers(C.chord_ring(n), tlat=2, loss=0, seed=1)
    tr.delayed = False
    tr.run(3, traj[:3])
    tr.delayed = True
    assert tr.log == {}
    before = tr.stamps()
    tr.loss = LO.loss_matrix(n, LO.DEAD)
    tr.taken_trace = []
    tr.run(2, traj[3:5])
    assert sum(tr.n_lost) == 0 and tr.taken_trace == []
    after = tr.stamps()
    np.testing.assert_array_equal(after - np.diag(np.diag(after)), before - np.diag(np.diag(before)))
    tr.run(1, traj[5:6])
    assert sum(tr.n_lost) == int(C.chord_ring(n).sum())  # round 5 is due the tables of round 3
    tr.loss = LO.loss_matrix(n, 0)
    tr.run(1, traj[6:7])
    assert sorted(set(P for _, _, _, P in tr.taken_trace)) == [4]
    # from round 0 on a zero-filled log: P < 0 is no table either
    tr = DG.DelayedTrackers(C.chord_ring(n), tlat=2, loss=LO.DEAD, seed=1)
    tr.run(2, traj[:2])
    assert sum(tr.n_lost) == 0


def test_the_mixed_batch_is_what_the_gpu_tests_need():
    trs = DC.mixed_trackers()
    assert all(not tr.bad_tlat() for tr in trs)
    assert (trs[7].tlat == 7).all() and {int(tr.tlat.max()) for tr in trs[:7]} == {3}
    assert any((tr.feed_loss == LO.DEAD).any() for tr in trs) and not trs[0].feed_loss.any()
    big = DG.DelayedTrackers(C.chord_ring(13), tlat=DC.tlat_draw(13, 1, 3), max_tlat=2)
    assert big.bad_tlat()


def test_the_composed_episode_at_latency_zero_is_the_est_episode():
    """fleet_delay_est_episode_oracle with tlat 0 and no outage flies
    fleet_est_episode_oracle's ring13 (track_every 2, loss 4096) record for
    record; at every link = 2 the tables are older and the flight differs."""
    import fleet_delay_est_episode_oracle as DXO
    import fleet_est_episode_cases as X
    cs = X.case("ring13_loss4096")
    _, _, ref = X.cpu_run("ring13_loss4096")

    def oracle(tlat):
        c = cs.cs
        return DXO.DelayEstFleetEpisode(c.p, c.adj, c.gains, c.q0, c.vel0, c.ep, c.lat,
                                        loss=cs.loss, seed=cs.seed, Pt=c.Pt, max_iter=c.max_iter,
                                        ticks_per_step=c.T, track_every=cs.track_every, diag=True,
                                        tlat=tlat, max_tlat=2)
    steps = 10
    ep, recs = X.fly(cs, oracle(0), steps)
    for a, b in zip(ref, recs):
        for k in ("q", "vel", "u", "est", "stamps"):
            np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)
        assert a["err2"] == b["err2"] and a["loc"] == b["loc"]
    ep2, recs2 = X.fly(cs, oracle(2), steps)
    assert ep2.xst["n_unknown"] > ep.xst["n_unknown"] and ep2.xst["err2_nbr"] > ep.xst["err2_nbr"]
    assert not np.array_equal(recs2[-1]["q"], recs[-1]["q"])


# ---- the ABI without a GPU ----

def test_exports_and_struct_layouts():
    from aclswarm_amd import _lib as L
    lib = L.lib()
    for s in ("acl_fleet_delay_localize_workspace_bytes", "acl_fleet_delay_localize_batch",
              "acl_fleet_delay_est_episode_batch"):
        assert s in L.EXPORTS and hasattr(lib, s)
    A = L.FleetDelayLocalizeArgs
    base = ct.sizeof(L.FleetLocalizeArgs)
    assert (A.base.offset, A.tlat.offset, A.max_tlat.offset, A.feed_loss.offset,
            A.n_missed.offset, A.workspace.offset, A.workspace_bytes.offset, ct.sizeof(A)) == \
        (0, base, base + 8, base + 16, base + 24, base + 32, base + 40, base + 48)
    E = L.FleetDelayEstEpisodeArgs
    base = ct.sizeof(L.FleetEstEpisodeArgs)
    assert (E.est.offset, E.tlat.offset, E.max_tlat.offset, E.feed_loss.offset,
            E.loc_n_missed.offset, E.loc_workspace.offset, E.loc_workspace_bytes.offset,
            ct.sizeof(E)) == \
        (0, base, base + 8, base + 16, base + 24, base + 32, base + 40, base + 48)
    assert lib.acl_abi_version() == 11


def test_workspace_bytes():
    from aclswarm_amd import _lib as L
    ws = L.lib().acl_fleet_delay_localize_workspace_bytes
    for n, B, m in ((1, 2, 3), (13, 8, 7), (64, 4, 2), (65, 4, 0), (128, 4, 7)):
        per = 32 + 28 * (m + 1) * n * n
        assert ws(n, B, m) == B * ((per + 7) // 8 * 8)
        tr = DG.DelayedTrackers(np.zeros((n, n), np.uint8), max_tlat=m) if n <= 13 else None
        assert tr is None or len(tr.log_bytes()) * B == ws(n, B, m)
    for bad in ((0, 1, 0), (129, 1, 0), (13, 0, 0), (13, 1, -1), (13, 1, 8)):
        assert ws(*bad) == 0


def test_delay_localize_argument_errors_without_gpu():
    from aclswarm_amd import _lib as L
    lib = L.lib()
    call = lib.acl_fleet_delay_localize_batch
    name = b"acl_fleet_delay_localize_batch: "
    F = L.Formations(129, 1, None, 8, None, None)
    d = L.FleetDelayLocalizeArgs()
    a = d.base

    def fails(msg):
        assert call(ct.byref(F), ct.byref(d), None) == 1  # INVALID_ARG
        err = lib.acl_last_error()
        assert err.startswith(name) and msg in err, err

    a.B, a.rounds, a.q_rounds = 1, 4, 4
    fails(b"n out of range [1, 128]")
    F.n = 0
    fails(b"n out of range [1, 128]")
    F.n = 13
    fails(b"required pointer is NULL")
    a.rounds = -1
    fails(b"rounds < 0")
    a.rounds = 4
    a.B = -1
    fails(b"B < 0")
    a.B = 1
    for bad in (0, 2, 3, 5):
        a.q_rounds = bad
        fails(b"q_rounds must be 1 or rounds")
    a.q_rounds = 1
    for bad in (-1, 8, 64):
        d.max_tlat = bad
        fails(b"max_tlat out of range [0, 7]")
    d.max_tlat = 3
    keys = ("fidx", "Pt", "stamp", "est", "round", "status")
    for k in keys:
        setattr(a, k, 8)  # never dereferenced: the calls below fail their checks
    for k in keys:
        setattr(a, k, None)
        fails(b"required pointer is NULL")
        setattr(a, k, 8)
    fails(b"rounds > 0 and q is NULL")
    a.q = 8
    fails(b"tlat is NULL")
    d.tlat = 8
    fails(b"workspace is NULL")
    d.workspace = 8
    need = lib.acl_fleet_delay_localize_workspace_bytes(13, 1, 3)
    for short in (0, need - 1):
        d.workspace_bytes = short
        fails(b"workspace_bytes is too small")
    d.workspace_bytes = need
    a.loss = 8
    fails(b"loss is given and seed is NULL")
    a.seed = 8
    fails(b"loss is given and n_lost is NULL")
    a.loss = None
    fails(b"seed is given and loss and feed_loss are NULL")
    a.seed = None
    d.feed_loss = 8
    fails(b"feed_loss is given and seed is NULL")
    a.seed = 8
    fails(b"feed_loss is given and n_missed is NULL")
    d.feed_loss, a.seed = None, None
    F.adj = None
    fails(b"required pointer is NULL")
    F.adj = 8
    F.n_formations = 0
    fails(b"formation table is empty")
    F.n_formations = 1
    a.B = 0
    a.fidx = None
    assert call(ct.byref(F), ct.byref(d), None) == 0  # empty batch
    assert call(None, ct.byref(d), None) == 1 and call(ct.byref(F), None, None) == 1
    assert lib.acl_last_error() == name + b"null argument"


def test_delay_est_episode_argument_errors_without_gpu():
    """The checks the new entry adds, reached behind those of
    acl_fleet_est_episode_batch on `est` (tests/test_fleet_est_episode.py walks
    those): every required pointer is a never-dereferenced 8."""
    from aclswarm_amd import _lib as L
    lib = L.lib()
    call = lib.acl_fleet_delay_est_episode_batch
    name = b"acl_fleet_delay_est_episode_batch: "
    F = L.Formations(13, 1, None, 8, None, None)
    y = L.FleetDelayEstEpisodeArgs()
    x = y.est
    a = x.lossy.delay.base

    def fails(msg):
        assert call(ct.byref(F), ct.byref(y), None) == 1
        err = lib.acl_last_error()
        assert err.startswith(name) and msg in err, err

    assert call(ct.byref(F), None, None) == 1
    assert lib.acl_last_error() == name + b"null argument"
    a.B, a.steps, a.ticks_per_step, a.queue_cap = 1, 2, 10, 16
    lib.acl_default_episode_params(ct.byref(a.ep))
    x.lossy.delay.max_lat = 1
    x.track_every = 0
    fails(b"track_every < 1")
    x.track_every = 2
    for bad in (-1, 8):
        y.max_tlat = bad
        fails(b"max_tlat out of range [0, 7]")
    y.max_tlat = 2
    y.feed_loss = 8
    fails(b"feed_loss is given and loc_n_missed is NULL")
    y.loc_n_missed = 8
    fails(b"required pointer is NULL")
    for k, _ in L.FleetEpisodeArgs._fields_:
        if k in ("fidx", "q", "vel", "P", "Pt", "open", "invalid", "just_received", "biditer",
                 "price", "who", "Rt", "final_price", "final_who", "done_tick", "vflags",
                 "n_thrown", "n_tally", "queue_len", "status", "adopt_step", "est", "ring_u",
                 "ring_ca", "fst", "workspace"):
            setattr(a, k, 8)
    x.lossy.delay.lat = 8
    x.lossy.link.loss, x.lossy.link.seed, x.lossy.link.n_lost = 8, 8, 8
    for k in ("loc_stamp", "loc_est", "loc_round", "loc_n_lost", "xst"):
        setattr(x, k, 8)
    fails(b"tlat is NULL")
    y.tlat = 8
    fails(b"loc_workspace is NULL")
    y.loc_workspace = 8
    y.loc_workspace_bytes = lib.acl_fleet_delay_localize_workspace_bytes(13, 1, 2) - 1
    fails(b"loc_workspace_bytes is too small")
    a.steps = 0
    assert call(ct.byref(F), ct.byref(y), None) == 0  # nothing to fly
