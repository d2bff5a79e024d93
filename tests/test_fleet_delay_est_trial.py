"""The trials on own estimates with tables on real links and the encounter
record (acl_fleet_delay_est_trial_batch) on the restatement
tests/fleet_delay_est_trial_oracle.py, without a GPU: the reductions (b) and
(c) of the header, consequence (a) on ring13_two -- what is delivered in the
rounds after a commit -- the conditions of the crafted encounter case, the
record's edge cases, and the argument errors of the two C entries."""
import copy
import ctypes as ct

import numpy as np

import fleet_delay_est_trial_cases as DK
import fleet_delay_est_trial_oracle as DXT
import fleet_est_trial_cases as X
import pyoracle as O
from test_fleet_est_trial import OWN_PTRS, TRIAL_PTRS


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


SAME = ("u", "us", "ca", "on", "P", "raised", "est", "stamps", "loc_rows", "Pt", "q", "vel",
        "ctl_on")


def _same(ra, rb, what):
    for k in SAME:
        a, b = np.asarray(ra[k]), np.asarray(rb[k])
        if a.dtype.kind == "f":
            a, b = _bits(a), _bits(b)
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: {k}")
    assert (ra["status"], ra["loc"], ra["err2"], ra["committed"]) == \
        (rb["status"], rb["loc"], rb["err2"], rb["committed"]), what


def test_reduction_b_latency_zero_is_the_est_trial_step_for_step():
    """ring13_two with every link at 0 and no outage, max_tlat 2: the records
    of fleet_est_trial_oracle bit for bit, and nothing missed."""
    cs, ft0, recs0 = X.cpu_run("ring13_two")
    dc = DK.DelayEstTrialCase(cs, 0, 2)
    ft, recs = DK.fly(dc, dc.oracle())
    assert len(recs) == len(recs0) == 26
    for ra, rb in zip(recs, recs0):
        _same(ra, rb, f"step {ra['step']}")
    assert ft.xst == ft0.xst and not any(ft.trackers.n_missed)
    assert X.adoption_steps(recs) == X.adoption_steps(recs0)


def test_reduction_c_a_then_b_equals_a_plus_b_across_a_commit():
    """ring13_two at latency 2: 26 steps flown at once equal 13 + 13 with the
    whole state copied at the boundary -- the step before the forced commit of
    step 14, whose rounds deliver tables published before the boundary."""
    cs, ft, recs = DK.cpu_run("ring13_two_lat2")
    a = cs.oracle()
    DK.fly(cs, a, 13)
    assert a.trackers.log and max(P for P, _ in a.trackers.log.values()) == 6
    b = copy.deepcopy(a)
    del a
    more = []
    for s in range(13, 26):
        if s in cs.force:
            cs.force[s](b)
        more.append(b.step())
        more[-1]["q"], more[-1]["vel"] = b.q.copy(), b.vel.copy()
    for ra, rb in zip(more, recs[13:]):
        _same(ra, rb, f"step {ra['step']}")
    assert b.enc.status == ft.enc.status and b.trackers.log_bytes() == ft.trackers.log_bytes()
    assert X.commit_steps(recs) == [3, DK.RING13_COMMIT_AT]


def _subscribers(tr, adj):
    """{(receiver, sender)} under adj and the trackers' rows of the moment."""
    keep = tr.adj
    tr.adj = np.asarray(adj)
    out = {(w, u) for w in range(tr.n) for u in tr.subscribed(w) if u != w}
    tr.adj = keep
    return out


def test_consequence_a_tables_published_before_a_commit_arrive_over_the_new_graph():
    """ring13_two, every link at 2 rounds, forced commit at step 14 (round 7).
    The rounds of steps 14 and 16 deliver tables published in rounds 5 and 6,
    under the first formation, to the subscribers of the DELIVERY round: the
    second formation's graph under the rows adopted at step 11. That set is
    not the first formation's under the same rows, and it is not the latency-0
    flight's: there no table published before the commit is delivered after it
    at all (the links of the delivery rounds are the same, since both flights
    adopted the same rows at step 11; what travels over them is not)."""
    cs = DK.case("ring13_two_lat2")
    commit_round = DK.RING13_COMMIT_AT // 2

    def flown(case):
        ft = case.oracle()
        ft.trackers.taken_trace = []
        old = new = None
        for s in range(18):
            if s in case.force:
                case.force[s](ft)
            if s == DK.RING13_COMMIT_AT:  # the rows of the delivery rounds
                old = _subscribers(ft.trackers, case.forms[0][1])
                rows = ft.loc_rows.copy()
            r = ft.step()
            if s in (14, 16):
                assert r["committed"] == (s == 14) and (ft.loc_rows == rows).all()
                new = _subscribers(ft.trackers, case.forms[1][1])
        return ft, old, new

    ft, old, new = flown(cs)
    late = [t for t in ft.trackers.taken_trace if t[0] in (commit_round, commit_round + 1)
            and t[1] != t[2]]
    assert late and all(P == r - 2 and P < commit_round for r, w, u, P in late)
    assert sorted({P for _, _, _, P in late}) == [5, 6]
    got = {(w, u) for _, w, u, _ in late}
    assert (ft.loc_rows != np.arange(13)).any()  # the rows of step 11, not the identity
    assert got == new and got != old
    f0, _, _ = flown(DK.DelayEstTrialCase(cs.cs, 0, 2))
    late0 = [t for t in f0.trackers.taken_trace if t[0] in (commit_round, commit_round + 1)
             and t[1] != t[2]]
    got0 = {(w, u) for r, w, u, P in late0 if P < commit_round}
    assert late0 and got0 == set() and got != got0
    assert {(w, u, P) for _, w, u, P in late}.isdisjoint({(w, u, P) for _, w, u, P in late0})
    print("delivered after the commit:", len(got), "links; old graph", len(old),
          "common", len(got & old), "; latency 0", len(got0), "common", len(got & got0))


def test_ring13_two_with_latency_differs_from_latency_zero_at_the_next_adoption():
    """By the step of the first adoption after the commit the tables differ
    from the latency-0 flight's in some byte."""
    cs, ft, recs = DK.cpu_run("ring13_two_lat2")
    _, _, recs0 = X.cpu_run("ring13_two")
    after = [s for s in X.adoption_steps(recs) if s > DK.RING13_COMMIT_AT]
    after0 = [s for s in X.adoption_steps(recs0) if s > DK.RING13_COMMIT_AT]
    s = min(after + after0)
    assert not np.array_equal(_bits(recs[s]["est"]), _bits(recs0[s]["est"]))
    print("first adoption after the commit: latency 2", after[:1], "latency 0", after0[:1])


def _conditions(name, pair):
    cs, ft, recs = DK.cpu_run(name)
    n, st = cs.n, ft.enc.status
    assert st["n_blind"] > 0 and st["n_ghost"] > 0 and st["n_breach"] > 0
    # a step whose minimum two pairs attain bit for bit: the tie rule decides
    r = recs[0]
    q = r["q0"]
    a = DXT._s2(q[pair[0][1]] - q[pair[0][0]])
    b = DXT._s2(q[pair[1][1]] - q[pair[1][0]])
    assert _bits(a) == _bits(b) == _bits(r["enc"]["sep2"]) == _bits(0.25)
    assert (r["enc"]["i"], r["enc"]["j"]) == min(pair) == (st["i"], st["j"])
    assert st["step"] == 0 or st["sep2_min"] < 0.25
    # a vehicle with on false whose blind pairs are not counted
    hidden = 0
    for r in recs:
        on = np.asarray(r["ctl_on"], bool)
        if on.all():
            continue
        full = DXT.encounter_record(r["q0"], r["est"], np.ones(n, bool), ft.s)
        assert (r["enc"]["blind"][~on] == 0).all() and (r["enc"]["ghost"][~on] == 0).all()
        hidden += int(full["blind"][~on].sum())
    assert hidden > 0
    assert ft.trackers.n_missed[DK.CRAFTED_DEAD] == len(recs) // 2
    assert int(ft.enc.blind.sum()) == st["n_blind"] and int(ft.enc.ghost.sum()) == st["n_ghost"]
    return cs, ft, recs


def test_the_crafted_case_meets_its_conditions_n13():
    cs, ft, recs = _conditions("crafted13", ((1, 12), (2, 3)))
    assert list(X.adoption_steps(recs)) == [11]
    # the vehicle whose feed is dead believes itself at the origin
    assert ft.enc.blind[DK.CRAFTED_DEAD] > 0 and ft.enc.ghost[DK.CRAFTED_DEAD] > 0
    assert (ft.enc.status["n_breach"], ft.enc.status["n_blind"], ft.enc.status["n_ghost"]) == \
        (48, 10, 7)


def test_the_crafted_case_meets_its_conditions_n65():
    """The first auction ends at max_iter 40: 10 vehicles adopt at step 13, 28
    at step 14, 26 at step 15 and one never does: steps with a strict subset of
    the controllers running."""
    cs, ft, recs = _conditions("crafted65", ((1, 64), (2, 3)))
    on = [int(r["ctl_on"].sum()) for r in recs]
    assert on[12:16] == [0, 10, 38, 64] and on[-1] == 64


def test_the_record_of_one_vehicle_two_vehicles_and_a_nan():
    s = O.default_safety()
    r = DXT.encounter_record(np.zeros((1, 3)), np.zeros((1, 1, 3)), [True], s)
    assert np.isposinf(r["sep2"]) and (r["i"], r["j"]) == (0xFFFF, 0xFFFF)
    assert (r["n_breach"], r["n_blind"], r["n_ghost"]) == (0, 0, 0)
    log = DXT.EncounterLog(1)
    log.add(0, r)
    assert log.status["step"] == -1 and np.isposinf(log.status["sep2_min"])
    # two vehicles 1 m apart in the plane (10 m in z: the record is planar)
    q = np.array([[0.0, 0.0, 0.0], [0.6, 0.8, 10.0]])
    est = np.array([[q[0], [9.0, 9.0, 0.0]], [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]])
    r = DXT.encounter_record(q, est, [True, True], s)
    assert r["sep2"] == 0.36 + 0.64 and (r["i"], r["j"], r["n_breach"]) == (0, 1, 1)
    assert r["blind"].tolist() == [1, 0] and r["ghost"].tolist() == [0, 0]
    # ... vehicle 0 is blind (its table shows vehicle 1 far away); vehicle 1
    # believes itself at the origin, where its table has vehicle 0 as well:
    # distance 0 is a candidate, so vehicle 0 is seen
    assert DXT.encounter_record(q, est, [True, False], s)["blind"].tolist() == [1, 0]
    est[1, 0] = [0.0, 0.0, 0.0]
    est[1, 1] = [0.0, 0.0, 0.0]
    q[1, :2] = (3.0, 4.0)
    r = DXT.encounter_record(q, est, [False, True], s)
    assert (r["n_blind"], r["ghost"].tolist(), r["n_breach"]) == (0, [0, 1], 0)
    # a NaN is never a minimum and never a breach; its candidate test is true
    q3 = np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [5.0, 0.0, 0.0]])
    r = DXT.encounter_record(q3, np.broadcast_to(q3, (3, 3, 3)), [True] * 3, s)
    assert (r["sep2"], r["i"], r["j"], r["n_breach"]) == (25.0, 0, 2, 0)
    assert (r["n_blind"], r["n_ghost"]) == (0, 0)


def test_abi_of_the_new_structs():
    from aclswarm_amd import _lib as L
    assert L.FLEET_ENCOUNTER_STATUS_DTYPE.itemsize == 32
    assert L.FLEET_ENCOUNTER_STEP_DTYPE.itemsize == 24
    base = ct.sizeof(L.FleetEstTrialArgs)
    y = L.FleetDelayEstTrialArgs
    assert y.est.offset == 0 and y.tlat.offset == base and ct.sizeof(y) == base + 80
    assert y.enc.offset == base + 48 and y.enc_hist.offset == base + 72
    assert L.lib().acl_abi_version() == 11
    assert "acl_fleet_delay_est_trial_batch" in L.EXPORTS


def test_argument_errors_of_the_c_entries_without_gpu():
    from aclswarm_amd import _lib as L
    lib = L.lib()
    F = L.Formations(13, 2, 8, 8, 8, 8, 5, None)
    log_bytes = lib.acl_fleet_delay_localize_workspace_bytes(13, 1, 2)

    def args():
        y = L.FleetDelayEstTrialArgs()
        x = y.est
        a = x.lossy.delay.base
        a.B, a.K, a.step0, a.steps = 1, 2, 0, 1
        a.ticks_per_step, a.max_iter, a.queue_cap = 10, 0, 52
        for k in TRIAL_PTRS:
            setattr(a, k, 8)  # never dereferenced: every call below fails its checks
        a.workspace_bytes = lib.acl_fleet_est_trial_workspace_bytes(13, 1, 52, 2)
        a.cntrl, a.safety, a.tp = L.default_gains(), L.default_safety(), L.default_trial_params()
        x.lossy.delay.lat, x.lossy.delay.max_lat = 8, 2
        x.lossy.link.loss = x.lossy.link.seed = x.lossy.link.n_lost = 8
        x.track_every, x.diag = 2, 1
        for k in OWN_PTRS:
            setattr(x, k, 8)
        y.tlat, y.max_tlat, y.feed_loss, y.loc_n_missed = 8, 2, 8, 8
        y.loc_workspace, y.loc_workspace_bytes = 8, log_bytes - 1
        y.enc = y.enc_blind = y.enc_ghost = y.enc_hist = 8
        return y

    calls = {b"acl_fleet_delay_est_trial_batch: ":
             lambda y: lib.acl_fleet_delay_est_trial_batch(ct.byref(F), ct.byref(y), None),
             b"acl_fleet_delay_est_trial_init: ":
             lambda y: lib.acl_fleet_delay_est_trial_init(ct.byref(y), F.n, None)}
    for name, call in calls.items():
        def fails(y, msg):
            assert call(y) == 1  # INVALID_ARG
            err = lib.acl_last_error()
            assert err.startswith(name) and msg in err, err

        # (everything else is in order)
        fails(args(),
              b"loc_workspace_bytes is too small (acl_fleet_delay_localize_workspace_bytes)")
        for bad in (-1, 8, 1 << 30):
            y = args()
            y.max_tlat = bad
            fails(y, b"max_tlat out of range [0, 7]")
        y = args()  # ... reported even when there is nothing to fly
        y.max_tlat, y.est.lossy.delay.base.B = 9, 0
        fails(y, b"max_tlat out of range [0, 7]")
        y = args()
        y.loc_n_missed = None
        fails(y, b"feed_loss is given and loc_n_missed is NULL")
        for k in ("enc_blind", "enc_ghost"):
            y = args()
            setattr(y, k, None)
            fails(y, b"enc is given and enc_blind or enc_ghost is NULL")
        y = args()
        y.tlat = None
        fails(y, b"tlat is NULL")
        y = args()
        y.loc_workspace = None
        fails(y, b"loc_workspace is NULL")
        y = args()
        y.loc_workspace_bytes = 0
        fails(y, b"loc_workspace_bytes is too small")
        # optional: feed_loss (with loc_n_missed), the whole encounter group, enc_hist
        for clear in (("feed_loss", "loc_n_missed"), ("enc", "enc_blind", "enc_ghost", "enc_hist"),
                      ("enc_hist",)):
            y = args()
            for k in clear:
                setattr(y, k, None)
            fails(y, b"loc_workspace_bytes is too small")
        # the own-estimate entry's checks on `est`, under the new entry's name
        y = args()
        y.est.track_every = 0
        fails(y, b"track_every < 1")
        y = args()
        y.est.loc_Pt = None
        fails(y, b"loc_stamp, loc_est, loc_round, loc_n_lost, loc_Pt or xst is NULL")
        y = args()
        y.loc_workspace_bytes = log_bytes
        y.est.lossy.delay.base.workspace_bytes -= 1
        fails(y, b"workspace_bytes is too small (acl_fleet_est_trial_workspace_bytes)")
        y = args()
        y.est.lossy.delay.max_lat = 65
        fails(y, b"max_lat out of range [1, 64]")
        y = args()
        y.est.lossy.delay.base.Pt = None
        fails(y, b"required pointer is NULL")
        # nothing to fly: no pointer is looked at
        y = L.FleetDelayEstTrialArgs()
        a = y.est.lossy.delay.base
        a.B, a.K, a.steps, a.ticks_per_step, a.queue_cap = 0, 1, 0, 1, 1
        a.tp = L.default_trial_params()
        y.est.lossy.delay.max_lat, y.est.track_every = 1, 1
        assert call(y) == 0
    null = ct.POINTER(L.FleetDelayEstTrialArgs)()
    assert lib.acl_fleet_delay_est_trial_batch(ct.byref(F), null, None) == 1
    assert b"null argument" in lib.acl_last_error()
    assert lib.acl_fleet_delay_est_trial_init(null, 13, None) == 1
    assert b"null argument" in lib.acl_last_error()
