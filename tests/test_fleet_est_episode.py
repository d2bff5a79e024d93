"""CPU tests of the episodes on each vehicle's own estimates
(acl_fleet_est_episode_batch): the restatement
tests/fleet_est_episode_oracle.py against the shared-snapshot restatement
tests/fleet_loss_episode_oracle.py (the two reductions), what stale estimates
do to a flight, gossip under loss, the error record, the input condition of
the GPU tests' cases (tests/fleet_est_episode_cases.py), and the ABI without a
GPU."""
import copy
import ctypes as ct

import numpy as np
import pytest

import fleet_auction_cases as C
import fleet_est_episode_cases as X
import fleet_est_episode_oracle as XO
import fleet_localize_oracle as GO

TOL = 1e-5  # the GPU tests' tolerance of a command


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_records(recs, srecs, commands_but=()):
    for r, sr in zip(recs, srecs):
        what = f"step {r['step']}"
        for k in ("q", "vel") if r["step"] in commands_but else ("u", "us", "q", "vel"):
            np.testing.assert_array_equal(_bits(r[k]), _bits(sr[k]), err_msg=f"{what}: {k}")
        for k in ("ca", "raised", "P"):
            np.testing.assert_array_equal(r[k], sr[k], err_msg=f"{what}: {k}")
        assert r["status"] == sr["status"] and r["per_vehicle"] == sr["per_vehicle"], what
        assert (r["cmd"] is None) == (sr["cmd"] is None), what
        if r["cmd"] is not None:
            np.testing.assert_array_equal(r["cmd"], sr["cmd"], err_msg=what)


def _same_fleet(ep, sh):
    a, b = C.snapshot_state(ep.fleet), C.snapshot_state(sh.fleet)
    for k in a:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)
    assert ep.fst == sh.fst and ep.n_ca_steps == sh.n_ca_steps
    assert (ep.converged_step, ep.gridlock_step) == (sh.converged_step, sh.gridlock_step)
    np.testing.assert_array_equal(ep.adopt_step, sh.adopt_step)


@pytest.mark.parametrize("name,adopt,ca", [("ring13_complete", {}, 30),
                                           ("ring6_complete", {5: 6, 11: 6}, 14)])
def test_complete_graph_is_the_shared_snapshot_episode(name, adopt, ca):
    """After one lossless round on a complete graph every table is q bit for
    bit: with track_every = 1 the flight equals LossyFleetEpisode's record for
    record (q, rows, final prices, CA steps), and the error record is 0."""
    cs, ep, recs = X.cpu_run(name)
    sh, srecs = X.cpu_shared(name)
    _same_records(recs, srecs)
    _same_fleet(ep, sh)
    assert X.adoption_steps(recs) == adopt and ep.n_ca_steps == ca
    for r in recs:
        assert r["err2"] == (0.0, 0.0, 0.0)
        np.testing.assert_array_equal(_bits(r["est"]), _bits(np.broadcast_to(r["q0"], r["est"].shape)))
    x = ep.xst
    assert (x["rounds_run"], x["n_unknown"], x["max_age"]) == (cs.steps, 0, 0)
    assert (x["err2_own"], x["err2_nbr"], x["err2_all"]) == (0.0, 0.0, 0.0)


def test_own_ring_at_track_every_1_equals_the_shared_snapshot_flight():
    """ring13 on its own ring, a round every step: the alignment and DistCntrl
    read the closed neighbourhood only, which is one hop = one round old = the
    truth, and no collision decision involves a non-neighbour. Adoptions at
    steps 7 and 19, 41 CA vehicle-steps, q and vel bit for bit at every step;
    the tables of non-neighbours are up to 9.7 mm off. The commands are equal
    bit for bit too, except at the two adoption steps: a vehicle flies its new
    row before a round under the new subscriptions has run, so its new
    neighbours are several hops old (u differs by up to 3.1e-3; the
    acceleration limit of makeSafeTraj gives the same q)."""
    cs, ep, recs = X.cpu_run("ring13_te1")
    sh, srecs = X.cpu_shared("ring13_te1")
    _same_records(recs, srecs, commands_but=(7, 19))
    for s in (7, 19):
        du = np.abs(recs[s]["u"] - srecs[s]["u"]).max()
        assert 5e-4 < du < 4e-3
    _same_fleet(ep, sh)
    assert X.adoption_steps(recs) == {7: 13, 19: 13} and ep.n_ca_steps == 41
    assert all(r["err2"][0] == 0.0 for r in recs)  # its own entry: sensed this step
    worst = max(max(r["err2"]) for r in recs)
    assert 9.6e-3 < np.sqrt(worst) < 9.8e-3
    assert ep.xst["err2_all"] == worst and ep.xst["rounds_run"] == 30


def test_stale_estimates_at_track_every_2():
    """A round every other step: the same adoption steps, but on odd steps
    every vehicle steers on positions one control period old, so u differs
    from the shared-snapshot u by more than the GPU tests' tolerance, q drifts
    apart (1.1e-4 m) and the final prices differ."""
    cs, ep, recs = X.cpu_run("ring13_te2")
    sh, srecs = X.cpu_shared("ring13_te2")
    assert X.adoption_steps(recs) == X.adoption_steps(srecs) == {7: 13, 19: 13}
    # step 1: the first step flown on tables one period old, from (still) equal q
    np.testing.assert_array_equal(_bits(recs[1]["q0"]), _bits(srecs[1]["q0"]))
    rel = np.abs(recs[1]["u"] - srecs[1]["u"]) / np.maximum(np.abs(srecs[1]["u"]), 1.0)
    assert rel.max() > TOL
    np.testing.assert_array_equal(_bits(recs[0]["u"]), _bits(srecs[0]["u"]))
    for r in recs:
        assert (r["err2"][0] == 0.0) == (r["step"] % 2 == 0)
    dq = np.abs(ep.q - sh.q).max()
    assert 1.0e-4 < dq < 1.2e-4
    assert not np.array_equal(ep.fleet.final_price, sh.fleet.final_price)
    assert 18.6e-3 < np.sqrt(max(max(r["err2"]) for r in recs)) < 18.8e-3
    assert ep.xst["rounds_run"] == 15


def test_rings12_never_hears_of_the_other_component():
    """Two disjoint rings of 6: each vehicle's table lacks the 6 vehicles of
    the other ring for the whole flight (12 x 6 = 72 entries at the origin),
    so collision avoidance sees phantoms there and the CA count differs from
    the shared-snapshot episode's (74 against 78)."""
    cs, ep, recs = X.cpu_run("rings12_te2")
    sh, srecs = X.cpu_shared("rings12_te2")
    unknown = [r["loc"]["n_unknown"] for r in recs if r["loc"]]
    assert unknown[:3] == [108, 84, 72] and set(unknown[2:]) == {72}
    assert ep.xst["n_unknown"] == 72 and not X.adoption_steps(recs)
    assert (ep.n_ca_steps, sh.n_ca_steps) == (74, 78)
    st = recs[-1]["stamps"]
    assert not st[:6, 6:].any() and not st[6:, :6].any() and st[:6, :6].all() and st[6:, 6:].all()


def test_ring65_and_odd_last128_figures():
    cs, ep, recs = X.cpu_run("ring65_te2")
    assert len(recs) == 12 and ep.xst["n_unknown"] == 3236 and ep.xst["rounds_run"] == 6
    cs, ep, recs = X.cpu_run("odd_last128_te2")
    assert len(recs) == 4 and ep.xst["rounds_run"] == 2 and all(r["per_vehicle"] for r in recs)


def test_gossip_under_loss_is_independent_of_the_bids():
    """ring13 under loss 4096: tables and bids are lost under the same matrix
    and seed, but a table's fate is that of (seed, w, u, round, 0xFFFFFFFF):
    the trackers lose what stand-alone trackers lose on the same snapshots,
    whatever the auction did. 30 tables and 15 bids lost. a + b steps equal
    the whole flight."""
    cs, ep, recs = X.cpu_run("ring13_loss4096")
    assert sum(ep.trackers.n_lost) == 30 and int(ep.fleet.n_lost.sum()) == 15
    assert not X.adoption_steps(recs)
    alone = GO.Trackers(cs.adj, Pt=cs.Pt, loss=cs.loss, seed=cs.seed)
    for r in recs:
        if r["step"] % cs.track_every == 0:
            alone.run(1, r["q0"])
    assert alone.n_lost == ep.trackers.n_lost
    np.testing.assert_array_equal(alone.stamps(), ep.trackers.stamps())
    np.testing.assert_array_equal(_bits(alone.est()), _bits(ep.trackers.est()))
    # the bids' counter is the fleet's own
    assert ep.trackers.n_lost != ep.fleet.n_lost.tolist()
    # a then b
    half = cs.oracle()
    X.fly(cs, half, steps=11)
    rest = copy.deepcopy(half)
    for s in range(11, cs.steps):
        rest.step()
    np.testing.assert_array_equal(_bits(rest.q), _bits(ep.q))
    assert rest.trackers.n_lost == ep.trackers.n_lost and rest.xst == ep.xst
    assert rest.trackers.round == ep.trackers.round == 15


def test_error_record_at_n_1_and_its_rules():
    cs, ep, recs = X.cpu_run("single")
    assert all(r["err2"] == (0.0, 0.0, 0.0) for r in recs) and ep.xst["rounds_run"] == 6
    # one vehicle, a table that is wrong about itself: own only
    q = np.array([[1.0, 2.0, 3.0]])
    est = np.array([[[1.5, 2.0, 1.0]]])
    assert XO.err2_record(est, [[1]], q, [[0]], [[0]]) == (0.25 + 4.0, 0.0, 0.0)
    assert XO.err2_record(est, [[1]], q, [[0]], [[1]]) == (4.25, 4.25, 0.0)  # a diagonal edge
    # three vehicles on a path 0 - 1 - 2 under the identity: vehicle 0 reads 1
    # (a neighbour, never heard of) and has heard of 2 (no neighbour); a NaN
    # never enters a maximum
    adj = np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]])
    q = np.array([[0.0, 0, 0], [3.0, 0, 0], [0, 4.0, 0]])
    est = np.broadcast_to(q, (3, 3, 3)).copy()
    est[0, 1] = 0.0          # unknown: the origin, 3 m off
    est[0, 2] = [0, 4.0, 2.0]
    est[1, 0] = np.nan
    stamps = np.ones((3, 3), np.int32)
    stamps[0, 1] = 0
    own, nbr, every = XO.err2_record(est, stamps, q, np.tile(np.arange(3), (3, 1)), adj)
    assert (own, nbr, every) == (0.0, 9.0, 4.0)


def test_input_condition_of_the_gpu_cases():
    """Every step and every vehicle with a close vehicle, on the step's own
    table and saturated command: d_margin >= 1e-6, edge and quarter margins >=
    1e-4 (no GPU comparison leaves a step or a vehicle out)."""
    seen = {}
    for name in X.GPU_CASES:
        cs, ep, recs = X.cpu_run(name)
        d, e, q = seen[name] = X.condition(recs)
        assert d >= X.D_MARGIN and e >= X.ANGLE_MARGIN and q >= X.ANGLE_MARGIN, (name, d, e, q)
    for name in ("single", "ring65_te2", "odd_last128_te2"):
        assert seen[name] == (np.inf,) * 3  # no close vehicle at all
    ring = [seen[k] for k in seen if k.startswith("ring13")]
    assert 0.46 < min(m[0] for m in ring) < 0.47
    assert 0.068 < min(m[1] for m in ring) < 0.070
    assert 0.087 < min(m[2] for m in ring) < 0.089
    d, e, q = seen["rings12_te2"]
    assert 0.29 < d < 0.31 and 0.49 < e < 0.51 and 0.058 < q < 0.060


# ---- the ABI without a GPU ----

def test_exports_and_struct_layout():
    from aclswarm_amd import _lib as L
    lib = L.lib()
    for fn in ("acl_fleet_est_episode_workspace_bytes", "acl_fleet_est_episode_batch"):
        assert fn in L.EXPORTS and hasattr(lib, fn)
    A = L.FleetEstEpisodeArgs
    base = ct.sizeof(L.FleetLossyEpisodeArgs)
    assert ct.sizeof(A) == base + 8 + 6 * 8
    assert (A.track_every.offset, A.diag.offset, A.loc_stamp.offset, A.err2_hist.offset) == \
        (base, base + 4, base + 8, base + 48)
    assert L.FLEET_EST_EPISODE_STATUS_DTYPE.itemsize == ct.sizeof(L.FleetEstEpisodeStatus) == 40
    assert L.FLEET_EST_EPISODE_STATUS_DTYPE.fields["err2_own"][1] == \
        L.FleetEstEpisodeStatus.err2_own.offset == 16
    assert lib.acl_abi_version() == 11
    # the layout of the entries with latency, two 16-byte status arrays appended
    for n, B, cap, ml in ((13, 3, 52, 5), (128, 8, 512, 1), (1, 1, 4, 64)):
        d = lib.acl_fleet_delay_episode_workspace_bytes(n, B, cap, ml)
        x = lib.acl_fleet_est_episode_workspace_bytes(n, B, cap, ml)
        assert d < x <= d + 2 * (16 * B + 256)
    for bad in ((0, 1, 4, 1), (129, 1, 4, 1), (13, 0, 4, 1), (13, 1, 0, 1), (13, 1, 4, 0),
                (13, 1, 4, 65)):
        assert lib.acl_fleet_est_episode_workspace_bytes(*bad) == 0


def test_argument_errors_of_the_c_entry_without_gpu():
    from aclswarm_amd import _lib as L
    lib = L.lib()
    call = lib.acl_fleet_est_episode_batch
    name = b"acl_fleet_est_episode_batch: "
    F = L.Formations(13, 1, 8, 8, 8, 8, 5, None)
    need = ("fidx", "q", "vel", "P", "adopt_step", "est", "ring_u", "ring_ca", "fst", "status",
            "workspace") + ("Pt", "open", "invalid", "just_received", "biditer", "price", "who",
                            "Rt", "final_price", "final_who", "done_tick", "vflags", "n_thrown",
                            "n_tally", "queue_len")
    own = ("loc_stamp", "loc_est", "loc_round", "loc_n_lost", "xst")

    def args():
        x = L.FleetEstEpisodeArgs()
        a = x.lossy.delay.base
        a.B, a.step0, a.steps, a.ticks_per_step, a.max_iter, a.queue_cap = 1, 0, 1, 10, 0, 52
        for k in need:
            setattr(a, k, 8)  # never dereferenced: every call below fails its checks
        a.workspace_bytes = lib.acl_fleet_est_episode_workspace_bytes(13, 1, 52, 2) - 1
        a.cntrl, a.safety, a.ep = L.default_gains(), L.default_safety(), L.default_episode_params()
        x.lossy.delay.lat, x.lossy.delay.max_lat = 8, 2
        x.lossy.link.loss = x.lossy.link.seed = x.lossy.link.n_lost = 8
        x.track_every, x.diag = 2, 1
        for k in own:
            setattr(x, k, 8)
        return x

    def fails(x, msg, F=F):
        assert call(ct.byref(F), ct.byref(x), None) == 1  # INVALID_ARG
        err = lib.acl_last_error()
        assert err.startswith(name) and msg in err, err

    # the workspace of the new size is asked for, by name; one of the entries
    # with latency alone is too small
    fails(args(), b"workspace_bytes is too small (acl_fleet_est_episode_workspace_bytes)")
    x = args()
    x.lossy.delay.base.workspace_bytes = lib.acl_fleet_delay_episode_workspace_bytes(13, 1, 52, 2)
    fails(x, b"acl_fleet_est_episode_workspace_bytes")
    for bad in (0, -3):
        x = args()
        x.track_every = bad
        fails(x, b"track_every < 1")
    x = args()  # ... reported even when there is nothing to fly
    x.track_every, x.lossy.delay.base.steps = 0, 0
    fails(x, b"track_every < 1")
    for k in own:
        x = args()
        setattr(x, k, None)
        fails(x, b"loc_stamp, loc_est, loc_round, loc_n_lost or xst is NULL")
    x = args()  # err2_hist may be NULL
    x.err2_hist = None
    fails(x, b"workspace_bytes")
    # the lossy episode entry's checks on `lossy`
    for k, msg in (("loss", b"loss is NULL"), ("seed", b"seed is NULL"),
                   ("n_lost", b"n_lost is NULL")):
        x = args()
        setattr(x.lossy.link, k, None)
        fails(x, msg)
    x = args()
    x.lossy.delay.lat = None
    fails(x, b"lat is NULL")
    for bad in (0, 65):
        x = args()
        x.lossy.delay.max_lat = bad
        fails(x, b"max_lat out of range [1, 64]")
    x = args()
    x.lossy.delay.base.ticks_per_step = 0
    fails(x, b"ticks_per_step < 1")
    x = args()
    x.lossy.delay.base.adopt_step = None
    fails(x, b"required pointer is NULL")
    x = args()
    x.lossy.delay.base.ep.auction_latency = 3
    fails(x, b"auction_latency")
    for n in (0, 129):
        fails(args(), b"n out of range [1, 128]", L.Formations(n, 1, 8, 8, 8, 8, 5, None))
    # nothing to do: no pointer is looked at
    for k, v in (("B", 0), ("steps", 0)):
        x = L.FleetEstEpisodeArgs()
        a = x.lossy.delay.base
        a.B, a.steps, a.ticks_per_step, a.queue_cap = 1, 1, 10, 52
        setattr(a, k, v)
        a.ep = L.default_episode_params()
        x.lossy.delay.max_lat, x.track_every = 1, 1
        assert call(ct.byref(F), ct.byref(x), None) == 0
    assert call(None, ct.byref(args()), None) == 1 and call(ct.byref(F), None, None) == 1
    assert lib.acl_last_error() == name + b"null argument"
