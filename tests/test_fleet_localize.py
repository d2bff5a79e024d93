"""CPU suite of fleet localization (acl_fleet_localize_batch) and of the fleet
auction started from own estimates (acl_fleet_est_auction_batch): the
plain-Python restatements (tests/fleet_localize_oracle.py,
tests/fleet_est_oracle.py) on the figures tests/fleet_localize_cases.py quotes,
their invariants (visiting order, chunked runs, bad rows, rewired rows), loss,
the three own-estimate cases the GPU tests rely on, and the ABI's argument
checks. None of it needs a GPU; the kernels are compared with the same
restatements in tests/test_gpu_fleet_localize.py and tests/test_gpu_fleet_est.py."""
import ctypes as ct

import numpy as np
import pytest

import fleet_auction_cases as C
import fleet_auction_oracle as FO
import fleet_delay_cases as DC
import fleet_est_oracle as EO
import fleet_localize_cases as GC
import fleet_localize_oracle as GO
import fleet_loss_cases as LC
import fleet_loss_oracle as LO


def _same(a, b):
    np.testing.assert_array_equal(a.stamps(), b.stamps())
    np.testing.assert_array_equal(a.est().view(np.uint64), b.est().view(np.uint64))
    assert a.round == b.round and a.n_lost == b.n_lost


# ---- lossless runs on identity rows ----

@pytest.mark.parametrize("n", [13, 64, 65, 128])
def test_chord_ring_knows_everybody_after_its_diameter(n):
    rounds, age = GC.KNOWN_AFTER[n]
    q = C.snapshot(np.random.RandomState(n), n)
    tr = GO.Trackers(C.chord_ring(n))
    st = tr.run(rounds - 1, q)
    print(n, st)
    assert st["n_unknown"] > 0
    st = tr.run(1, q)
    print(n, st)
    assert st == dict(rounds_run=1, n_unknown=0, max_age=age, flags=0)
    np.testing.assert_array_equal(tr.est(), np.broadcast_to(q, (n, n, 3)))
    # a vehicle k hops away is k - 1 rounds old: the own entry and the neighbours' are fresh
    ages = tr.round - tr.stamps()
    adj = C.chord_ring(n)
    assert (ages[adj != 0] == 0).all() and (np.diag(ages) == 0).all()


def test_two_rings_never_hear_of_each_other():
    n = 12
    q = C.snapshot(np.random.RandomState(5), n)
    tr = GO.Trackers(C.two_rings(6))
    for rounds in (3, 40):
        st = tr.run(rounds, q)
        assert st["n_unknown"] == 72 and st["flags"] == 0
    s, e = tr.stamps(), tr.est()
    assert (s[:6, 6:] == 0).all() and (s[6:, :6] == 0).all() and (s[:6, :6] > 0).all()
    assert not e[:6, 6:].any() and not e[6:, :6].any()
    assert st["max_age"] == 2  # a ring of 6: three hops


# ---- invariants ----

def test_result_is_independent_of_the_visiting_order():
    sc = C.random_rows(13)
    traj = GC.trajectory(13, 9, 1)
    a = GO.Trackers(sc.adj, Pt=sc.Pt, loss=GC.LOSS_THR, seed=3)
    b = GO.Trackers(sc.adj, Pt=sc.Pt, loss=GC.LOSS_THR, seed=3)
    rng = np.random.RandomState(0)
    b.order = lambda w, senders: [senders[k] for k in rng.permutation(len(senders))]
    assert a.run(9, traj) == b.run(9, traj)
    _same(a, b)
    assert sum(a.n_lost) > 0


def test_rounds_a_then_b_equals_a_plus_b_under_loss():
    traj = GC.trajectory(13, 24, 2)
    a, b = GC.ring_loss(1), GC.ring_loss(1)
    sa = a.run(24, traj)
    b.run(5, traj[:5])
    sb = b.run(19, traj[5:])
    _same(a, b)
    assert dict(sa, rounds_run=19) == sb and sum(a.n_lost) == GC.LOSS_TOTALS[1]


def test_a_bad_row_receives_nothing_but_is_heard():
    n, v = 13, 4
    Pt = GC.identity(n)
    Pt[v, 0] = Pt[v, 1]
    q = C.snapshot(np.random.RandomState(8), n)
    tr = GO.Trackers(C.chord_ring(n), Pt=Pt)
    st = tr.run(10, q)
    assert st["flags"] == GO.BAD_ROW
    s = tr.stamps()
    assert s[v, v] == 10 and (np.delete(s[v], v) == 0).all()
    assert (s[:, v] > 0).all() and st["n_unknown"] == n - 1


def test_a_row_change_between_calls_rewires_the_subscriptions():
    """Vehicle 0 swaps points with vehicle 6 in its own row: it now hears the
    neighbours of point 6 (5, 7 and, over the chord, whoever holds point 0: 6)
    and no longer 1 and 12."""
    n = 13
    adj = C.chord_ring(n)
    tr = GO.Trackers(adj)
    assert tr.subscribed(0) == [1, 6, 12]
    q1, q2 = (C.snapshot(np.random.RandomState(s), n) for s in (1, 2))
    tr.run(2, q1)
    tr.Pt[0, 0], tr.Pt[0, 6] = 6, 0
    assert tr.subscribed(0) == [5, 6, 7]
    before = tr.stamps()[0].copy()
    tr.run(1, q2)
    s = tr.stamps()[0]
    assert s[5] == s[7] == 3 and s[1] == before[1] and s[12] == before[12]
    np.testing.assert_array_equal(tr.est()[0, 5], q2[5])
    np.testing.assert_array_equal(tr.est()[0, 1], q1[1])


# ---- loss ----

def test_loss_totals_per_seed_and_stale_neighbours():
    q = C.snapshot(np.random.RandomState(4), 13)
    adj = C.chord_ring(13)
    totals = []
    for seed in range(8):
        tr = GC.ring_loss(seed)
        st = tr.run(GC.LOSS_ROUNDS, q)
        totals.append(sum(tr.n_lost))
        ages = tr.round - tr.stamps()
        # at least one subscribed sender's entry is one round old
        assert any(ages[w][u] == 1 for w in range(13) for u in tr.subscribed(w)), seed
        assert st["n_unknown"] == 0
    print(totals)
    assert totals == GC.LOSS_TOTALS
    assert (adj.sum(axis=1) == np.array([len(tr.subscribed(w)) for w in range(13)])).all()


def test_a_dead_link_loses_one_table_per_round():
    """two_rings(6), no chords: vehicle 2 hears 1 and 3. Link 3 -> 2 dead: one
    table lost per round at 2, and 3's entry reaches 2 over 4, 5, 0, 1 (five
    hops: its age settles at 4). Both links into 2 dead: 2 hears nothing and
    knows only itself. Both links dying after three clean rounds: nobody relays
    3's entry to 2 any more, and its age grows by one per round."""
    q = np.ones((12, 3))
    loss = np.zeros((12, 12), np.int64)
    loss[2, 3] = LO.DEAD
    tr = GO.Trackers(C.two_rings(6), loss=loss, seed=9)
    for r in range(1, 9):
        tr.run(1, q)
        assert tr.n_lost[2] == r and sum(tr.n_lost) == r
    assert tr.round - tr.stamps()[2, 3] == 4
    loss[2, 1] = LO.DEAD
    tr = GO.Trackers(C.two_rings(6), loss=loss, seed=9)
    tr.run(8, q)
    assert tr.n_lost[2] == 16 and (np.delete(tr.stamps()[2], 2) == 0).all()
    # a dead link whose entry nobody relays: the age grows by one per round
    tr = GO.Trackers(C.two_rings(6), seed=9)
    tr.run(3, q)
    tr.loss[2, 3] = tr.loss[2, 1] = LO.DEAD
    ages = []
    for _ in range(4):
        tr.run(1, q)
        ages.append(int(tr.round - tr.stamps()[2, 3]))
    assert ages == [1, 2, 3, 4]


# ---- the own-estimate auction ----

LOSS_BATCHES = [("item5", "swarm6"), ("item5", "ring13"), ("rings", 64), ("rings", 65),
                ("rings", 128), ("matrices13",), ("wrap13",)]


@pytest.mark.parametrize("key", LOSS_BATCHES, ids=lambda k: "-".join(str(x) for x in k))
def test_a_est_equal_to_q_is_the_lossy_restatement(key):
    """(a) every committed loss batch (and the two dead-link cases below): every
    window's status and state."""
    for lc, (fl0, recs0) in zip(getattr(LC, key[0])(*key[1:]), LC.cpu_batch(*key)):
        fl, recs = DC.run_oracle(GC.EstCase(lc))
        assert len(recs) == len(recs0)
        for k, (r, r0) in enumerate(zip(recs, recs0)):
            assert r["status"] == r0["status"], (lc.name, k)
            for name in C.STATE_KEYS + ("queue_len",):
                np.testing.assert_array_equal(r["state"][name], r0["state"][name],
                                              err_msg=f"{lc.name} window {k}: {name}")
        np.testing.assert_array_equal(fl.n_lost, fl0.n_lost)
        np.testing.assert_array_equal(fl.qv, fl0.qv)


def one_round_auctions(sc_name="rows13"):
    """(b): the scenario's rows and snapshot; one lossless round on fresh
    trackers; the auction from own estimates and the shared-snapshot one."""
    sc = DC.SCENARIOS[sc_name]()
    n, q = sc.n, sc.windows[0][1]
    tr = GO.Trackers(sc.adj, Pt=sc.Pt)
    st = tr.run(1, q)
    rows = GC.identity(n) if sc.Pt is None else np.asarray(sc.Pt)
    est = tr.est()
    fe = EO.EstFleet(sc.p, sc.adj, 1, Pt=sc.Pt)
    se = fe.run(sc.ticks, cmd=C._all(n), Rt=EO.align_rt(sc.p, sc.adj, est, rows), est=est)
    fs = LO.LossyFleet(sc.p, sc.adj, 1, Pt=sc.Pt)
    ss = fs.run(sc.ticks, q=q, cmd=C._all(n), Rt=C.align_rt(sc.p, sc.adj, q, rows))
    return sc, tr, st, (fe, se), (fs, ss)


def test_a_on_the_dead_link_cases():
    for lc, cap in ((LC.dead_link()[0], None), (LC.dead_into_3(), 2)):
        fl0, recs0 = DC.run_oracle(lc)
        fl, recs = DC.run_oracle(GC.EstCase(lc))
        assert [r["status"] for r in recs] == [r["status"] for r in recs0]
        for name in C.STATE_KEYS:
            np.testing.assert_array_equal(np.array(getattr(fl, name)), np.array(getattr(fl0, name)))
        np.testing.assert_array_equal(fl.n_lost, fl0.n_lost)
        assert fl.n_lost.sum() > 0


@pytest.mark.parametrize("name", ["ring13", "rows13"])
def test_b_one_round_is_enough_for_the_auction(name):
    sc, tr, st, (fe, se), (fs, ss) = one_round_auctions(name)
    n = sc.n
    deg = sc.adj.sum(axis=1)
    s = tr.stamps()
    for w in range(n):  # n - 1 - deg vehicles still at the origin
        i = tr._point(w)
        unknown = np.where(s[w] == 0)[0]
        assert len(unknown) == n - 1 - deg[i] > 0
        assert not tr.est()[w, unknown].any()
    assert st["n_unknown"] == n * (n - 1) - int(deg.sum())
    assert se == ss and se["flags"] & FO.QUIESCENT
    for k in C.STATE_KEYS:
        a, b = np.array(getattr(fe, k)), np.array(getattr(fs, k))
        if k.endswith("price"):
            a, b = a.view(np.uint32), b.view(np.uint32)
        np.testing.assert_array_equal(a, b, err_msg=k)
    np.testing.assert_array_equal(fe.Rt.view(np.uint64), fs.Rt.view(np.uint64))
    assert ((fe.vflags & FO.V_CONSENSUS) != 0).all()


def test_c_the_stale_batch_meets_its_condition():
    sb, trs, runs, shared = GC.stale13()
    assert GC.stale_condition(runs, shared)
    assert sum(trs[0].n_lost) == 0 and all(sum(tr.n_lost) > 0 for tr in trs[1:])
    # every swarm has heard of everybody; the lossless one holds, per entry, the
    # true position of the round its age names
    for tr in trs:
        assert tr.status()["n_unknown"] == 0
    s, e = trs[0].stamps(), trs[0].est()
    for w in range(sb.n):
        for i in range(sb.n):
            np.testing.assert_array_equal(e[w, i], sb.traj[s[w, i] - 1][i])
    assert (trs[0].round - s).max() == 5
    # the lossy swarms ran a clean auction all the same: consensus everywhere
    for fl, st in runs:
        assert st["n_open"] == 0 and ((fl.vflags & FO.V_CONSENSUS) != 0).all()
    # and a batch that does not meet the condition is told apart: swarm 0 twice
    assert not GC.stale_condition([runs[0], runs[0]], shared)
    assert not GC.stale_condition(runs[1:], shared)


# ---- the ABI without a GPU ----

def test_exports_and_struct_layouts():
    from aclswarm_amd import _lib as L
    lib = L.lib()
    for s in ("acl_fleet_localize_batch", "acl_fleet_est_auction_batch"):
        assert s in L.EXPORTS and hasattr(lib, s)
    assert ct.sizeof(L.FleetLocalizeArgs) == 96 and L.FleetLocalizeArgs.fidx.offset == 16
    assert L.FleetLocalizeArgs.status.offset == 88
    assert ct.sizeof(L.FleetEstArgs) == ct.sizeof(L.FleetLossyArgs) + 8
    assert (L.FleetEstArgs.lossy.offset, L.FleetEstArgs.est.offset) == (0, ct.sizeof(L.FleetLossyArgs))
    assert L.FLEET_LOCALIZE_STATUS_DTYPE.itemsize == 16
    assert L.FLEET_LOC_BAD_ROW == GO.BAD_ROW and L.FLEET_BAD_INPUT == GO.BAD_INPUT
    assert lib.acl_abi_version() == 11


def test_localize_argument_errors_without_gpu():
    from aclswarm_amd import _lib as L
    lib = L.lib()
    call = lib.acl_fleet_localize_batch
    name = b"acl_fleet_localize_batch: "
    F = L.Formations(129, 1, None, 8, None, None)
    a = L.FleetLocalizeArgs()

    def fails(msg):
        assert call(ct.byref(F), ct.byref(a), None) == 1  # INVALID_ARG
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
    for k in ("fidx", "Pt", "stamp", "est", "round", "status"):
        setattr(a, k, 8)  # never dereferenced: the calls below fail their checks
    for k in ("fidx", "Pt", "stamp", "est", "round", "status"):
        setattr(a, k, None)
        fails(b"required pointer is NULL")
        setattr(a, k, 8)
    fails(b"rounds > 0 and q is NULL")
    a.q = 8
    a.loss = 8
    fails(b"loss is given and seed is NULL")
    a.seed = 8
    fails(b"loss is given and n_lost is NULL")
    a.loss = None
    fails(b"seed is given and loss is NULL")
    a.seed = None
    F.adj = None
    fails(b"required pointer is NULL")
    F.adj = 8
    F.n_formations = 0
    fails(b"formation table is empty")
    F.n_formations = 1
    a.B = 0
    a.fidx = None
    assert call(ct.byref(F), ct.byref(a), None) == 0  # empty batch
    assert call(None, ct.byref(a), None) == 1 and call(ct.byref(F), None, None) == 1
    assert lib.acl_last_error() == name + b"null argument"


def test_est_auction_argument_errors_without_gpu():
    from aclswarm_amd import _lib as L
    lib = L.lib()
    call = lib.acl_fleet_est_auction_batch
    name = b"acl_fleet_est_auction_batch: "
    F = L.Formations(129, 1, 8, 8, None, None)
    ea = L.FleetEstArgs()
    lo = ea.lossy
    d, a = lo.delay, lo.delay.base

    def fails(msg):
        assert call(ct.byref(F), ct.byref(ea), None) == 1  # INVALID_ARG
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
    for k, _ in L.FleetAuctionArgs._fields_[4:-1]:
        setattr(a, k, 8)  # never dereferenced
    a.hist_biditer = a.hist_open = None
    a.q = None  # ignored by this entry
    a.workspace_bytes = lib.acl_fleet_delay_workspace_bytes(13, 1, 4, 3)
    fails(b"lat is NULL")
    d.lat = 8
    d.max_lat = 65
    fails(b"max_lat out of range [1, 64]")
    d.max_lat = 3
    lo.link.loss = lo.link.seed = lo.link.n_lost = 8
    for k, msg in (("loss", b"loss is NULL"), ("seed", b"seed is NULL"),
                   ("n_lost", b"n_lost is NULL")):
        setattr(lo.link, k, None)
        fails(msg)
        setattr(lo.link, k, 8)
    fails(b"cmd is given and est is NULL")
    ea.est = 8
    a.workspace_bytes -= 1
    fails(b"workspace_bytes is too small (acl_fleet_delay_workspace_bytes)")
    a.workspace_bytes += 1
    a.ticks = 0
    fails(b"at least one tick")
    a.ticks = 1
    F.n_formations = 0
    fails(b"formation table is empty")
    F.n_formations = 1
    a.B = 0
    ea.est = None
    assert call(ct.byref(F), ct.byref(ea), None) == 0  # empty batch
    assert call(None, ct.byref(ea), None) == 1 and call(ct.byref(F), None, None) == 1
    assert lib.acl_last_error() == name + b"null argument"
    # the lossy entry still wants its q
    a.B, ea.est = 1, 8
    assert lib.acl_fleet_lossy_auction_batch(ct.byref(F), ct.byref(lo), None) == 1
    assert b"cmd is given and q is NULL" in lib.acl_last_error()
