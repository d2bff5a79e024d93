"""CPU tests of the trials on each vehicle's own estimates
(acl_fleet_est_trial_batch): the restatement tests/fleet_est_trial_oracle.py on
the cases of tests/fleet_est_trial_cases.py -- its two reductions, the
conditions that make ring13_two distinguish the published-assignment model
from the auctioneer-row one, the input condition of the collision decisions,
the figures the cases' docstring quotes -- and the C entry's ABI and argument
errors, which need no GPU."""
import ctypes as ct

import numpy as np
import pytest

import fleet_auction_oracle as FO
import fleet_est_episode_oracle as XO
import fleet_est_trial_cases as X
import fleet_localize_oracle as GO
import trial_oracle as T


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _ident(n):
    return np.tile(np.arange(n), (n, 1))


# ---- the reductions ----

@pytest.mark.parametrize("name", ["ring13_one", "single", "ring65_te2"])
def test_reduction_a_one_formation_is_the_episode_localization(name):
    """K = 1: loc_rows equal the auctioneers' rows after every step, and the
    trackers are those of the est-episode restatement's gossip -- a
    fleet_localize_oracle.Trackers on the formation's graph whose rows are the
    fleet's of the moment, one round on the step's q every track_every steps."""
    cs, ft, recs = X.cpu_run(name)
    adj = cs.forms[0][1]
    tr = GO.Trackers(adj, loss=cs.loss, seed=cs.seed)
    rows = _ident(cs.n)
    for r in recs:
        if r["step"] % cs.track_every == 0:
            tr.Pt = rows.copy()
            st = tr.run(1, r["q0"])
            assert st == r["loc"], r["step"]
            np.testing.assert_array_equal(r["gossip_rows"], rows)
        else:
            assert r["loc"] is None
        np.testing.assert_array_equal(r["stamps"], tr.stamps())
        np.testing.assert_array_equal(_bits(r["est"]), _bits(tr.est()))
        np.testing.assert_array_equal(r["loc_rows"], r["Pt"])
        rows = r["Pt"]
    if name == "ring13_one":
        assert (rows != _ident(13)).any() and (rows == rows[0]).all()


def test_reduction_b_complete_graphs_equal_the_lossy_trial():
    """sync6_complete: after the step's round every table is q bit for bit, and
    the flight is the shared-snapshot trial's record for record: commands,
    flags, statuses, rows, controller starts, supervisor states; u, q and vel
    to 1e-9 (the two control steps sum in different orders)."""
    cs, ft, recs = X.cpu_run("sync6_complete")
    sh, srecs = X.cpu_shared("sync6_complete")
    assert len(recs) == len(srecs) == cs.steps
    for r, s in zip(recs, srecs):
        what = f"step {r['step']}"
        np.testing.assert_array_equal(_bits(r["est"]),
                                      _bits(np.broadcast_to(r["q0"], (6, 6, 3))), err_msg=what)
        assert r["err2"] == (0.0, 0.0, 0.0), what
        for k in ("raised", "P", "ctl_on", "on", "ca", "n_thrown", "invalid", "open"):
            np.testing.assert_array_equal(r[k], s[k], err_msg=f"{what}: {k}")
        assert (r["cmd"] is None) == (s["cmd"] is None), what
        if r["cmd"] is not None:
            np.testing.assert_array_equal(r["cmd"], s["cmd"], err_msg=what)
        for k in ("status", "state", "committed", "per_vehicle", "lost"):
            assert r[k] == s[k], (what, k)
        for k in ("u", "us", "q", "vel"):
            np.testing.assert_allclose(r[k], s[k], rtol=0, atol=1e-9, err_msg=f"{what}: {k}")
    assert ft.fst == sh.fst and ft.sup.state == sh.sup.state
    np.testing.assert_array_equal(ft.fleet.Pt, sh.fleet.Pt)
    np.testing.assert_array_equal(ft.adopt_step, sh.adopt_step)
    assert (ft.xst["rounds_run"], ft.xst["n_unknown"], ft.xst["max_age"]) == (cs.steps, 0, 0)


# ---- what ring13_two is for ----

def _window(recs):
    """The steps from the forced commit up to and including the second adoption."""
    ad = sorted(X.adoption_steps(recs))
    return X.RING13_COMMIT_AT, ad[1]


def _subscribers(adj, rows):
    tr = GO.Trackers(adj, Pt=rows)
    return [tr.subscribed(w) for w in range(len(adj))]


def test_ring13_two_distinguishes_the_published_rows_from_the_auctioneers():
    cs, ft, recs = X.cpu_run("ring13_two")
    cw, wrong, wrecs = X.cpu_run("ring13_two", "auction")
    n = 13
    assert X.commit_steps(recs) == X.commit_steps(wrecs) == [3, X.RING13_COMMIT_AT]
    first = min(X.adoption_steps(recs))
    # 1. the first adoption installs a row that is not the identity: the
    #    auction answers the swapped start by exchanging vehicles 3 and 5
    row = recs[first]["loc_rows"][0]
    assert (recs[first]["loc_rows"] == row).all()
    assert np.nonzero(row != np.arange(n))[0].tolist() == [3, 5] and (row[3], row[5]) == (5, 3)
    lo, hi = _window(recs)
    assert first < lo < hi
    # 2. under the new adjacency the published rows and the identity subscribe
    #    some vehicle to different senders, in the rounds of the window
    adj2 = cs.forms[1][1]
    differ = 0
    for r in recs[lo:hi + 1]:
        assert r["fidx"] == 1
        if r["gossip_rows"] is not None:
            a, b = _subscribers(adj2, r["gossip_rows"]), _subscribers(adj2, _ident(n))
            differ += sum(x != y for x, y in zip(a, b))
    assert differ > 0
    # (the auctioneers' rows ARE the identity there: the commit reset them)
    assert all((w["gossip_rows"] == _ident(n)).all() for w in wrecs[lo:hi]
               if w["gossip_rows"] is not None)
    # 3. flown under the auctioneers' rows, a stamp differs in the window
    assert X.STAMPS_DIFFER_AT in range(lo, hi + 1)
    for s, (r, w) in enumerate(zip(recs, wrecs)):
        same = np.array_equal(r["stamps"], w["stamps"])
        assert same == (s < X.STAMPS_DIFFER_AT) or s > hi, s
    # 4. a START in the window reads a table that differs between the two
    starts = [s for s in range(lo, hi + 1) if recs[s]["cmd"] is not None]
    assert starts == [lo + 1] and (recs[lo + 1]["cmd"] == FO.START).all()
    r, w = recs[lo + 1], wrecs[lo + 1]
    assert any(not np.array_equal(_bits(r["est"][v]), _bits(w["est"][v])) for v in range(n))
    # outside the window the two models agree: no formation change, no difference
    for r, w in zip(recs[:lo], wrecs[:lo]):
        np.testing.assert_array_equal(_bits(r["est"]), _bits(w["est"]))


def test_ring13_two_the_rows_survive_the_commit_and_follow_the_adoption():
    """loc_rows change at the steps of an adoption only, to the adopters' rows;
    the commit resets the auctioneers' rows and leaves loc_rows alone."""
    cs, ft, recs = X.cpu_run("ring13_two")
    prev = _ident(13)
    for r in recs:
        ad = (r["raised"] & FO.V_ADOPTED) != 0
        np.testing.assert_array_equal(r["loc_rows"][~ad], prev[~ad])
        np.testing.assert_array_equal(r["loc_rows"][ad], r["Pt"][ad])
        if r["committed"]:
            assert (r["Pt"] == _ident(13)).all() and not r["ctl_on"].any()
        prev = r["loc_rows"]
    c = recs[X.RING13_COMMIT_AT]
    assert (c["loc_rows"] != _ident(13)).any()
    # err2_nbr is taken over the running controllers: none between commit and
    # adoption, where the episode's sentence (every vehicle) finds wrong entries
    lo, hi = _window(recs)
    assert all(r["err2"][1] == 0.0 and r["err2"][2] > 0.0 for r in recs[lo:hi])
    adj2 = cs.forms[1][1]
    ungated = [XO.err2_record(r["est"], r["stamps"], r["q0"], r["Pt"], adj2) for r in recs[lo:hi]]
    assert all(u[0] == r["err2"][0] and u[2] == r["err2"][2] for u, r in zip(ungated, recs[lo:hi]))
    assert max(u[1] for u in ungated) > 0.0
    assert recs[hi + 1]["err2"][1] > 0.0


# ---- the input condition and the quoted figures ----

def test_collision_decisions_keep_the_input_condition():
    seen = {}
    for name in X.CASES:
        cs, ft, recs = X.cpu_run(name)
        seen[name] = d, e, q = X.condition(recs)
        assert d >= X.D_MARGIN and e >= X.ANGLE_MARGIN and q >= X.ANGLE_MARGIN, (name, d, e, q)
    d, e, q = seen["ring13_one"]
    assert 0.46 < d < 0.47 and 0.36 < e < 0.37 and 0.26 < q < 0.27
    assert all(seen[k] == (np.inf,) * 3 for k in seen if k != "ring13_one")


def _figures(name):
    cs, ft, recs = X.cpu_run(name)
    return dict(adopt={k: len(v) for k, v in X.adoption_steps(recs).items()},
                commits=X.commit_steps(recs), rounds=ft.xst["rounds_run"],
                unknown=ft.xst["n_unknown"], tables_lost=sum(ft.trackers.n_lost),
                bids_lost=int(ft.fleet.n_lost.sum()),
                ca=sum(int(r["ca"][r["on"]].sum()) for r in recs), state=ft.sup.state)


def test_the_figures_the_cases_quote():
    fly, wait = T.FLYING, T.WAITING
    want = {
        "single": dict(adopt={}, commits=[3], rounds=8, unknown=0, tables_lost=0, bids_lost=0,
                       ca=0, state=wait),
        "sync6_complete": dict(adopt={9: 6, 18: 6}, commits=[3, X.SYNC6_COMMIT_AT], rounds=21,
                               unknown=0, tables_lost=0, bids_lost=0, ca=0, state=fly),
        "ring13_one": dict(adopt={11: 13}, commits=[3], rounds=11, unknown=0, tables_lost=0,
                           bids_lost=0, ca=11, state=fly),
        "ring13_two": dict(adopt={11: 13, 22: 13}, commits=[3, X.RING13_COMMIT_AT], rounds=13,
                           unknown=0, tables_lost=0, bids_lost=0, ca=0, state=fly),
        "ring13_two_loss": dict(adopt={}, commits=[3, X.RING13_COMMIT_AT], rounds=10, unknown=0,
                                tables_lost=19, bids_lost=9, ca=0, state=wait),
        "rings12_two": dict(adopt={}, commits=[3, 10], rounds=8, unknown=72, tables_lost=0,
                            bids_lost=0, ca=0, state=wait),
        "ring65_te2": dict(adopt={}, commits=[3], rounds=6, unknown=3236, tables_lost=0,
                           bids_lost=0, ca=0, state=wait),
        "near128_two": dict(adopt={14: 9, 15: 27}, commits=[3, X.NEAR128_COMMIT_AT], rounds=10,
                            unknown=13282, tables_lost=0, bids_lost=0, ca=0, state=fly),
    }
    assert set(want) == set(X.CASES)
    for name, w in want.items():
        assert _figures(name) == w, name
    # rings12: every auction INVALID, every entry across the components unknown throughout
    cs, ft, recs = X.cpu_run("rings12_two")
    unknown = [r["loc"]["n_unknown"] for r in recs if r["loc"]]
    assert min(unknown) == 72 and unknown[3:] == [72] * (len(unknown) - 3)  # (diameter 3)
    assert ft.fst["n_invalid"] > 0 and ft.fst["n_adopted"] == 0
    # near128: the adopters are a strict subset in both halves of the lane range
    cs, ft, recs = X.cpu_run("near128_two")
    ad = np.nonzero(ft.adopt_step >= 0)[0]
    assert 0 < (ad < 64).sum() < 64 and 0 < (ad >= 64).sum() < 64
    changed = (recs[-1]["loc_rows"] != _ident(128)).any(axis=1)
    np.testing.assert_array_equal(np.nonzero(changed)[0], ad)
    assert recs[X.NEAR128_COMMIT_AT]["committed"] and changed.any()
    # under loss the rows stay the identity across the commit
    cs, ft, recs = X.cpu_run("ring13_two_loss")
    assert (ft.loc_rows == _ident(13)).all()


def test_a_finished_trial_stands_still():
    """A trial whose formation sequence is out of range ends at step 0: no
    round, no tick, no record."""
    cs = X.case("ring13_one")
    ft = cs.oracle()
    ft.fbad, ft.t.fidx = True, 0
    r = ft.step()
    assert ft.t.done and not r["live"] and r["loc"] is None and r["err2"] is None
    assert ft.trackers.round == 0 and ft.xst["rounds_run"] == 0
    assert r["status"]["flags"] == 0x4


# ---- the ABI without a GPU ----

def test_exports_and_struct_layout():
    from aclswarm_amd import _lib as L
    import aclswarm_amd
    lib = L.lib()
    for fn in ("acl_fleet_est_trial_workspace_bytes", "acl_fleet_est_trial_init",
               "acl_fleet_est_trial_batch"):
        assert fn in L.EXPORTS and hasattr(lib, fn)
    assert "FleetEstTrial" in aclswarm_amd.__all__
    A = L.FleetEstTrialArgs
    base = ct.sizeof(L.FleetLossyTrialArgs)
    assert ct.sizeof(A) == base + 8 + 7 * 8
    assert (A.track_every.offset, A.diag.offset, A.loc_stamp.offset, A.loc_Pt.offset,
            A.xst.offset, A.err2_hist.offset) == \
        (base, base + 4, base + 8, base + 40, base + 48, base + 56)
    assert lib.acl_abi_version() == 11
    # the delay-trial layout, two 16-byte status arrays appended
    for n, B, cap, ml in ((13, 3, 52, 5), (128, 8, 512, 1), (1, 1, 4, 64)):
        d = lib.acl_fleet_delay_trial_workspace_bytes(n, B, cap, ml)
        x = lib.acl_fleet_est_trial_workspace_bytes(n, B, cap, ml)
        assert d < x <= d + 2 * (16 * B + 256)
    for bad in ((0, 1, 4, 1), (129, 1, 4, 1), (13, 0, 4, 1), (13, 1, 0, 1), (13, 1, 4, 0),
                (13, 1, 4, 65)):
        assert lib.acl_fleet_est_trial_workspace_bytes(*bad) == 0


TRIAL_PTRS = ("fseq", "fidx", "q", "vel", "P", "ts", "ctl_on", "ring_u", "ring_ca", "posf", "dist",
              "t_conv", "t_avoid", "n_assign", "Pt", "open", "invalid", "just_received", "biditer",
              "price", "who", "Rt", "final_price", "final_who", "done_tick", "vflags", "n_thrown",
              "n_tally", "queue_len", "status", "adopt_step", "fst", "workspace")
OWN_PTRS = ("loc_stamp", "loc_est", "loc_round", "loc_n_lost", "loc_Pt", "xst")


def test_argument_errors_of_the_c_entries_without_gpu():
    from aclswarm_amd import _lib as L
    lib = L.lib()
    F = L.Formations(13, 2, 8, 8, 8, 8, 5, None)

    def args():
        x = L.FleetEstTrialArgs()
        a = x.lossy.delay.base
        a.B, a.K, a.step0, a.steps = 1, 2, 0, 1
        a.ticks_per_step, a.max_iter, a.queue_cap = 10, 0, 52
        for k in TRIAL_PTRS:
            setattr(a, k, 8)  # never dereferenced: every call below fails its checks
        a.workspace_bytes = lib.acl_fleet_est_trial_workspace_bytes(13, 1, 52, 2) - 1
        a.cntrl, a.safety, a.tp = L.default_gains(), L.default_safety(), L.default_trial_params()
        x.lossy.delay.lat, x.lossy.delay.max_lat = 8, 2
        x.lossy.link.loss = x.lossy.link.seed = x.lossy.link.n_lost = 8
        x.track_every, x.diag = 2, 1
        for k in OWN_PTRS:
            setattr(x, k, 8)
        return x

    calls = {b"acl_fleet_est_trial_batch: ": lambda x, F=F: lib.acl_fleet_est_trial_batch(
                 ct.byref(F), ct.byref(x), None),
             b"acl_fleet_est_trial_init: ": lambda x, F=F: lib.acl_fleet_est_trial_init(
                 ct.byref(x), F.n, None)}
    for name, call in calls.items():
        batch = name.startswith(b"acl_fleet_est_trial_batch")

        def fails(x, msg, F=F):
            assert call(x, F) == 1  # INVALID_ARG
            err = lib.acl_last_error()
            assert err.startswith(name) and msg in err, err

        # the workspace of the new size is asked for, by name; the delay entry's is too small
        fails(args(), b"workspace_bytes is too small (acl_fleet_est_trial_workspace_bytes)")
        x = args()
        x.lossy.delay.base.workspace_bytes = lib.acl_fleet_delay_trial_workspace_bytes(13, 1, 52, 2)
        fails(x, b"acl_fleet_est_trial_workspace_bytes")
        for bad in (0, -3):
            x = args()
            x.track_every = bad
            fails(x, b"track_every < 1")
        x = args()  # ... reported even when there is nothing to fly
        x.track_every, x.lossy.delay.base.steps = 0, 0
        fails(x, b"track_every < 1")
        for k in OWN_PTRS:
            x = args()
            setattr(x, k, None)
            fails(x, b"loc_stamp, loc_est, loc_round, loc_n_lost, loc_Pt or xst is NULL")
        x = args()  # err2_hist may be NULL
        x.err2_hist = None
        fails(x, b"workspace_bytes")
        # the lossy trial entry's checks on `lossy`
        if batch:  # (the init reads no loss matrix)
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
        x.lossy.delay.base.K = 0
        fails(x, b"K >= 1")
        x = args()
        x.lossy.delay.base.adopt_step = None
        fails(x, b"required pointer is NULL")
        x = args()
        x.lossy.delay.base.tp.ep.auction_latency = 3
        fails(x, b"auction_latency")
        for n in (0, 129):
            fails(args(), b"n out of range [1, 128]", L.Formations(n, 2, 8, 8, 8, 8, 5, None))
        # nothing to do: no pointer is looked at
        for k, v in (("B", 0),) + ((("steps", 0),) if batch else ()):
            x = L.FleetEstTrialArgs()
            a = x.lossy.delay.base
            a.B, a.K, a.steps, a.ticks_per_step, a.queue_cap = 1, 1, 1, 10, 52
            setattr(a, k, v)
            a.tp = L.default_trial_params()
            x.lossy.delay.max_lat, x.track_every = 1, 1
            assert call(x, F) == 0
    assert lib.acl_fleet_est_trial_batch(None, ct.byref(args()), None) == 1
    assert lib.acl_fleet_est_trial_batch(ct.byref(F), None, None) == 1
    assert lib.acl_last_error() == b"acl_fleet_est_trial_batch: null argument"
    assert lib.acl_fleet_est_trial_init(None, 13, None) == 1
    assert lib.acl_last_error() == b"acl_fleet_est_trial_init: null argument"
