"""GPU parity of acl_fleet_est_trial_init / acl_fleet_est_trial_batch (the
trials on each vehicle's own estimates) against the plain-Python restatement
tests/fleet_est_trial_oracle.py.

Teacher-forced exactly as tests/test_gpu_fleet_loss_trial.py and
tests/test_gpu_fleet_est_episode.py (whose helpers and tolerances these are):
one control step per call; before step k the restatement takes the GPU's q and
vel, at START steps the GPU's Rt (bits pinned to acl_vehicle_start_batch's on
the B n tables); after it every fleet state and output array, adopt_step, P,
ctl_on, fidx, the trial status, the status structs, the step's flags, n_lost,
the trackers (loc_stamp, loc_est, loc_round, loc_n_lost), loc_Pt, xst and the
error record are bit-exact, u within 1e-5 relative, CA flags exact, q / vel
within 1e-9; at the end the records bit for bit. Then: ring13_two against the
WRONG model (gossip under the auctioneers' rows), the complete-graph reduction
against acl_fleet_lossy_trial_batch on the same GPU, chunked calls, diag off
against on, a BAD_INPUT swarm and a finished trial between good ones, a trial
that moves between the two entries, the init's outputs, the argument errors.

track_every is an argument of the call: the chord rings of 13 at track_every 2
fly as the swarms of one launch."""
import ctypes as ct

import numpy as np
import pytest

import fleet_auction_cases as C
import fleet_auction_oracle as FO
import fleet_est_trial_cases as X
import test_gpu_fleet_delay_trial as GT
import test_gpu_fleet_est as GX
from test_fleet_est_trial import test_argument_errors_of_the_c_entries_without_gpu  # noqa: F401
from test_gpu_fleet_trial import (FLEET_KEYS, Q_ATOL, STATE, U_RTOL, _adoptions, _bits, _check_rt,
                                  _check_status, _dev, _force_commit, _params, _t, _u16,
                                  _write_ts)

pytestmark = pytest.mark.gpu

LOC = ("loc_stamp", "loc_est", "loc_round", "loc_n_lost", "loc_Pt")
XSTATE = STATE + ("n_lost", "xst") + LOC
XINT = ("rounds_run", "n_unknown", "max_age", "flags")
XERR = ("err2_own", "err2_nbr", "err2_all")


def _batch(cases):
    """test_gpu_fleet_delay_trial._lat_batch and the swarms' loss matrices,
    seeds and the call's track_every."""
    assert len({c.track_every for c in cases}) == 1
    bt = GT._lat_batch(cases)
    bt["loss"] = np.stack([c.loss for c in cases])
    bt["seed"] = np.array([c.seed for c in cases], np.uint32)
    bt["te"] = cases[0].track_every
    bt["cases"] = cases
    return bt


def _trial(bt, diag=True, own=True):
    """own False: a FleetTrial on acl_fleet_lossy_trial_batch."""
    from aclswarm_amd import engine
    c0 = bt["case"]
    p, adj, G = zip(*bt["forms"])
    Tb = engine.FormationTable.from_host(list(p), list(adj), list(G), device=_dev())
    kw = dict(params=_params(c0), max_iter=c0.max_iter, ticks_per_step=c0.T,
              latency=_t(bt["lat"], np.uint8), max_latency=bt["max_lat"], loss=_u16(bt["loss"]),
              loss_seed=_t(bt["seed"].view(np.int32), np.int32))
    if own:
        kw.update(track_every=bt["te"], diag=diag)
    cls = engine.FleetEstTrial if own else engine.FleetTrial
    return cls(Tb, _t(bt["fseq"], np.int32), _t(bt["q"], np.float64), _t(bt["vel"], np.float64),
               **kw)


def _oracles(bt, follow="published"):
    import fleet_est_trial_oracle as XT
    c0 = bt["case"]
    return [XT.EstFleetTrial(bt["fseq"][b], bt["forms"], bt["q"][b], bt["vel"][b], c0.tp,
                             bt["lat"][b], loss=bt["loss"][b], seed=int(bt["seed"][b]),
                             max_iter=c0.max_iter, ticks_per_step=c0.T, track_every=bt["te"],
                             diag=True, loc_rows_follow=follow)
            for b in range(len(bt["fseq"]))]


def _state(ft, keys=XSTATE):
    import torch
    torch.cuda.synchronize()
    d = {k: getattr(ft, k).cpu().numpy() for k in keys}
    for k in ("Pt", "loc_Pt"):
        if k in d:
            d[k] = d[k].view(np.uint16).astype(np.int64)
    d["P"] = d["P"].view(np.uint16)
    return d


def _xst(a):
    from aclswarm_amd import _lib as L
    return np.ascontiguousarray(a).view(L.FLEET_EST_EPISODE_STATUS_DTYPE).reshape(-1)


def _forces(cases):
    """{step: [f(ft, oracles)]} of the cases' forced commits."""
    out = {}
    for b, c in enumerate(cases):
        for s in c.force:
            out.setdefault(s, []).append(_force_commit(b))
    return out


def _teacher_forced(cases, steps, own_at=lambda s: True, wrong=None):
    """Flies the cases step by step on the GPU and on the restatement; step s
    on the own-estimate entry when own_at(s), else on the lossy entry. wrong:
    (swarm, step): a second restatement of that swarm under the auctioneers'
    rows is flown along up to that step, where its stamps must differ from the
    device's. Returns (ft, oracles, records [step][swarm], histories)."""
    from aclswarm_amd import _lib as L
    bt = _batch(cases)
    ft = _trial(bt)
    oracles = _oracles(bt)
    bad = _oracles(bt, "auction")[wrong[0]] if wrong else None
    force = _forces(cases)
    B, n = bt["q"].shape[:2]
    ident = np.tile(np.arange(n), (n, 1))
    one = [len(set(c.fseq.tolist())) == 1 for c in cases]
    recs, hists = [], []
    for s in range(steps):
        own = own_at(s)
        for f in force.get(s, ()):
            f(ft, oracles)
            if bad is not None and s in cases[wrong[0]].force:
                cases[wrong[0]].force[s](bad)
        before = _state(ft)
        h = ft.run(1, history=True, own_estimates=own)
        got = _state(ft)
        h = {k: v.cpu().numpy()[0] for k, v in h.items()}
        h["P"] = h["P"].view(np.uint16)
        hists.append(h)
        assert ("err2" in h) == own
        ts = got["ts"].view(L.TRIAL_STATUS_DTYPE).reshape(-1)
        fs = got["fst"].view(L.FLEET_EPISODE_STATUS_DTYPE).reshape(-1)
        tk = got["_status"].view(L.FLEET_STATUS_DTYPE).reshape(-1)
        xs = _xst(got["xst"])
        row, cmds, rows = [], np.zeros((B, n), np.uint8), before["Pt"].copy()
        for b, o in enumerate(oracles):
            what = f"{cases[b].name} (swarm {b}) step {s}"
            o.q, o.vel = before["q"][b].copy(), before["vel"][b].copy()
            sup = (h["u"][b], h["ca"][b], h["q"][b])
            r = o.step(Rt=got["Rt"][b], sup=sup, own=own)
            row.append(r)
            if r["cmd"] is not None:
                cmds[b] = r["cmd"]
            if r["committed"]:
                rows[b] = ident
            exp = C.snapshot_state(o.fleet)
            for k in FLEET_KEYS:
                np.testing.assert_array_equal(_bits(got[k][b]),
                                              _bits(np.asarray(exp[k], got[k].dtype)),
                                              err_msg=f"{what}: {k}")
            np.testing.assert_array_equal(got["adopt_step"][b], o.adopt_step, err_msg=what)
            np.testing.assert_array_equal(got["ctl_on"][b], o.t.ctl_on, err_msg=what)
            np.testing.assert_array_equal(h["ctl"][b], r["on"], err_msg=what)
            np.testing.assert_array_equal(got["P"][b], o.P, err_msg=what)
            np.testing.assert_array_equal(h["P"][b], o.P, err_msg=what)
            assert got["fidx"][b] == o.t.fidx, what
            np.testing.assert_array_equal(h["vflags"][b], r["raised"], err_msg=what)
            np.testing.assert_array_equal(got["n_lost"][b], o.fleet.n_lost, err_msg=what)
            assert {k: int(tk[k][b]) for k in r["status"]} == r["status"], what
            assert {k: int(fs[k][b]) for k in o.fst} == o.fst, what
            _check_status(ts[b], o, what)
            assert h["state"][b] == o.sup.state, what
            # the trackers, the localization rows and the record
            tr = o.trackers
            np.testing.assert_array_equal(got["loc_stamp"][b], tr.stamps(), err_msg=what)
            np.testing.assert_array_equal(_bits(got["loc_est"][b]), _bits(tr.est()), err_msg=what)
            assert got["loc_round"][b] == tr.round, what
            np.testing.assert_array_equal(got["loc_n_lost"][b], tr.n_lost, err_msg=what)
            np.testing.assert_array_equal(got["loc_Pt"][b], o.loc_rows, err_msg=f"{what}: loc_Pt")
            if one[b] and all(own_at(t) for t in range(s + 1)):  # reduction (a)
                np.testing.assert_array_equal(got["loc_Pt"][b], got["Pt"][b], err_msg=what)
            assert {k: int(xs[k][b]) for k in XINT} == {k: o.xst[k] for k in XINT}, what
            np.testing.assert_array_equal(_bits(np.array([xs[k][b] for k in XERR])),
                                          _bits(np.array([o.xst[k] for k in XERR])), err_msg=what)
            if own:
                e = r["err2"] if r["err2"] is not None else (0.0, 0.0, 0.0)
                np.testing.assert_array_equal(_bits(h["err2"][b]), _bits(np.array(e)),
                                              err_msg=what)
            # the commands and the flight
            on = r["on"]
            if on.any():
                np.testing.assert_allclose(h["u"][b][on], r["u"][on], rtol=U_RTOL, atol=U_RTOL,
                                           err_msg=what)
                np.testing.assert_array_equal(h["ca"][b][on], r["ca"][on], err_msg=what)
            assert not h["u"][b][~on].any() and not h["ca"][b][~on].any(), what
            np.testing.assert_allclose(got["q"][b], o.q, rtol=0, atol=Q_ATOL, err_msg=what)
            np.testing.assert_allclose(got["vel"][b], o.vel, rtol=0, atol=Q_ATOL, err_msg=what)
            np.testing.assert_array_equal(h["q"][b], got["q"][b], err_msg=what)
            np.testing.assert_array_equal(h["vel"][b], got["vel"][b], err_msg=what)
            if bad is not None and b == wrong[0] and s <= wrong[1]:
                bad.q, bad.vel = before["q"][b].copy(), before["vel"][b].copy()
                bad.step(Rt=got["Rt"][b], sup=sup)
                same = np.array_equal(got["loc_stamp"][b], bad.trackers.stamps())
                assert same == (s < wrong[1]), f"{what}: against the auctioneers' rows"
        if own:  # the tables of this step: nothing after the round writes them
            assert GX._check_rt(ft, cmds, got["loc_est"], rows, got["Rt"]) == \
                int((cmds == FO.START).sum())
        else:
            _check_rt(ft, cmds, rows, got["fidx"], before["q"], got["Rt"])
        recs.append(row)
    rec = ft.records()
    for b, o in enumerate(oracles):
        r = o.sup.record()
        np.testing.assert_array_equal(rec["dist"][b].view(np.uint64),
                                      np.asarray(r["dist"], np.float64).view(np.uint64))
        np.testing.assert_array_equal(rec["time"][b], r["time"])
        np.testing.assert_array_equal(rec["time_avoidance"][b], r["time_avoidance"])
        np.testing.assert_array_equal(rec["assignments"][b], r["assignments"])
        assert (rec["state"][b], rec["last_state"][b], rec["done_step"][b]) == \
            (r["state"], r["last_state"], r["done_step"])
    return ft, oracles, recs, hists


def _n_adopt(hists, b):
    return {s: len(v) for s, v in _adoptions(hists, b).items()}


def test_parity_a_single_vehicle():
    """n = 1: no edge, nobody to hear of; the error record is three zeros."""
    cs = X.case("single")
    ft, oracles, recs, hists = _teacher_forced([cs], cs.steps)
    x = ft.fleet_status()["estimates"][0]
    assert (x["rounds_run"], x["n_unknown"], x["max_age"]) == (8, 0, 0)
    assert all(not h["err2"].any() for h in hists)


def test_parity_ring13_the_published_rows_not_the_auctioneers():
    """ring13_two, ring13_two_loss and ring13_one as the swarms of one launch.
    Swarm 0 matches the restatement under the PUBLISHED rows after every step;
    the same flight restated under the auctioneers' rows agrees up to the
    forced commit and has other stamps at step 14, the first round on (new
    graph, old assignment). Adoptions at steps 11 and 22; under loss 27 tables (26 steps)
    and 9 bids are lost and nobody adopts; loc_Pt == Pt throughout for K = 1."""
    cases = [X.case("ring13_two"), X.case("ring13_two_loss"), X.case("ring13_one")]
    ft, oracles, recs, hists = _teacher_forced(cases, 26, wrong=(0, X.STAMPS_DIFFER_AT))
    assert _n_adopt(hists, 0) == {11: 13, 22: 13} and _n_adopt(hists, 1) == {}
    assert _n_adopt(hists, 2) == {11: 13}
    assert GT._commit_steps(recs, 0) == GT._commit_steps(recs, 1) == [3, X.RING13_COMMIT_AT]
    assert GT._commit_steps(recs, 2) == [3]
    lp = ft.loc_Pt.cpu().numpy()
    assert (recs[X.RING13_COMMIT_AT][0]["loc_rows"] != np.arange(13)).any()
    assert (lp[1] == np.arange(13)).all()
    assert ft.loc_n_lost.cpu().numpy().sum(axis=1).tolist()[:2] == [0, 27]
    assert ft.n_lost.cpu().numpy().sum(axis=1).tolist()[:2] == [0, 9]
    x = ft.fleet_status()["estimates"]
    assert x["rounds_run"].tolist() == [13, 13, 13]
    assert (x["err2_all"][[0, 2]] > 0).all() and x["err2_all"][1] == 0  # (under loss nobody flies)
    assert sum(int(h["ca"][2].sum()) for h in hists) > 0  # collision avoidance flew


def test_parity_rings12_split_graph():
    """Two components: 72 entries unknown for the whole flight, every auction
    INVALID, loc_Pt stays the identity across the forced commit."""
    cs = X.case("rings12_two")
    ft, oracles, recs, hists = _teacher_forced([cs], cs.steps)
    assert ft.fleet_status()["estimates"][0]["n_unknown"] == 72
    fl = ft.fleet_status()["fleet"][0]
    assert fl["n_invalid"] > 0 and fl["n_adopted"] == 0
    assert GT._commit_steps(recs, 0) == [3, 10]


def test_parity_ring65_second_wave():
    """n = 65: the second wave with one live lane and the second mask word."""
    cs = X.case("ring65_te2")
    ft, oracles, recs, hists = _teacher_forced([cs], cs.steps)
    x = ft.fleet_status()["estimates"][0]
    assert (x["rounds_run"], x["n_unknown"]) == (6, 3236)


def test_parity_near128_a_strict_subset_adopts_in_both_halves():
    """n = 128: 9 vehicles adopt at step 14 and 27 at step 15; loc_Pt changes
    for exactly those, below and above lane 64; the forced commit of step 17
    leaves their rows in place."""
    cs = X.case("near128_two")
    ft, oracles, recs, hists = _teacher_forced([cs], cs.steps)
    assert _n_adopt(hists, 0) == {14: 9, 15: 27}
    ad = np.nonzero(ft.adopt_step.cpu().numpy()[0] >= 0)[0]
    lp = ft.loc_Pt.cpu().numpy()[0].view(np.uint16)
    changed = np.nonzero((lp != np.arange(128)).any(axis=1))[0]
    np.testing.assert_array_equal(changed, ad)
    assert 0 < (ad < 64).sum() < 64 and 0 < (ad >= 64).sum() < 64
    assert GT._commit_steps(recs, 0) == [3, X.NEAR128_COMMIT_AT]
    assert (ft.Pt.cpu().numpy()[0].view(np.uint16) == np.arange(128)).all()


FLOATS = ("q", "vel", "ring_u", "posf", "dist")


def test_complete_graphs_equal_the_lossy_entry():
    """Reduction (b): sync6_complete beside acl_fleet_lossy_trial_batch on the
    same GPU, teacher-forced from the same q and vel each step. Every fleet
    array, flag, status and record bit for bit; u within 1e-5 and what derives
    from q within 1e-9 (the two control kernels sum in different orders); every
    table is q bit for bit and err2 is zero."""
    import torch
    cs = X.case("sync6_complete")
    bt = _batch([cs])
    fx, fl = _trial(bt), _trial(bt, own=False)
    keys = tuple(k for k in STATE if k not in FLOATS) + ("n_lost",)
    for s in range(cs.steps):
        if s in cs.force:
            _write_ts(fx, 0, commit=1, formation=1)
            _write_ts(fl, 0, commit=1, formation=1)
        fl.q.copy_(fx.q)
        fl.vel.copy_(fx.vel)
        q0 = fx.q.cpu().numpy()[0]
        hx, hl = fx.run(1, history=True), fl.run(1, history=True)
        a, b = _state(fx), _state(fl, keys + FLOATS)
        what = f"step {s}"
        for k in keys:
            np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{what}: {k}")
        for k in ("vflags", "ca", "P", "ctl", "state"):
            assert torch.equal(hx[k], hl[k]), f"{what}: {k}"
        np.testing.assert_allclose(hx["u"].cpu().numpy(), hl["u"].cpu().numpy(), rtol=U_RTOL,
                                   atol=U_RTOL, err_msg=what)
        for k in FLOATS:
            np.testing.assert_allclose(a[k], b[k], rtol=0, atol=Q_ATOL, err_msg=f"{what}: {k}")
        assert not hx["err2"].cpu().numpy().any(), what
        np.testing.assert_array_equal(_bits(a["loc_est"][0]),
                                      _bits(np.broadcast_to(q0, (6, 6, 3))), err_msg=what)
    x = fx.fleet_status()["estimates"][0]
    assert (x["rounds_run"], x["n_unknown"], x["max_age"]) == (cs.steps, 0, 0)
    assert np.sort(fx.adopt_step.cpu().numpy()[0]).tolist() == [18] * 6
    assert fx.fleet_status()["fleet"][0]["n_adopted"] == 12


def _flown(cases, steps, cuts, diag=True, poison=None):
    """The cases without their forced commits, as calls cut at `cuts`."""
    import torch
    ft = _trial(_batch(cases), diag=diag)
    if poison is not None:
        ft.xst.copy_(_t(poison.view(np.uint8).reshape(len(cases), -1), np.uint8))
    hs = []
    edges = [0] + list(cuts) + [steps]
    for a, b in zip(edges[:-1], edges[1:]):
        hs.append(ft.run(b - a, history=True))
    torch.cuda.synchronize()
    hist = {k: torch.cat([h[k] for h in hs]).cpu().numpy() for k in hs[0]}
    return _state(ft), hist


def test_chunks_equal_step_by_step():
    """ring13_two and ring13_one, 16 steps: one call, and calls cut at step 3
    (the commit the supervisor requested at step 2 is pending), 5 (between the
    rounds of steps 4 and 6), 6 (the auction of step 4 is open, bids in flight)
    and 12 (after the adoption), equal 16 calls of one step bit for bit: state,
    trackers, loc_Pt, xst, histories."""
    cases = [X.case("ring13_two"), X.case("ring13_one")]
    ref = _flown(cases, 16, range(1, 16))
    for cuts in ((), (3, 5, 6, 12)):
        got = _flown(cases, 16, cuts)
        for x, y in zip(ref, got):
            assert x.keys() == y.keys()
            for k in x:
                np.testing.assert_array_equal(_bits(x[k]), _bits(y[k]), err_msg=k)
    assert ref[1]["err2"].any() and _xst(ref[0]["xst"])["rounds_run"].tolist() == [8, 8]
    assert (ref[0]["adopt_step"] == 11).all() and (ref[0]["loc_Pt"] == ref[0]["Pt"]).all()


def test_diag_off_equals_diag_on_but_for_the_record():
    """Every array but the err2 fields equal bit for bit; with diag off the
    err2 fields of xst keep what the caller put there and no err2 history
    comes back; the integer fields are kept up to date."""
    from aclswarm_amd import _lib as L
    cases = [X.case("ring13_two"), X.case("ring13_two_loss")]
    poison = np.zeros(2, L.FLEET_EST_EPISODE_STATUS_DTYPE)
    for k, v in zip(XERR, (7.0, 8.0, 9.0)):
        poison[k] = v
    on, hon = _flown(cases, 14, (7,))
    off, hoff = _flown(cases, 14, (7,), diag=False, poison=poison)
    for k in on:
        if k != "xst":
            np.testing.assert_array_equal(_bits(on[k]), _bits(off[k]), err_msg=k)
    assert "err2" in hon and "err2" not in hoff
    for k in hoff:
        np.testing.assert_array_equal(_bits(hon[k]), _bits(hoff[k]), err_msg=k)
    a, b = _xst(on["xst"]), _xst(off["xst"])
    for k in XINT:
        assert a[k].tolist() == b[k].tolist(), k
    assert a["rounds_run"].tolist() == [7, 7]
    assert [b[k].tolist() for k in XERR] == [[7.0] * 2, [8.0] * 2, [9.0] * 2]
    assert a["err2_all"][0] > 0 and (on["loc_Pt"][0] != np.arange(13)).any()


def test_a_bad_swarm_and_a_finished_trial_are_untouched_between_good_ones():
    """A row that is no permutation (swarm 1) and a finished trial (swarm 2)
    between good swarms: no round, no tick; loc_stamp, loc_est, loc_round,
    loc_n_lost, loc_Pt and xst keep what they held, their err2 rows stay 0,
    and the good swarms equal a run without them."""
    import torch
    cs = X.case("ring13_two_loss")
    ft = _trial(_batch([cs] * 4))
    ft.Pt[1, 4, 9] = 2  # vehicle 4's own row names vehicle 2 twice
    _write_ts(ft, 2, done_step=0, state=9)  # TERMINATE
    rng = np.random.RandomState(3)
    new = LOC + ("xst",)
    for k in new:  # something to keep
        t = getattr(ft, k)
        t[1:3] = _t(rng.randint(1, 12, size=tuple(t.shape)), t.cpu().numpy().dtype)[1:3]
        if k == "loc_est":
            t[1:3] *= 0.125
    kept = {k: getattr(ft, k).clone() for k in new}
    before = _state(ft)
    h = ft.run(12, history=True)
    after = _state(ft)
    alone = _trial(_batch([cs]))
    ha = alone.run(12, history=True)
    ref = _state(alone)
    assert ft.fleet_status()["fleet"][1]["flags"] == 0x4
    assert ft.status()[2]["done_step"] == 0
    for b in (1, 2):
        for k in new:
            assert torch.equal(getattr(ft, k)[b], kept[k][b]), (b, k)
        for k in ("q", "vel", "Pt", "n_lost", "adopt_step", "ctl_on"):
            np.testing.assert_array_equal(_bits(after[k][b]), _bits(before[k][b]), err_msg=k)
        assert not h["err2"].cpu().numpy()[:, b].any()
    for k in h:  # the BAD_INPUT swarm writes no history row at all
        assert not h[k].cpu().numpy()[:, 1].any(), k
    for b in (0, 3):
        for k in XSTATE:
            if k != "fidx":  # (every swarm of the batch has its own copy of the formations)
                np.testing.assert_array_equal(_bits(after[k][b]), _bits(ref[k][0]), err_msg=k)
        for k in h:
            np.testing.assert_array_equal(_bits(h[k].cpu().numpy()[:, b]),
                                          _bits(ha[k].cpu().numpy()[:, 0]), err_msg=k)
    assert ft.fleet_status()["estimates"][0]["rounds_run"] == 6
    assert ft.loc_n_lost[0].sum().item() > 0


def test_a_trial_moves_between_the_two_entries():
    """Three steps on the own-estimate entry, three on
    acl_fleet_lossy_trial_batch, and so on, on one workspace of the new size,
    against the restatement doing the same. While the shared-snapshot entry
    flies, the trackers, xst and loc_Pt stand still: the adoption of step 11
    is made there and does not reach loc_Pt; the one of step 22 is not."""
    cases = [X.case("ring13_two"), X.case("ring13_one")]
    ft, oracles, recs, hists = _teacher_forced(cases, 26, own_at=lambda s: (s // 3) % 2 == 0)
    assert ft.ws.numel() == ft.workspace_bytes()
    assert 11 in _n_adopt(hists, 0) and (11 // 3) % 2 == 1
    assert (recs[13][0]["loc_rows"] == np.arange(13)).all()
    assert (recs[13][0]["Pt"] != np.arange(13)).any()
    # own steps 0-2, 6-8, 12-14, 18-20, 24-25: rounds at 0, 2, 6, 8, 12, 14, 18, 20, 24
    assert ft.fleet_status()["estimates"]["rounds_run"].tolist() == [9, 9]
    assert not any("err2" in h for s, h in enumerate(hists) if (s // 3) % 2)


def test_the_init_sets_the_new_arrays_and_the_workspace_tail():
    import torch
    from aclswarm_amd import _lib as L
    cs = X.case("ring13_two")
    ft = _trial(_batch([cs, cs]))
    lib = L.lib()
    assert ft.ws.numel() == lib.acl_fleet_est_trial_workspace_bytes(13, 2, ft.queue_cap, 1)
    tail = lib.acl_fleet_delay_trial_workspace_bytes(13, 2, ft.queue_cap, 1)
    assert tail < ft.ws.numel()
    ft.run(6)
    for k in LOC + ("xst",):
        getattr(ft, k).fill_(3)
    ft.ws.fill_(0x5A)
    x = ft._est_args(0)
    stream = ct.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    assert lib.acl_fleet_est_trial_init(ct.byref(x), 13, stream) == 0
    st = _state(ft)
    assert (st["loc_Pt"] == np.arange(13)).all() and (st["Pt"] == np.arange(13)).all()
    for k in ("loc_stamp", "loc_est", "loc_round", "loc_n_lost", "xst"):
        assert not st[k].any(), k
    assert not ft.ws.cpu().numpy()[tail:].any()  # the status arrays of the two entries
    assert (st["adopt_step"] == -1).all() and not st["ctl_on"].any()


def test_python_argument_errors():
    """The ValueErrors before anything runs, and the C entry's workspace check
    through engine."""
    import torch
    from aclswarm_amd import _lib as L
    from aclswarm_amd import engine
    import aclswarm_amd
    assert aclswarm_amd.FleetEstTrial is engine.FleetEstTrial
    cs = X.case("ring13_two")
    ft = _trial(_batch([cs]))

    def make(**kw):
        return engine.FleetEstTrial(ft.table, ft.fseq, ft.q, ft.vel, params=ft.tp, **kw)
    for bad in (0, -2, 1.5, True, None):
        with pytest.raises(ValueError, match="track_every"):
            make(track_every=bad)
    with pytest.raises(ValueError, match="loss_seed is given without loss"):
        make(loss_seed=3)
    with pytest.raises(ValueError, match="out of range"):
        make(latency=0)
    ok = make()  # latency None: 1 tick on every link; loss None: zeros, seed 0
    assert (ok.track_every, ok.diag, ok.max_latency) == (2, False, 1)
    assert (ok.latency == 1).all() and not ok.loss.any() and ok.loss_seed.tolist() == [0]
    h = ok.run(2, history=True)
    assert "err2" not in h and ok.ws.numel() == ok.workspace_bytes()
    assert set(ok.fleet_status()) == {"fleet", "ticks", "estimates"}
    assert ok.fleet_status()["estimates"]["rounds_run"][0] == 1
    ok.track_every = 0
    with pytest.raises(ValueError, match="track_every"):
        ok.run(1)
    ok.track_every = 2
    with pytest.raises(ValueError, match="steps"):
        ok.run(-1)
    full = ok.ws
    ok.ws = torch.zeros(L.lib().acl_fleet_delay_trial_workspace_bytes(13, 1, ok.queue_cap, 1),
                        dtype=torch.uint8, device=_dev())
    with pytest.raises(RuntimeError, match="acl_fleet_est_trial_workspace_bytes"):
        ok.run(1)
    ok.ws = full
    assert ok.step == 2
    ok.run(1)
    torch.cuda.synchronize()
    assert ok.fleet_status()["estimates"]["rounds_run"][0] == 2  # (steps 0 and 2)
