"""GPU parity of acl_fleet_est_episode_batch (the closed loop on each vehicle's
own estimates) against the plain-Python restatement
tests/fleet_est_episode_oracle.py.

Teacher-forced exactly as tests/test_gpu_fleet_loss_episode.py (whose helpers
and tolerances these are): one control step per call; before step k the
restatement takes the GPU's q and vel, at START steps the GPU's Rt (bits pinned
to acl_vehicle_start_batch's on the B n tables); after it every fleet state
and output array, adopt_step, P, the status structs, the step's flags, n_lost,
the trackers (loc_stamp, loc_est, loc_round, loc_n_lost), xst and the error
record are bit-exact, u within 1e-5 relative, CA flags exact, q / vel within
1e-9. Then: the complete-graph reduction against acl_fleet_lossy_episode_batch
on the same GPU, chunked calls, diag off against on, BAD_INPUT swarms between
good ones, an episode that moves between the two entries, the argument errors.

track_every is an argument of the call, not of a swarm: ring13 at track_every
1, 2 and 3 are three launches; the three ring13 cases at track_every 2 (loss 0,
64, 4096) fly as the swarms of one."""
import numpy as np
import pytest

import fleet_auction_cases as C
import fleet_auction_oracle as FO
import fleet_est_episode_cases as X
import test_gpu_fleet_est as GX
from test_gpu_fleet_episode import (CLEAN, FLEET_KEYS, Q_ATOL, STATE, U_RTOL, _bits, _check_rt,
                                    _dev, _raised, _t, _u16, _write_q)

pytestmark = pytest.mark.gpu

LOC = ("loc_stamp", "loc_est", "loc_round", "loc_n_lost")
XSTATE = STATE + ("n_lost", "xst") + LOC
XINT = ("rounds_run", "n_unknown", "max_age", "flags")
XERR = ("err2_own", "err2_nbr", "err2_all")


def _episode(cases, diag=True, track_every=None, own=True):
    """The cases (one n, ticks_per_step, max_iter, track_every, set of episode
    parameters) as the swarms of one FleetEstEpisode; own False: of one
    FleetEpisode on acl_fleet_lossy_episode_batch."""
    from aclswarm_amd import _lib as L
    from aclswarm_amd import engine
    c0 = cases[0]
    assert all((c.n, c.T, c.max_iter, c.ep, c.track_every) ==
               (c0.n, c0.T, c0.max_iter, c0.ep, c0.track_every) for c in cases)
    T = engine.FormationTable.from_host([c.p for c in cases], [c.adj for c in cases],
                                        [c.gains for c in cases], device=_dev())
    ep = L.default_episode_params()
    ep.auction_every, ep.bufflen = c0.ep["auction_every"], c0.ep["bufflen"]
    kw = dict(Pt=_u16(np.stack([c.Pt for c in cases])), params=ep, max_iter=c0.max_iter,
              ticks_per_step=c0.T, latency=_t(np.stack([c.lat for c in cases]), np.uint8),
              max_latency=max(c.max_lat for c in cases),
              loss=_u16(np.stack([c.loss for c in cases])),
              loss_seed=_t(np.array([c.seed for c in cases], np.uint32).view(np.int32), np.int32))
    if own:
        kw.update(track_every=c0.track_every if track_every is None else track_every, diag=diag)
    cls = engine.FleetEstEpisode if own else engine.FleetEpisode
    fe = cls(T, _t(np.arange(len(cases)), np.int32),
             _t(np.stack([c.q0 for c in cases]), np.float64),
             _t(np.stack([c.vel0 for c in cases]), np.float64), **kw)
    for b, c in enumerate(cases):
        for v in c.invalid0:
            fe.invalid[b, v] = 1
    return fe


def _state(fe, keys=XSTATE):
    import torch
    torch.cuda.synchronize()
    d = {k: getattr(fe, k).cpu().numpy() for k in keys}
    d["Pt"] = d["Pt"].view(np.uint16).astype(np.int64)
    d["P"] = d["P"].view(np.uint16)
    return d


def _xst(a):
    from aclswarm_amd import _lib as L
    return np.ascontiguousarray(a).view(L.FLEET_EST_EPISODE_STATUS_DTYPE).reshape(-1)


def _teacher_forced(cases, steps, own_at=lambda s: True):
    """Flies the cases step by step on the GPU and on the restatement; step s
    on the own-estimate entry when own_at(s), else on the lossy entry.
    Returns (fe, oracles, records [step][swarm], histories [step] of numpy)."""
    fe = _episode(cases)
    every = cases[0].ep["auction_every"]
    oracles = [c.oracle() for c in cases]
    recs, hists = [], []
    for s in range(steps):
        own = own_at(s)
        _write_q(fe, cases, s)
        before = _state(fe)
        h = fe.run(1, history=True, own_estimates=own)
        got = _state(fe)
        h = {k: v.cpu().numpy()[0] for k, v in h.items()}
        h["P"] = h["P"].view(np.uint16)
        hists.append(h)
        st = fe.status()
        assert ("err2" in h) == own
        if s % every == 0:
            cmd = np.stack([o.auto_cmd() for o in oracles])
            if own:  # the tables of this step: nothing after the round writes them
                assert GX._check_rt(fe, cmd, got["loc_est"], before["Pt"], got["Rt"]) == \
                    int((cmd == FO.START).sum())
            else:
                _check_rt(fe, cmd, before["q"], before["Pt"], got["Rt"])
        row = []
        for b, o in enumerate(oracles):
            what = f"{cases[b].name} (swarm {b}) step {s}"
            o.q, o.vel = before["q"][b].copy(), before["vel"][b].copy()
            r = o.step(Rt=got["Rt"][b], sup=(h["u"][b], h["ca"][b]), own=own)
            row.append(r)
            exp = C.snapshot_state(o.fleet)
            for k in FLEET_KEYS:
                np.testing.assert_array_equal(_bits(got[k][b]),
                                              _bits(np.asarray(exp[k], got[k].dtype)),
                                              err_msg=f"{what}: {k}")
            np.testing.assert_array_equal(got["adopt_step"][b], o.adopt_step, err_msg=what)
            np.testing.assert_array_equal(got["P"][b], o.P, err_msg=what)
            np.testing.assert_array_equal(h["P"][b], o.P, err_msg=what)
            np.testing.assert_array_equal(h["vflags"][b], r["raised"], err_msg=what)
            np.testing.assert_array_equal(got["n_lost"][b], o.fleet.n_lost, err_msg=what)
            assert {k: int(st["ticks"][k][b]) for k in r["status"]} == r["status"], what
            assert {k: int(st["fleet"][k][b]) for k in o.fst} == o.fst, what
            # the trackers and the record
            tr = o.trackers
            np.testing.assert_array_equal(got["loc_stamp"][b], tr.stamps(), err_msg=what)
            np.testing.assert_array_equal(_bits(got["loc_est"][b]), _bits(tr.est()), err_msg=what)
            assert got["loc_round"][b] == tr.round, what
            np.testing.assert_array_equal(got["loc_n_lost"][b], tr.n_lost, err_msg=what)
            x = st["estimates"][b]
            assert {k: int(x[k]) for k in XINT} == {k: o.xst[k] for k in XINT}, what
            np.testing.assert_array_equal(_bits(np.array([x[k] for k in XERR])),
                                          _bits(np.array([o.xst[k] for k in XERR])), err_msg=what)
            if own:
                np.testing.assert_array_equal(_bits(h["err2"][b]), _bits(np.array(r["err2"])),
                                              err_msg=what)
            # the commands and the flight
            np.testing.assert_allclose(h["u"][b], r["u"], rtol=U_RTOL, atol=U_RTOL, err_msg=what)
            np.testing.assert_array_equal(h["ca"][b], r["ca"], err_msg=what)
            np.testing.assert_allclose(got["q"][b], o.q, rtol=0, atol=Q_ATOL, err_msg=what)
            np.testing.assert_allclose(got["vel"][b], o.vel, rtol=0, atol=Q_ATOL, err_msg=what)
            np.testing.assert_array_equal(h["q"][b], got["q"][b], err_msg=what)
            np.testing.assert_array_equal(h["vel"][b], got["vel"][b], err_msg=what)
            e = st["episode"][b]
            assert (e["converged_step"], e["gridlock_step"]) == \
                (o.converged_step, o.gridlock_step), what
            assert (e["converged"], e["gridlocked"]) == \
                (int(o.sup.converged), int(o.sup.gridlocked)), what
            assert (e["n_samples"], e["n_ca_steps"]) == (o.sup.n_samples, o.n_ca_steps), what
            assert e["per_vehicle"] == o.per_vehicle, what
        recs.append(row)
    return fe, oracles, recs, hists


def test_parity_a_single_vehicle():
    """n = 1: no edge, nobody to hear of; the error record is three zeros."""
    cs = X.case("single")
    fe, oracles, recs, hists = _teacher_forced([cs], cs.steps)
    x = fe.status()["estimates"][0]
    assert (x["rounds_run"], x["n_unknown"], x["max_age"]) == (6, 0, 0)
    assert all(not h["err2"].any() for h in hists)


@pytest.mark.parametrize("name", ["ring13_te1", "ring13_te3"])
def test_parity_ring13_track_every_1_and_3(name):
    """A round every step, and every third step (the adoption of step 7 flies
    rows whose new neighbours were never heard of: metres of error in
    err2_nbr). Adoptions at steps 7 and 19 on the GPU's own run."""
    cs = X.case(name)
    fe, oracles, recs, hists = _teacher_forced([cs], cs.steps)
    assert _raised(hists, 0) == {0: [FO.V_STARTED], 7: [CLEAN], 12: [FO.V_STARTED], 19: [CLEAN],
                                 24: [FO.V_STARTED]}
    x = fe.status()["estimates"][0]
    assert x["rounds_run"] == {"ring13_te1": 30, "ring13_te3": 10}[name]
    if name == "ring13_te1":
        assert 9.6e-3 < np.sqrt(max(x[k] for k in XERR)) < 9.8e-3 and x["err2_own"] == 0.0
    else:
        assert x["err2_own"] > 0.0 and x["err2_nbr"] > 1.0


def test_parity_ring13_track_every_2_without_and_under_loss():
    """ring13 at track_every 2 under loss 0, 64 and 4096 as the three swarms of
    one launch: tables and bids are lost under the same matrix and seed, and
    counted apart (under 4096: 30 tables, 15 bids)."""
    cases = [X.case("ring13_te2"), X.case("ring13_loss64"), X.case("ring13_loss4096")]
    fe, oracles, recs, hists = _teacher_forced(cases, 30)
    assert fe.loc_n_lost.cpu().numpy().sum(axis=1).tolist() == [0, 0, 30]
    assert fe.n_lost.cpu().numpy().sum(axis=1).tolist() == [0, 1, 15]
    assert _raised(hists, 0)[7] == [CLEAN]
    x = fe.status()["estimates"]
    assert x["rounds_run"].tolist() == [15, 15, 15]
    assert 18.6e-3 < np.sqrt(max(x[0][k] for k in XERR)) < 18.8e-3


def test_parity_rings12_split_graph():
    """Two components (the first mask word only): 72 entries unknown for the
    whole flight, phantoms at the origin."""
    cs = X.case("rings12_te2")
    fe, oracles, recs, hists = _teacher_forced([cs], cs.steps)
    assert fe.status()["estimates"][0]["n_unknown"] == 72
    assert fe.status()["episode"][0]["n_ca_steps"] == oracles[0].n_ca_steps > 0


def test_parity_ring65_second_wave():
    """n = 65: the second wave and the second mask word of the error kernel,
    the localize kernel's other wave count; 3 236 entries unknown after 6
    rounds."""
    cs = X.case("ring65_te2")
    fe, oracles, recs, hists = _teacher_forced([cs], cs.steps)
    x = fe.status()["estimates"][0]
    assert (x["rounds_run"], x["n_unknown"]) == (6, 3236) and x["err2_all"] > 0.0


def test_parity_odd_last128():
    """n = 128, rows that differ (per-vehicle rows from step 0), 4 steps."""
    cs = X.case("odd_last128_te2")
    fe, oracles, recs, hists = _teacher_forced([cs], cs.steps)
    assert fe.status()["episode"]["per_vehicle"][0] == 1
    assert fe.status()["estimates"][0]["rounds_run"] == 2


@pytest.mark.parametrize("name", ["ring6_complete", "ring13_complete"])
def test_complete_graph_equals_the_lossy_entry(name):
    """On a complete graph with a lossless round every step every table is q
    bit for bit: the entry against acl_fleet_lossy_episode_batch on the same
    GPU, teacher-forced from the same state each step. Every fleet array,
    history flag and status bit for bit; u within 1e-5 and q / vel within 1e-9
    (the two control kernels sum in different orders); err2 all zero."""
    import torch
    cs = X.case(name)
    fx, fl = _episode([cs]), _episode([cs], own=False)
    keys = tuple(k for k in STATE if k not in ("q", "vel", "ring_u")) + ("n_lost",)
    for s in range(cs.steps):
        fl.q.copy_(fx.q)
        fl.vel.copy_(fx.vel)
        q0 = fx.q.cpu().numpy()[0]
        hx, hl = fx.run(1, history=True), fl.run(1, history=True)
        a, b = _state(fx), _state(fl, keys + ("q", "vel", "ring_u"))
        what = f"{name} step {s}"
        for k in keys:
            np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{what}: {k}")
        for k in ("vflags", "ca", "P"):
            assert torch.equal(hx[k], hl[k]), f"{what}: {k}"
        np.testing.assert_allclose(hx["u"].cpu().numpy(), hl["u"].cpu().numpy(), rtol=U_RTOL,
                                   atol=U_RTOL, err_msg=what)
        for k in ("q", "vel"):
            np.testing.assert_allclose(a[k], b[k], rtol=0, atol=Q_ATOL, err_msg=what)
        assert not hx["err2"].cpu().numpy().any(), what
        np.testing.assert_array_equal(_bits(a["loc_est"][0]),
                                      _bits(np.broadcast_to(q0, (cs.n, cs.n, 3))), err_msg=what)
    x = fx.status()["estimates"][0]
    assert (x["rounds_run"], x["n_unknown"], x["max_age"]) == (cs.steps, 0, 0)
    assert fx.status()["fleet"][0]["n_adopted"] == fl.status()["fleet"][0]["n_adopted"]
    assert fx.status()["episode"][0]["n_ca_steps"] > 0


def _flown(cases, steps, cuts, diag=True, poison=None):
    import torch
    fe = _episode(cases, diag=diag)
    if poison is not None:
        fe.xst.copy_(_t(poison.view(np.uint8).reshape(len(cases), -1), np.uint8))
    hs = []
    edges = [0] + list(cuts) + [steps]
    for a, b in zip(edges[:-1], edges[1:]):
        hs.append(fe.run(b - a, history=True))
    torch.cuda.synchronize()
    hist = {k: torch.cat([h[k] for h in hs]).cpu().numpy() for k in hs[0]}
    return _state(fe), hist


def test_chunks_equal_step_by_step():
    """ring13 at track_every 3 (rounds at steps 0, 3, 6, ...), diag on: one
    call of 30 steps, and a split with a cut inside an auction (step 5: the
    auction of step 0 ends in step 7) and cuts between two rounds (13, 14),
    equal 30 calls of one step bit for bit: state, trackers, xst, histories."""
    cases = [X.case("ring13_te3"), X.case("ring13_te3")]
    ref = _flown(cases, 30, range(1, 30))
    for cuts in ((), (5, 13, 14, 25)):
        got = _flown(cases, 30, cuts)
        for x, y in zip(ref, got):
            assert x.keys() == y.keys()
            for k in x:
                np.testing.assert_array_equal(_bits(x[k]), _bits(y[k]), err_msg=k)
    assert ref[1]["err2"].any() and _xst(ref[0]["xst"])["rounds_run"].tolist() == [10, 10]


def test_diag_off_equals_diag_on_but_for_the_record():
    """Every array but the err2 fields equal bit for bit; with diag off the
    err2 fields of xst are untouched (they keep what the caller put there) and
    no err2 history comes back; the integer fields are kept up to date."""
    from aclswarm_amd import _lib as L
    cases = [X.case("ring13_te2"), X.case("ring13_loss4096")]
    poison = np.zeros(2, L.FLEET_EST_EPISODE_STATUS_DTYPE)
    for k, v in zip(XERR, (7.0, 8.0, 9.0)):
        poison[k] = v
    on, hon = _flown(cases, 16, (7,))
    off, hoff = _flown(cases, 16, (7,), diag=False, poison=poison)
    for k in on:
        if k != "xst":
            np.testing.assert_array_equal(_bits(on[k]), _bits(off[k]), err_msg=k)
    assert "err2" in hon and "err2" not in hoff
    for k in hoff:
        np.testing.assert_array_equal(_bits(hon[k]), _bits(hoff[k]), err_msg=k)
    a, b = _xst(on["xst"]), _xst(off["xst"])
    for k in XINT:
        assert a[k].tolist() == b[k].tolist(), k
    assert a["rounds_run"].tolist() == [8, 8]
    assert [b[k].tolist() for k in XERR] == [[7.0] * 2, [8.0] * 2, [9.0] * 2]
    assert (a["err2_all"] > 0).all()


def test_bad_input_swarms_are_untouched_between_good_ones():
    """A bad fidx (swarm 1), a row that is no permutation (swarm 2) and a bad
    latency entry (swarm 3) between good swarms: ACL_FLEET_BAD_INPUT, no round
    and no tick; loc_*, loc_n_lost and xst keep what they held, and the good
    swarms equal a run without them."""
    import torch
    cs = X.case("ring13_loss4096")
    fe = _episode([cs] * 5)
    fe.fidx[1] = 9
    fe.Pt[2, 4, 9] = 2  # vehicle 4's own row names vehicle 2 twice
    fe.latency[3, 12, 0] = 0
    rng = np.random.RandomState(3)
    for k in LOC + ("xst",):  # something to keep
        t = getattr(fe, k)
        t.copy_(_t(rng.randint(1, 100, size=tuple(t.shape)), t.cpu().numpy().dtype))
        if k == "loc_est":
            t.mul_(0.125)
    kept = {k: getattr(fe, k).clone() for k in LOC + ("xst",)}
    for b in (0, 4):  # the good swarms start from fresh trackers
        for k in LOC + ("xst",):
            getattr(fe, k)[b] = 0
    before = _state(fe)
    h = fe.run(14, history=True)
    after = _state(fe)
    st = fe.status()
    alone = _episode([cs])
    ha = alone.run(14, history=True)
    ref = _state(alone)
    for b in (1, 2, 3):
        assert st["fleet"][b]["flags"] == 0x4 and tuple(st["fleet"][b])[1:] == (0,) * 7
        for k in XSTATE:
            if k not in ("fst", "_status"):
                np.testing.assert_array_equal(_bits(after[k][b]), _bits(before[k][b]), err_msg=k)
        for k in LOC + ("xst",):
            assert torch.equal(getattr(fe, k)[b], kept[k][b]), k
        for k in h:
            assert not h[k].cpu().numpy()[:, b].any(), k
    for b in (0, 4):
        for k in XSTATE:
            np.testing.assert_array_equal(_bits(after[k][b]), _bits(ref[k][0]), err_msg=k)
        for k in h:
            np.testing.assert_array_equal(_bits(h[k].cpu().numpy()[:, b]),
                                          _bits(ha[k].cpu().numpy()[:, 0]), err_msg=k)
    assert st["estimates"][0]["rounds_run"] == 7 and fe.loc_n_lost[0].sum().item() > 0


def test_an_episode_moves_between_the_two_entries():
    """Three steps on the own-estimate entry, three on
    acl_fleet_lossy_episode_batch, and so on, on one workspace of the new
    size, against the restatement doing the same: while the shared-snapshot
    entry flies, the trackers and xst stand still (and age)."""
    cases = [X.case("ring13_loss64"), X.case("ring13_te2")]
    fe, oracles, recs, hists = _teacher_forced(cases, 24, own_at=lambda s: (s // 3) % 2 == 0)
    assert fe.ws.numel() == fe.workspace_bytes()
    x = fe.status()["estimates"]
    # own steps 0-2, 6-8, 12-14, 18-20: rounds at 0, 2, 6, 8, 12, 14, 18, 20
    assert x["rounds_run"].tolist() == [8, 8] and fe.loc_round.cpu().numpy().tolist() == [8, 8]
    assert fe.status()["fleet"]["n_adopted"].sum() > 0
    assert not any("err2" in h for s, h in enumerate(hists) if (s // 3) % 2)


def test_python_argument_errors():
    """The ValueErrors before anything runs, and the C entry's argument errors
    through engine."""
    import torch
    from aclswarm_amd import _lib as L
    from aclswarm_amd import engine
    cs = X.case("ring13_te2")
    fe = _episode([cs])

    def make(**kw):
        return engine.FleetEstEpisode(fe.table, fe.fidx, fe.q, fe.vel, **kw)
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
    for k in LOC + ("xst",):
        assert not getattr(ok, k).any()
    h = ok.run(2, history=True)
    assert "err2" not in h and ok.ws.numel() == ok.workspace_bytes()
    lib = L.lib()
    assert ok.workspace_bytes() == lib.acl_fleet_est_episode_workspace_bytes(13, 1, ok.queue_cap, 1)
    assert ok.workspace_bytes() > lib.acl_fleet_delay_episode_workspace_bytes(13, 1, ok.queue_cap, 1)
    assert set(ok.status()) == {"episode", "fleet", "ticks", "estimates"}
    assert ok.status()["estimates"]["rounds_run"][0] == 1
    ok.track_every = 0
    with pytest.raises(ValueError, match="track_every"):
        ok.run(1)
    ok.track_every = 2
    with pytest.raises(ValueError, match="steps"):
        ok.run(-1)
    # the C entry's own checks
    full = ok.ws
    ok.ws = torch.zeros(lib.acl_fleet_delay_episode_workspace_bytes(13, 1, ok.queue_cap, 1),
                        dtype=torch.uint8, device=_dev())
    with pytest.raises(RuntimeError, match="acl_fleet_est_episode_workspace_bytes"):
        ok.run(1)
    ok.ws = full
    ok.ticks_per_step = 0
    with pytest.raises(RuntimeError, match="ticks_per_step < 1"):
        ok.run(1)
    ok.ticks_per_step = 10
    ok.max_latency = 65
    with pytest.raises(RuntimeError, match="max_lat out of range"):
        ok.run(1)
    ok.max_latency = 1
    assert ok.step == 2
    ok.run(1)
    torch.cuda.synchronize()
    assert ok.status()["estimates"]["rounds_run"][0] == 2  # (steps 0 and 2)
