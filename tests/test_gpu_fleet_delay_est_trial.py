"""GPU parity of acl_fleet_delay_est_trial_init / acl_fleet_delay_est_trial_batch
(the trials on own estimates with tables on real links, and the encounter
record) against the composed restatement tests/fleet_delay_est_trial_oracle.py.

The comparison is tests/test_gpu_fleet_est_trial.py's own, teacher-forced one
step per call (its _teacher_forced, with its bars: every integer and tracker
array, loc_Pt, xst, n_lost and the error record bit for bit, u within 1e-5
relative, CA flags exact, q / vel within 1e-9), flown on the new entry. Beside
it, with no tolerance: n_missed, the bytes of the publication log (n <= 13),
every step's encounter record and the accumulated one. Each step starts from
the restatement's state, so q and the tables are the oracle's bit for bit and
the record has nothing to be tolerant about.

Then the reduction to acl_fleet_est_trial_batch on the same GPU byte for byte,
chunked calls against step by step, a trial that moves in from
acl_fleet_est_trial_batch mid-flight, a latency above max_tlat and a bad fseq
between good swarms, the record without its history, and the Python surface."""
import functools

import numpy as np
import pytest

import fleet_delay_est_trial_cases as DK
import fleet_delay_est_trial_oracle as DXT
import fleet_delay_localize_cases as DC
import fleet_est_trial_cases as X
import fleet_est_trial_oracle as XT
import fleet_loss_oracle as LO
import test_gpu_fleet_est_trial as GE
from test_fleet_delay_est_trial import test_argument_errors_of_the_c_entries_without_gpu  # noqa: F401
from test_gpu_fleet_trial import _bits, _dev, _t, _u16, _write_ts

pytestmark = pytest.mark.gpu


def _links(cases):
    return dict(table_latency=_t(np.stack([c.tlat for c in cases]), np.uint8),
                max_table_latency=max(c.max_tlat for c in cases),
                feed_loss=_u16(np.stack([c.feed for c in cases])))


class _Patched:
    """While active, test_gpu_fleet_est_trial's _trial builds its FleetEstTrial
    with the cases' table links and the encounter record, and its _oracles
    builds DelayEstFleetTrials. links_at(step): whether that step flies on the
    new entry (else on acl_fleet_est_trial_batch)."""

    def __init__(self, cases, links_at=None, encounters=True, **kw):
        self.cases, self.links_at, self.enc = cases, links_at or (lambda s: True), encounters
        self.kw = kw or _links(cases)

    def __enter__(self):
        from aclswarm_amd import engine
        self.cls, self.ocls = engine.FleetEstTrial, XT.EstFleetTrial
        links_at, todo = self.links_at, list(self.cases)
        mx = max(c.max_tlat for c in self.cases)

        class Trial(self.cls):
            def run(self, steps, history=False, stream=None, own_estimates=True):
                return super().run(steps, history=history, stream=stream,
                                   own_estimates=own_estimates, table_links=links_at(self.step))

        class Oracle(DXT.DelayEstFleetTrial):
            def step(self, Rt=None, sup=None, own=True):
                return super().step(Rt=Rt, sup=sup, own=own, delayed=links_at(self.step_no))

        def oracle(*args, **kw):
            c = todo.pop(0)  # (built in the order of the swarms)
            return Oracle(*args, tlat=c.tlat, max_tlat=mx, feed_loss=c.feed, **kw)

        engine.FleetEstTrial = functools.partial(Trial, encounters=self.enc, **self.kw)
        XT.EstFleetTrial = oracle
        return self

    def __exit__(self, *exc):
        from aclswarm_amd import engine
        engine.FleetEstTrial, XT.EstFleetTrial = self.cls, self.ocls


def _trial(cases, **kw):
    with _Patched(cases, **kw):
        return GE._trial(GE._batch(cases))


def _enc_status(a):
    from aclswarm_amd import _lib as L
    return np.ascontiguousarray(a).view(L.FLEET_ENCOUNTER_STATUS_DTYPE).reshape(-1)


def _enc_steps(a):
    from aclswarm_amd import _lib as L
    return np.ascontiguousarray(a).view(L.FLEET_ENCOUNTER_STEP_DTYPE).reshape(a.shape[:-1])


def _step_record(e):
    """A restatement's step record as an acl_fleet_encounter_step_t (None: the
    untouched, zeroed row of a finished or skipped trial)."""
    from aclswarm_amd import _lib as L
    r = np.zeros((), L.FLEET_ENCOUNTER_STEP_DTYPE)
    if e is not None:
        r["sep2"], r["i"], r["j"] = e["sep2"], e["i"], e["j"]
        r["n_breach"], r["n_blind"], r["n_ghost"] = e["n_breach"], e["n_blind"], e["n_ghost"]
    return r


def _check_record(ft, oracles, what=""):
    """The accumulated record, n_missed and (n <= 13) the log, bit for bit."""
    got = ft.encounters()
    missed, log = ft.n_missed.cpu().numpy(), ft.loc_ws.cpu().numpy()
    per = log.size // len(oracles)
    for b, o in enumerate(oracles):
        w = f"{what} swarm {b}"
        st = got["status"][b]
        for k, v in o.enc.status.items():
            if k == "sep2_min":
                assert _bits(st[k]) == _bits(v), (w, k, st[k], v)
            else:
                assert int(st[k]) == int(v), (w, k, st[k], v)
        assert int(st["reserved"]) == 0, w
        np.testing.assert_array_equal(got["blind"][b], o.enc.blind, err_msg=w)
        np.testing.assert_array_equal(got["ghost"][b], o.enc.ghost, err_msg=w)
        np.testing.assert_array_equal(missed[b], o.trackers.n_missed, err_msg=w)
        if ft.n <= 13:
            exp = np.frombuffer(o.trackers.log_bytes(), np.uint8)
            assert exp.size == per, w
            np.testing.assert_array_equal(log[b * per:(b + 1) * per], exp, err_msg=f"{w}: log")
    return got


def _teacher_forced(cases, steps, links_at=None):
    """test_gpu_fleet_est_trial._teacher_forced on the new entry; then every
    step's encounter record and the accumulated state, with no tolerance."""
    at = links_at or (lambda s: True)
    with _Patched(cases, links_at=at):
        ft, oracles, recs, hists = GE._teacher_forced(cases, steps)
    for s, (row, h) in enumerate(zip(recs, hists)):
        assert ("enc" in h) == at(s)
        if not at(s):
            continue
        got = _enc_steps(h["enc"])
        for b, r in enumerate(row):
            exp = _step_record(r["enc"])
            assert got[b].tobytes() == exp.tobytes(), \
                f"{cases[b].name} (swarm {b}) step {s}: {got[b]} != {exp}"
    enc = _check_record(ft, oracles)
    return ft, oracles, recs, hists, enc


def test_parity_a_single_vehicle_has_no_pair():
    """n = 1: +inf, pair 0xFFFF, step -1, every count 0, at every step."""
    cs = DK.DelayEstTrialCase(X.case("single"), 1, 1)
    ft, oracles, recs, hists, enc = _teacher_forced([cs], cs.steps)
    st = enc["status"][0]
    assert np.isposinf(st["sep2_min"]) and (st["step"], st["i"], st["j"]) == (-1, 0xFFFF, 0xFFFF)
    h = _enc_steps(np.stack([h["enc"] for h in hists]))
    assert np.isposinf(h["sep2"]).all() and (h["i"] == 0xFFFF).all() and (h["j"] == 0xFFFF).all()
    assert ft.fleet_status()["estimates"][0]["rounds_run"] == 8


def test_parity_two_vehicles():
    cs = DK.case("pair2")
    ft, oracles, recs, hists, enc = _teacher_forced([cs], cs.steps)
    st = enc["status"][0]
    assert (st["i"], st["j"]) == (0, 1) and np.isfinite(st["sep2_min"])
    assert GE._n_adopt(hists, 0) != {}


def test_parity_n6_complete_graphs():
    """sync6_complete at track_every 1, latencies drawn in 0..1, across the
    forced commit of step 12."""
    cs = DK.DelayEstTrialCase(X.case("sync6_complete"), DC.tlat_draw(6, 950, 1), 1)
    ft, oracles, recs, hists, enc = _teacher_forced([cs], cs.steps)
    assert GE.GT._commit_steps(recs, 0) == [3, X.SYNC6_COMMIT_AT]
    assert ft.fleet_status()["estimates"][0]["rounds_run"] == cs.steps


def test_parity_rings12_two_components():
    cs = DK.DelayEstTrialCase(X.case("rings12_two"), DC.tlat_draw(12, 951, 2), 2)
    ft, oracles, recs, hists, enc = _teacher_forced([cs], cs.steps)
    assert ft.fleet_status()["estimates"][0]["n_unknown"] == 72
    assert enc["status"][0]["n_blind"] == 0  # nobody adopts: no controller runs


def test_parity_ring13_latencies_a_slow_swarm_and_dead_feeds():
    """ring13_two, B = 4, max_tlat 7: latencies drawn in 0..2 per swarm and a
    dead feed on vehicle 3 + b; swarm 3 with every link at 7 rounds. Across
    the forced commit of step 14: tables published under the first formation
    are delivered under the second."""
    cases = [DK.ring13_links(b, max_tlat=7) for b in range(3)]
    cases.append(DK.DelayEstTrialCase(X.case("ring13_two"), 7, 7, name="ring13_two_all7"))
    ft, oracles, recs, hists, enc = _teacher_forced(cases, 26)
    assert GE.GT._commit_steps(recs, 0) == [3, DK.RING13_COMMIT_AT]
    missed = ft.n_missed.cpu().numpy()
    assert [int(missed[b, 3 + b]) for b in range(3)] == [13] * 3 and not missed[3].any()
    x = ft.fleet_status()["estimates"]
    assert x["rounds_run"].tolist() == [13] * 4
    # every link at 7 rounds: after 13 rounds a vehicle knows its neighbours at most
    assert x["n_unknown"][3] > x["n_unknown"][:3].max()
    print("ring13 encounters:", enc["status"].tolist(), "adoptions:",
          [GE._n_adopt(hists, b) for b in range(4)], "n_unknown", x["n_unknown"].tolist())


def test_parity_ring13_under_loss():
    """One swarm under loss_matrices13(), and the thresholds 0 / 8192 / 0xFFFF
    on every link; drawn latencies and feed outages."""
    cases = DK.ring13_loss_swarms()
    ft, oracles, recs, hists, enc = _teacher_forced(cases, 20)
    lost = ft.loc_n_lost.cpu().numpy().sum(axis=1)
    assert lost[1] == 0 and lost[2] > 0 and lost[3] > lost[2]
    assert ft.n_missed.cpu().numpy().sum() > 0


@pytest.mark.parametrize("name", ["ring64_te2", "ring65_te2"])
def test_parity_the_lane_slot_boundary(name):
    """n = 64: the first slot exactly full; n = 65: one live lane in the second."""
    if name == "ring64_te2":
        cs = DK.case(name)
    else:
        feed = np.zeros(65, np.int64)
        feed[64] = LO.DEAD
        cs = DK.DelayEstTrialCase(X.case(name), DC.tlat_draw(65, 941, 2), 2, feed)
    ft, oracles, recs, hists, enc = _teacher_forced([cs], 6)
    n = cs.n
    assert ft.n_missed.cpu().numpy()[0, n - 1] == 3
    assert enc["status"][0]["j"] < n


def test_parity_near128_both_slots_full():
    """n = 128: vehicles stride the four waves, both slots of every lane; a
    strict subset adopts at steps 14 and 15 (their controllers run, the others'
    do not), the forced commit of step 17 stops them."""
    cs = DK.DelayEstTrialCase(X.case("near128_two"), DC.tlat_draw(128, 942, 2), 2)
    ft, oracles, recs, hists, enc = _teacher_forced([cs], cs.steps)
    on = [int(r[0]["ctl_on"].sum()) for r in recs]
    assert 0 < max(on) < 128 and on[-1] == 0
    print("near128 encounters:", enc["status"].tolist())


@pytest.mark.parametrize("name", ["crafted13", "crafted65"])
def test_parity_the_crafted_encounters(name):
    """Breaches, a tie between two pairs with bit-identical s2, blind and
    ghost pairs, and vehicles whose controller does not run."""
    cs = DK.case(name)
    _, fo, _ = DK.cpu_run(name)
    ft, oracles, recs, hists, enc = _teacher_forced([cs], cs.steps)
    st = enc["status"][0]
    assert st["n_breach"] > 0 and st["n_blind"] > 0 and st["n_ghost"] > 0
    h0 = _enc_steps(hists[0]["enc"])[0]
    assert (h0["sep2"], h0["i"], h0["j"]) == (0.25, 1, cs.n - 1)
    # (teacher-forced from the device's q: the free flight of the restatement
    # differs by last bits at most, its counts are the same)
    assert (st["n_breach"], st["n_blind"], st["n_ghost"]) == \
        tuple(fo.enc.status[k] for k in ("n_breach", "n_blind", "n_ghost"))


def _flown(ft, cuts, steps, commit_at=None):
    """(state, histories) of ft flown as calls cut at `cuts`. commit_at (one of
    the cuts): every swarm's commit is forced before that step."""
    import torch
    assert commit_at is None or commit_at in cuts
    hs = []
    edges = [0] + list(cuts) + [steps]
    for a, b in zip(edges[:-1], edges[1:]):
        if a == commit_at:
            for s in range(ft.B):
                _write_ts(ft, s, commit=1, formation=1)
        hs.append(ft.run(b - a, history=True))
    torch.cuda.synchronize()
    st = GE._state(ft)
    if ft.loc_ws is not None:
        st["n_missed"], st["log"] = ft.n_missed.cpu().numpy(), ft.loc_ws.cpu().numpy()
    if ft.enc is not None:
        for k in ("enc", "enc_blind", "enc_ghost"):
            st[k] = getattr(ft, k).cpu().numpy()
    return st, {k: torch.cat([h[k] for h in hs]).cpu().numpy() for k in hs[0]}


def _equal(x, y, what=""):
    assert x.keys() == y.keys(), (x.keys(), y.keys())
    for k in x:
        np.testing.assert_array_equal(_bits(x[k]), _bits(y[k]), err_msg=f"{what}{k}")


@pytest.mark.parametrize("names,steps,cuts,commit_at",
                         [(("ring13_two", "ring13_two_loss"), 18, (7, 14), 14),
                          (("ring65_te2",), 6, (3,), None)])
def test_latency_zero_without_the_record_equals_the_est_trial_entry(names, steps, cuts,
                                                                    commit_at):
    """Reduction (b) on the same GPU, byte for byte over every output: every
    link at 0, no outage and enc NULL against acl_fleet_est_trial_batch, in
    several calls (n = 13: across the forced commit of step 14), the log
    workspace overwritten with 0xA5 after the init."""
    cases = [X.case(k) for k in names]
    old = GE._trial(GE._batch(cases))
    new = _trial([DK.DelayEstTrialCase(c, 0, 2) for c in cases], encounters=False,
                 table_latency=0, max_table_latency=2)
    assert new.table_latency is not None and old.table_latency is None and new.enc is None
    new.loc_ws.fill_(0xA5)
    a, ha = _flown(old, cuts, steps, commit_at)
    b, hb = _flown(new, cuts, steps, commit_at)
    assert not b.pop("n_missed").any() and (b.pop("log") != 0xA5).any()  # (the log is written)
    _equal(ha, hb, "history ")
    _equal(a, b)
    assert old.fleet_status()["estimates"]["rounds_run"].tolist() == [steps // 2] * len(cases)


def _ring13_batch():
    return [DK.ring13_links(b) for b in range(3)]


def _with_commit(ft, cuts, steps, at=DK.RING13_COMMIT_AT):
    """_flown with the forced commit of every swarm before step `at` (a cut)."""
    return _flown(ft, cuts, steps, commit_at=at)


def test_chunks_equal_step_by_step_across_a_commit():
    """Reduction (c): 24 steps of ring13_two under drawn latencies and dead
    feeds as one call per step, and as 5 + 9 + 10 and 14 + 10 (the commit is
    forced before step 14; the calls of 9 and 10 steps carry tables in flight
    across their boundary and across the commit): state, trackers, loc_Pt,
    xst, n_missed, the log, the record and the histories bit for bit."""
    cases = _ring13_batch()
    ref = _with_commit(_trial(cases), range(1, 24), 24)
    for cuts in ((5, 14), (14,)):
        got = _with_commit(_trial(cases), cuts, 24)
        for x, y in zip(ref, got):
            _equal(x, y)
    st = _enc_status(ref[0]["enc"])
    assert ref[0]["n_missed"].sum() > 0 and (st["step"] >= 0).all()
    assert _enc_steps(ref[1]["enc"])["n_ghost"].sum() > 0


def test_a_trial_moves_in_from_the_est_trial_entry_mid_flight():
    """Steps 0..8 on acl_fleet_est_trial_batch, the rest on the new entry, on
    one workspace, against the restatement doing the same: the log starts
    empty at step 9 (a table published under the other entry is not in it),
    the record begins there."""
    cases = [DK.ring13_links(0), DK.ring13_links(1)]
    ft, oracles, recs, hists, enc = _teacher_forced(cases, 18, links_at=lambda s: s >= 9)
    assert (enc["status"]["step"] >= 9).all()
    assert ft.fleet_status()["estimates"]["rounds_run"].tolist() == [9, 9]
    assert ft.n_missed.cpu().numpy()[0, 3] == 4  # rounds at steps 10, 12, 14, 16


def test_a_latency_above_max_tlat_and_a_bad_fseq_between_good_swarms():
    """Consequence (d): swarm 1 holds an off-diagonal latency of 3 at max_tlat
    2: ACL_FLEET_BAD_INPUT, skipped like a swarm with a bad row -- state,
    counters, record and log unchanged as bytes. Swarm 2's fseq names a
    formation outside the table: the trial ends at once (TERMINATE), as under
    every trial entry, and nothing of it moves either. Swarms 0 and 3 equal a
    run without them."""
    import torch
    cs = DK.ring13_links(0)
    ft = _trial([cs] * 4)
    ft.run(6)  # something in the log and the record
    ft.table_latency[1, 4, 9] = 3
    ft.fseq[2, 1] = 99
    keys = GE.XSTATE
    extra = ("n_missed", "loc_ws", "enc", "enc_blind", "enc_ghost")

    def snap():
        torch.cuda.synchronize()
        d = GE._state(ft, keys)
        d.update({k: getattr(ft, k).cpu().numpy() for k in extra})
        return d
    before = snap()
    h = ft.run(8, history=True)
    after = snap()
    per = before["loc_ws"].size // 4
    assert ft.fleet_status()["fleet"]["flags"].tolist() == [0, 0x4, 0, 0]
    assert ft.status()[2]["done_step"] == 6 and ft.status()[2]["state"] == 9
    # (of a trial that ends, the supervisor's own records move: what the
    # existing entries' tests compare for a finished trial, and all that is new)
    finished = ("q", "vel", "Pt", "n_lost", "adopt_step", "ctl_on") + GE.LOC + ("xst",) + extra
    for b in (1, 2):
        for k in (keys + extra if b == 1 else finished):
            x, y = (before[k], after[k])
            if k == "loc_ws":
                x, y = x[b * per:(b + 1) * per], y[b * per:(b + 1) * per]
            else:
                x, y = x[b], y[b]
            if k == "fst":  # (its first word is the verdict itself, asserted above)
                x, y = x[4:], y[4:]
            if k == "_status":  # (the ticks' own record of a refused swarm: the verdict again)
                assert y.tolist() == [0, 0, 0, 0x4]
                continue
            np.testing.assert_array_equal(_bits(x), _bits(y), err_msg=f"swarm {b}: {k}")
        assert not h["enc"].cpu().numpy()[:, b].any()
    for k in h:  # the BAD_INPUT swarm writes no history row at all
        assert not h[k].cpu().numpy()[:, 1].any(), k
    alone = _trial([cs])
    alone.run(6)
    ha = alone.run(8, history=True)
    torch.cuda.synchronize()
    ref = GE._state(alone, keys)
    ref.update({k: getattr(alone, k).cpu().numpy() for k in extra})
    for b in (0, 3):
        for k in keys + extra:
            if k == "fidx":
                continue  # (every swarm of the batch has its own copy of the formations)
            x = after[k][b * per:(b + 1) * per] if k == "loc_ws" else after[k][b]
            y = ref[k] if k == "loc_ws" else ref[k][0]
            np.testing.assert_array_equal(_bits(x), _bits(y), err_msg=f"swarm {b}: {k}")
        for k in h:
            np.testing.assert_array_equal(_bits(h[k].cpu().numpy()[:, b]),
                                          _bits(ha[k].cpu().numpy()[:, 0]), err_msg=k)


def test_the_record_without_its_history():
    """enc given with enc_hist NULL: the same accumulated record."""
    import torch
    cs = DK.case("crafted13")
    a, b = _trial([cs]), _trial([cs])
    ha = a.run(cs.steps, history=True)
    assert b.run(cs.steps) is None
    torch.cuda.synchronize()
    for k in ("enc", "enc_blind", "enc_ghost", "q", "loc_est", "n_missed"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    st = a.encounters()["status"][0]
    assert st["n_blind"] > 0 and _enc_steps(ha["enc"].cpu().numpy())["n_blind"].sum() == \
        st["n_blind"]


def test_the_init_resets_the_log_the_counters_and_the_record():
    import ctypes as ct
    import torch
    from aclswarm_amd import _lib as L
    cs = DK.ring13_links(0)
    ft = _trial([cs, cs])
    ft.run(8)
    torch.cuda.synchronize()
    assert ft.loc_ws.any().item() and ft.n_missed.any().item()
    for k in ("enc", "enc_blind", "enc_ghost"):
        getattr(ft, k).fill_(3)
    y = ft._delay_est_args(0)
    stream = ct.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    assert L.lib().acl_fleet_delay_est_trial_init(ct.byref(y), 13, stream) == 0
    torch.cuda.synchronize()
    assert not ft.loc_ws.any().item() and not ft.n_missed.any().item()
    enc = ft.encounters()
    assert not enc["blind"].any() and not enc["ghost"].any()
    st = enc["status"]
    assert np.isposinf(st["sep2_min"]).all() and (st["step"] == -1).all()
    assert (st["i"] == 0xFFFF).all() and (st["j"] == 0xFFFF).all()
    assert not any(st[k].any() for k in ("n_breach", "n_blind", "n_ghost", "reserved"))
    assert (GE._state(ft)["loc_Pt"] == np.arange(13)).all() and not ft.loc_stamp.any().item()


def test_python_surface():
    from aclswarm_amd import engine
    cs = X.case("ring13_two")
    ft = GE._trial(GE._batch([cs]))

    def make(**kw):
        return engine.FleetEstTrial(ft.table, ft.fseq, ft.q, ft.vel, params=ft.tp, **kw)
    for kw in (dict(table_latency=8), dict(table_latency=-1), dict(table_latency=1.5),
               dict(table_latency=2, max_table_latency=1), dict(max_table_latency=8),
               dict(feed_loss=65536), dict(feed_loss=-1), dict(encounters=1),
               dict(table_latency=ft.latency[0])):
        with pytest.raises(ValueError):
            make(**kw)
    plain = make()
    assert plain.table_latency is None and plain.loc_ws is None and plain.enc is None
    assert set(plain.fleet_status()) == {"fleet", "ticks", "estimates"}
    with pytest.raises(ValueError, match="encounters"):
        plain.encounters()
    ok = make(encounters=True)  # alone: every table link at 0
    assert ok.max_table_latency == 0 and not ok.table_latency.any().item()
    h = ok.run(3, history=True)
    assert h["enc"].shape == (3, 1, 24) and "err2" not in h
    assert set(ok.fleet_status()) == {"fleet", "ticks", "estimates", "encounters"}
    e = ok.encounters()
    assert e["status"].shape == (1,) and e["blind"].shape == (1, 13)
    assert e["status"][0]["step"] == 0 and np.isfinite(e["status"][0]["sep2_min"])
    lk = make(table_latency=1, feed_loss=0xFFFF)
    assert lk.max_table_latency == 1 and lk.enc is None
    hl = lk.run(3, history=True)
    assert "enc" not in hl and lk.n_missed.cpu().numpy().tolist() == [[2] * 13]
    assert not lk.loc_stamp.any().item()
    assert "enc" not in ok.run(1, history=True, table_links=False)
