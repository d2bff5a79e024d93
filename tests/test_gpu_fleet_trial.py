"""GPU parity of acl_fleet_trial_batch (trials on the message-level auction)
against the plain-Python restatement tests/fleet_trial_oracle.py.

Teacher-forced, one control step per call: before step k the restatement
takes the GPU's q and vel, at START steps the GPU's Rt (whose bits are pinned
to acl_vehicle_start_batch's); after it every fleet state and output array,
adopt_step, ctl_on, P, fidx, both status structs, the last call's fleet status
and the step's flags are bit-exact, and the project's tolerances hold: u
within 1e-5 relative, CA flags exact, q / vel within 1e-9, the supervisor's
tick re-derived from the GPU's recorded commands, flags and positions. At the
end the records (dist, time, time_avoidance, assignments) bit for bit. Then
chunked calls against the step-by-step run, the synchronous trial where the
two models must agree, BAD_INPUT rows, the argument errors. Same-shape cases
fly as the swarms of one launch."""
import ctypes as ct

import numpy as np
import pytest

import fleet_auction_cases as C
import fleet_auction_oracle as FO
import fleet_trial_cases as K
import fleet_trial_oracle as FT
import trial_cases as TC
import trial_oracle as T

pytestmark = pytest.mark.gpu

U_RTOL = 1e-5  # as tests/test_gpu_trial.py
Q_ATOL = 1e-9

FLEET_KEYS = C.STATE_KEYS + ("queue_len",)
STATE = ("q", "vel", "P", "fidx", "ts", "ctl_on", "ring_u", "ring_ca", "posf", "dist", "t_conv",
         "t_avoid", "n_assign", "adopt_step", "fst", "_status", "Rt") + FLEET_KEYS


def _dev():
    import torch
    return torch.device("cuda:0")


def _t(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dt)).to(_dev())


def _u16(a):
    return _t(np.ascontiguousarray(a, np.uint16).view(np.int16), np.int16)


def _batch(cases, fseq_extra=()):
    """The cases (one n, ticks_per_step, max_iter and set of parameters) side by
    side: one formation table, fseq [B][K] with K the longest sequence (a
    shorter one flies its last formation again). fseq_extra: further swarms
    (fseq row, case whose start it takes)."""
    c0 = cases[0]
    assert all((c.n, c.T, c.max_iter, c.tp_over, c.ep_over) ==
               (c0.n, c0.T, c0.max_iter, c0.tp_over, c0.ep_over) for c in cases)
    Kmax = max(len(c.fseq) for c in cases)
    forms, fseq, q = [], [], []
    for c in cases:
        f = list(len(forms) + c.fseq) + [len(forms) + c.fseq[-1]] * (Kmax - len(c.fseq))
        fseq.append(f)
        forms += c.forms
        q.append(c.q)
    for row, c in fseq_extra:
        fseq.append(list(row))
        q.append(c.q)
    return dict(forms=forms, fseq=np.asarray(fseq, np.int32), q=np.stack(q),
                vel=np.zeros_like(np.stack(q)), case=c0)


def _params(c0):
    from aclswarm_amd import _lib as L
    tp = L.default_trial_params()
    for k, v in c0.tp_over.items():
        setattr(tp, k, v)
    for k, v in c0.ep_over.items():
        setattr(tp.ep, k, v)
    return tp


def _trial(bt, queue_cap=None):
    from aclswarm_amd import engine
    c0 = bt["case"]
    p, adj, G = zip(*bt["forms"])
    Tb = engine.FormationTable.from_host(list(p), list(adj), list(G), device=_dev())
    return engine.FleetTrial(Tb, _t(bt["fseq"], np.int32), _t(bt["q"], np.float64),
                             _t(bt["vel"], np.float64), params=_params(c0), queue_cap=queue_cap,
                             max_iter=c0.max_iter, ticks_per_step=c0.T)


def _oracles(bt):
    c0 = bt["case"]
    return [FT.FleetTrial(bt["fseq"][b], bt["forms"], bt["q"][b], bt["vel"][b], c0.tp,
                          max_iter=c0.max_iter, ticks_per_step=c0.T)
            for b in range(len(bt["fseq"]))]


def _state(ft):
    import torch
    torch.cuda.synchronize()
    d = {k: getattr(ft, k).cpu().numpy() for k in STATE}
    d["Pt"] = d["Pt"].view(np.uint16).astype(np.int64)
    d["P"] = d["P"].view(np.uint16)
    return d


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize]) if a.dtype.kind == "f" else a


def _check_rt(ft, cmd, rows, fidx, q, Rt):
    """The Rt the step wrote for every started vehicle has the bits of
    engine.vehicle_start for the row it started under and the same snapshot."""
    import torch
    from aclswarm_amd import engine
    bs, vs = np.nonzero(cmd == FO.START)
    if not len(bs):
        return
    out = engine.vehicle_start(ft.table, _t(fidx[bs], np.int32), _t(vs, np.int32),
                               _t(q, np.float64), _u16(rows[bs, vs]), qidx=_t(bs, np.int32),
                               want_bid=False)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(Rt[bs, vs].view(np.uint64),
                                  out["Rt"].cpu().numpy().view(np.uint64))
    assert not out["flags"].cpu().numpy().any()


def _check_status(ts, o, what):
    s = o.sup
    want = dict(state=s.state, last_state=s.last_state, timer_ticks=s.timer_ticks,
                formation=s.formation, ticks=s.ticks, received=int(s.received),
                logging=int(s.logging), commit=int(s.commit), next_auction=o.t.next_auction,
                done_step=s.done_step, n_auctions=o.n_auctions, n_invalid=0, n_skipped=0,
                n_disagree=0, per_vehicle=o.per_vehicle,
                conv_len=len(s.buffers.get("converged_orig_vel", ())),
                grid_len=len(s.buffers.get("gridlocked_active_ca", ())))
    got = {k: int(ts[k]) for k in want}
    assert got == want, (what, got, want)


def _teacher_forced(bt, steps, force=None):
    """Flies the batch step by step on the GPU and on the restatement. force:
    {step: f(ft, oracles)} applied before that step. Returns (ft, oracles,
    records [step][swarm], histories [step] of numpy)."""
    from aclswarm_amd import _lib as L
    ft = _trial(bt)
    oracles = _oracles(bt)
    B, n = bt["q"].shape[:2]
    ident = np.tile(np.arange(n), (n, 1))
    recs, hists = [], []
    for s in range(steps):
        if force and s in force:
            force[s](ft, oracles)
        before = _state(ft)
        h = ft.run(1, history=True)
        got = _state(ft)
        h = {k: v.cpu().numpy()[0] for k, v in h.items()}
        h["P"] = h["P"].view(np.uint16)
        hists.append(h)
        ts = got["ts"].view(L.TRIAL_STATUS_DTYPE).reshape(-1)
        fs = got["fst"].view(L.FLEET_EPISODE_STATUS_DTYPE).reshape(-1)
        tk = got["_status"].view(L.FLEET_STATUS_DTYPE).reshape(-1)
        row, cmds, rows = [], np.zeros((B, n), np.uint8), before["Pt"].copy()
        for b, o in enumerate(oracles):
            what = f"swarm {b} step {s}"
            o.q, o.vel = before["q"][b].copy(), before["vel"][b].copy()
            r = o.step(Rt=got["Rt"][b], sup=(h["u"][b], h["ca"][b], h["q"][b]))
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
            assert {k: int(tk[k][b]) for k in r["status"]} == r["status"], what
            assert {k: int(fs[k][b]) for k in o.fst} == o.fst, what
            _check_status(ts[b], o, what)
            assert h["state"][b] == o.sup.state, what
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


def _write_ts(ft, b, **fields):
    """The caller's rewrite of swarm b's acl_trial_status_t between calls."""
    from aclswarm_amd import _lib as L
    ts = ft.ts.cpu().numpy().view(L.TRIAL_STATUS_DTYPE).reshape(-1).copy()
    for k, v in fields.items():
        ts[k][b] = v
    ft.ts.copy_(_t(ts.view(np.uint8).reshape(ft.ts.shape), np.uint8))


def _force_commit(b):
    def f(ft, oracles):
        _write_ts(ft, b, commit=1, formation=1)
        K.force_commit(oracles[b])
    return f


def _one_formation_left(b):
    """Swarm b starts as if its first formation were behind it: it flies the
    batch's last formation only."""
    def f(ft, oracles):
        _write_ts(ft, b, formation=0)
        oracles[b].sup.formation = 0
    return f


def _adoptions(hists, b):
    return {s: np.nonzero(h["vflags"][b] & FO.V_ADOPTED)[0].tolist() for s, h in enumerate(hists)
            if (h["vflags"][b] & FO.V_ADOPTED).any()}


def _commit_steps(recs, b):
    return [s for s, row in enumerate(recs) if row[b]["committed"]]


# ---- (a) .. (g) ----

def test_parity_n6_interrupt_reassign_finished_and_bad_formation():
    """(a) n = 6, two ticks per step, auction_every = 31, one launch:
    interrupt6; reassign(6); a swarm with one formation left to fly (K is the
    batch's, so its status starts with the first formation behind it), which
    COMPLETEs early and stays finished while the others fly; a swarm with a
    formation index outside the table, which TERMINATEs at step 0 and stays
    finished and untouched. The run goes past the end of every trial:
    finished trials stay as they are."""
    a, b, c, d = range(4)
    i6 = K.case("interrupt6")
    re6 = K._from_trial("reassign6", TC.reassign(6), 0, 2, auction_every=31)
    one6 = K._from_trial("calm6", TC.calm(6), 0, 2, auction_every=31)
    bt = _batch([i6, re6, one6], fseq_extra=[((0, 99), i6)])
    steps = 290
    ft, oracles, recs, hists = _teacher_forced(bt, steps, force={0: _one_formation_left(c)})
    st = ft.status()
    assert st[c]["done_step"] + 100 < st[a]["done_step"]
    assert ft.records()["assignments"][c].tolist() == [0, 1]
    # interrupt6: the second formation commits onto open auctioneers with queued bids
    second = _commit_steps(recs, a)[1]
    assert recs[second][a]["before"]["open"].sum() >= 1
    assert recs[second][a]["before"]["queued"].sum() >= 1
    assert ft.n_thrown.cpu().numpy()[a].sum() > recs[second - 1][a]["n_thrown"].sum()
    for x in (a, b, c):
        assert (st[x]["state"], st[x]["last_state"]) == (T.COMPLETE, T.HOVERING)
        assert 0 < st[x]["done_step"] < steps - 1
    assert (st[d]["state"], st[d]["last_state"], st[d]["done_step"]) == (T.TERMINATE, T.HOVERING, 0)
    assert ft.fidx.cpu().numpy()[d] == 0
    fl = ft.fleet_status()["fleet"]
    assert tuple(fl[d]) == (0,) * 8 and not any(h["vflags"][d].any() for h in hists)
    np.testing.assert_array_equal(ft.q.cpu().numpy()[d], bt["q"][d])
    assert fl[a]["n_restarted"] > 0


def test_parity_interrupt13():
    """(b) reassign(13), auction_every = 33: as interrupt6, a wave's worth of
    vehicles; the auctions change vehicle 0's table after the second commit."""
    bt = _batch([K.case("interrupt13")])
    ft, oracles, recs, hists = _teacher_forced(bt, 345)
    second = _commit_steps(recs, 0)[1]
    assert recs[second][0]["before"]["open"].sum() >= 1
    assert recs[second][0]["before"]["queued"].sum() >= 1
    assert ft.n_thrown.cpu().numpy()[0].sum() > recs[second - 1][0]["n_thrown"].sum()
    assert ft.status()[0]["state"] == T.COMPLETE


def test_parity_restart13():
    """(c) every auto-auction restarts the auction in flight; nobody adopts;
    WAITING_ON_ASSIGNMENT -> TERMINATE."""
    bt = _batch([K.case("restart13")])
    ft, oracles, recs, hists = _teacher_forced(bt, 230)
    st, fl = ft.status()[0], ft.fleet_status()["fleet"][0]
    assert (st["state"], st["last_state"]) == (T.TERMINATE, T.WAITING)
    assert fl["n_restarted"] == fl["n_started"] - 13 > 0 and fl["n_adopted"] == 0
    assert not ft.ctl_on.cpu().numpy().any() and not _adoptions(hists, 0)


def test_parity_stagger13_two_ticks_per_step():
    """(d) controllers start over three steps; vehicle 0 is in the last group
    and the supervisor leaves WAITING_ON_ASSIGNMENT for it."""
    bt = _batch([K.case("stagger13_t2")])
    ft, oracles, recs, hists = _teacher_forced(bt, 80)
    ad = _adoptions(hists, 0)
    assert len(ad) >= 2 and 0 not in ad[min(ad)]
    s0 = next(s for s, v in ad.items() if 0 in v)
    flying = TC.first_step([h["state"][0] for h in hists], T.FLYING)
    assert s0 <= flying <= s0 + 1
    assert all(h["state"][0] == T.WAITING for h in hists[min(ad):flying])
    assert 0 < hists[min(ad)]["ctl"][0].sum() < 13
    assert ft.records()["assignments"][0].tolist() == [1]


def test_parity_rings12_invalid():
    """(e) INVALID and FLUSH alternate, no controller starts, TERMINATE."""
    bt = _batch([K.case("rings12_invalid")])
    ft, oracles, recs, hists = _teacher_forced(bt, 230)
    st, fl = ft.status()[0], ft.fleet_status()["fleet"][0]
    assert (st["state"], st["last_state"]) == (T.TERMINATE, T.WAITING)
    assert fl["n_invalid"] == fl["n_flushed"] > 0 and fl["n_adopted"] == 0
    assert not any(h["ctl"][0].any() for h in hists)


def test_parity_ring65_second_wave():
    """(f) n = 65: the second wave of every new kernel with one live lane;
    adoptions spread over several steps."""
    bt = _batch([K.case("ring65")])
    ft, oracles, recs, hists = _teacher_forced(bt, 50)
    ad = _adoptions(hists, 0)
    assert len(ad) >= 2 and sum(len(v) for v in ad.values()) == 65
    assert ft.status()[0]["state"] == T.FLYING




def test_parity_near128_and_interrupt128():
    """(g) n = 128, both task slots of every lane. near128: the vehicles near
    the chords adopt (0 and 127 among them), the others flag INVALID, the swarm
    flies per-vehicle rows, FLYING follows. interrupt128: a commit forced after
    three steps of the first auction, onto open auctioneers, queued bids and
    bids in flight."""
    a, b = 0, 1
    bt = _batch([K.case("near128"), K.case("interrupt128")])
    ft, oracles, recs, hists = _teacher_forced(bt, 18, force={K.INTERRUPT128_AT: _force_commit(b)})
    ad = sorted(sum(_adoptions(hists, a).values(), []))
    assert 0 in ad and 127 in ad and len(ad) < 128
    fl = ft.fleet_status()["fleet"]
    assert fl[a]["n_invalid"] == 128 - len(ad)
    st = ft.status()
    assert st[a]["per_vehicle"] == 1 and st[a]["state"] == T.FLYING
    before = recs[K.INTERRUPT128_AT][b]["before"]
    fly = np.array(before["inflight"])
    assert recs[K.INTERRUPT128_AT][b]["committed"] and before["open"].all()
    assert before["queued"].sum() >= 1 and fly[:64].any() and fly[64:].any()
    assert ft.fidx.cpu().numpy()[b] == 2  # the second formation of the second case


# ---- chunks ----

def _flown(name, edges):
    import torch
    bt = _batch([K.case(name)])
    ft = _trial(bt)
    hs = []
    for x, y in zip(edges[:-1], edges[1:]):
        hs.append(ft.run(y - x, history=True))
    torch.cuda.synchronize()
    return _state(ft), {k: torch.cat([h[k] for h in hs]).cpu().numpy() for k in hs[0]}


def test_chunks_equal_step_by_step():
    """stagger13_t2, 80 steps: one call, a split inside the auction (step 50:
    the auction runs from 31 to 69) and a split right before the commit step
    (21) equal the step-by-step run bit for bit: state, histories, statuses."""
    steps = 80
    ref = _flown("stagger13_t2", list(range(steps + 1)))
    for edges in ([0, steps], [0, 50, 68, steps], [0, 21, steps]):
        got = _flown("stagger13_t2", edges)
        for x, y in zip(ref, got):
            assert x.keys() == y.keys()
            for k in x:
                np.testing.assert_array_equal(_bits(x[k]), _bits(y[k]), err_msg=f"{edges}: {k}")


# ---- the synchronous trial ----

def test_sync6_equals_trial_on_the_gpu():
    """ticks_per_step = 60 holds one clean auction of six vehicles: FleetTrial
    and Trial fly the same swarms through the same supervisor states, step by
    step, to the same records. Both run the same control kernels on the same
    tables, so a difference points at the new code."""
    import torch
    from aclswarm_amd import engine
    bt = _batch([K.case("sync6_two"), K.case("sync6_reassign")])
    ft = _trial(bt)
    tr = engine.Trial(ft.table, ft.fseq, _t(bt["q"], np.float64), _t(bt["vel"], np.float64),
                      params=_params(bt["case"]))
    steps = 200
    hf, ht = ft.run(steps, history=True), tr.run(steps, history=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(hf["state"].cpu().numpy(), ht["state"].cpu().numpy())
    np.testing.assert_array_equal(hf["ctl"].cpu().numpy(), ht["ctl"].cpu().numpy())
    np.testing.assert_array_equal(hf["P"].cpu().numpy(), ht["P"].cpu().numpy())
    rf, rt = ft.records(), tr.records()
    assert (rf["state"] == T.COMPLETE).all()
    for k in rf:
        np.testing.assert_array_equal(_bits(rf[k]), _bits(rt[k]), err_msg=k)
    assert (ft.status()["n_auctions"] == tr.status()["n_auctions"]).all()


# ---- BAD_INPUT, argument errors, ValueErrors ----

def test_a_row_that_is_no_permutation_leaves_the_swarm_untouched():
    import torch
    cs = K.case("stagger13_t2")
    bt = _batch([cs, cs])
    ft = _trial(bt)
    ft.run(40)  # inside the first auction
    rows = ft.Pt.cpu().numpy().view(np.uint16).copy()
    good = rows.copy()
    rows[1, 4, 9] = rows[1, 4, 2]  # vehicle 4's own row names a vehicle twice
    ft.Pt.copy_(_u16(rows))
    before = _state(ft)
    h = ft.run(6, history=True)
    after = _state(ft)
    assert ft.fleet_status()["fleet"]["flags"].tolist() == [0, FT.BAD_INPUT]
    for k in STATE:
        if k not in ("fst", "_status"):
            np.testing.assert_array_equal(_bits(after[k][1]), _bits(before[k][1]), err_msg=k)
    assert not h["vflags"].cpu().numpy()[:, 1].any() and not h["q"].cpu().numpy()[:, 1].any()
    alone = _trial(_batch([cs]))
    alone.run(46)
    ref = _state(alone)
    for k in STATE:
        np.testing.assert_array_equal(_bits(after[k][0]), _bits(ref[k][0]), err_msg=k)
    # the repaired rows: the next call flies the swarm on
    ft.Pt.copy_(_u16(good))
    ft.run(2)
    torch.cuda.synchronize()
    assert ft.fleet_status()["fleet"]["flags"].tolist() == [0, 0]
    ticks = before["ts"].view(ft.status().dtype).reshape(-1)["ticks"]
    # steps 40 .. 47 tick at 40, 42, 44 and 46; the flagged swarm missed all but the last
    assert ft.status()["ticks"].tolist() == [ticks[0] + 4, ticks[1] + 1]


def test_argument_errors_of_the_c_entry():
    from aclswarm_amd import _lib as L
    from aclswarm_amd import engine
    ft = _trial(_batch([K.case("stagger13_t2")]))
    ft.run(1)
    F = ft.table.struct()
    lib = L.lib()

    def err(a, F=F):
        assert lib.acl_fleet_trial_batch(ct.byref(F), ct.byref(a), None) == 1  # INVALID_ARG
        return lib.acl_last_error()
    before = _state(ft)
    a = ft._args(1)
    a.ticks_per_step = 0
    assert b"ticks_per_step" in err(a)
    a = ft._args(1)
    a.queue_cap = 0
    assert b"queue_cap" in err(a)
    a = ft._args(1)
    a.adopt_step = None
    assert b"NULL" in err(a)
    a = ft._args(1)
    a.tp.ep.auction_latency = 3
    assert b"auction_latency" in err(a)
    a = ft._args(1)
    a.tp.ep.assignment = 1
    assert b"assignment" in err(a)
    a = ft._args(1)
    a.workspace_bytes -= 1
    assert b"workspace_bytes" in err(a)
    T129 = engine.FormationTable.from_host([np.zeros((129, 3))], [C.chord_ring(129)], None,
                                           device=_dev())
    assert b"n out of range [1, 128]" in err(ft._args(1), T129.struct())
    a = ft._args(0)
    a.fseq = None
    assert lib.acl_fleet_trial_batch(ct.byref(F), ct.byref(a), None) == 0  # steps = 0
    after = _state(ft)
    for k in before:
        np.testing.assert_array_equal(_bits(before[k]), _bits(after[k]), err_msg=k)  # nothing ran
    assert ft.tp.ep.auction_latency == 0 and ft.tp.ep.assignment == 0


def test_fleet_trial_value_errors_on_the_gpu():
    import torch
    from aclswarm_amd import engine
    bt = _batch([K.case("stagger13_t2")])
    ft = _trial(bt)
    q = _t(bt["q"], np.float64)
    fseq = _t(bt["fseq"], np.int32)
    with pytest.raises(ValueError, match="fseq"):
        engine.FleetTrial(ft.table, fseq.cpu(), q, q)                  # one device
    with pytest.raises(ValueError, match="vel"):
        engine.FleetTrial(ft.table, fseq, q, q.to(torch.float32))      # dtype
    with pytest.raises(ValueError, match="q must be"):
        engine.FleetTrial(ft.table, fseq, q[0], q)                     # shape
    with pytest.raises(ValueError, match="ticks_per_step"):
        engine.FleetTrial(ft.table, fseq, q, q, ticks_per_step=0)
    with pytest.raises(ValueError, match="steps"):
        ft.run(-1)
    assert ft.workspace_bytes() == ft.ws.numel()
