"""GPU parity of acl_fleet_delay_trial_batch (trials on the message-level
auction with per-link latency) against the plain-Python restatement
tests/fleet_delay_trial_oracle.py.

Teacher-forced exactly as tests/test_gpu_fleet_trial.py (whose helpers and
tolerances these are): one control step per call; before step k the
restatement takes the GPU's q and vel, at START steps the GPU's Rt (bits
pinned to acl_vehicle_start_batch's); after it every fleet state and output
array, adopt_step, ctl_on, P, fidx, the status structs and the step's flags
are bit-exact, u within 1e-5 relative, CA flags exact, q / vel within 1e-9; at
the end the records bit for bit. Then: every link at 1 tick against
acl_fleet_trial_batch on the same GPU, chunked calls with bids in flight at
the boundaries, bad latency matrices beside a bad row and a finished trial,
the argument errors. Same-shape cases fly as the swarms of one launch."""
import ctypes as ct

import numpy as np
import pytest

import fleet_auction_cases as C
import fleet_delay_trial_cases as D
import fleet_trial_cases as K
import fleet_trial_oracle as FT
import trial_oracle as T
from test_gpu_fleet_trial import (FLEET_KEYS, Q_ATOL, STATE, U_RTOL, _adoptions, _batch, _bits,
                                  _check_rt, _check_status, _commit_steps, _dev, _force_commit,
                                  _params, _state, _t, _u16)

pytestmark = pytest.mark.gpu


def _lat_batch(cases, fseq_extra=()):
    """test_gpu_fleet_trial._batch and the swarms' latency matrices (a further
    swarm takes the matrix of the case whose start it takes)."""
    bt = _batch(cases, fseq_extra)
    bt["lat"] = np.stack([c.lat for c in cases] + [c.lat for _, c in fseq_extra])
    bt["max_lat"] = max(c.max_lat for c in cases)
    return bt


def _trial(bt, latency="case"):
    """latency "case": the batch's matrices; None: the entry without latency."""
    from aclswarm_amd import engine
    c0 = bt["case"]
    p, adj, G = zip(*bt["forms"])
    Tb = engine.FormationTable.from_host(list(p), list(adj), list(G), device=_dev())
    kw = {}
    if latency is not None:
        kw = dict(latency=_t(bt["lat"], np.uint8), max_latency=bt["max_lat"])
    return engine.FleetTrial(Tb, _t(bt["fseq"], np.int32), _t(bt["q"], np.float64),
                             _t(bt["vel"], np.float64), params=_params(c0),
                             max_iter=c0.max_iter, ticks_per_step=c0.T, **kw)


def _oracles(bt):
    import fleet_delay_trial_oracle as DT
    c0 = bt["case"]
    return [DT.DelayFleetTrial(bt["fseq"][b], bt["forms"], bt["q"][b], bt["vel"][b], c0.tp,
                               bt["lat"][b], max_iter=c0.max_iter, ticks_per_step=c0.T)
            for b in range(len(bt["fseq"]))]


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


def _n_adopt(hists, b):
    return {s: len(v) for s, v in _adoptions(hists, b).items()}


def test_parity_interrupt6_ends_by_the_assignment_timeout():
    """n = 6 under the 1..5 draw: no auction fits its period of 62 ticks;
    every auto-auction restarts the six open auctioneers; TERMINATE through
    the assignment timeout, flown two steps past the trial's end."""
    cs = D.case("interrupt6_draw")
    ft, oracles, recs, hists = _teacher_forced(_lat_batch([cs]), 227)
    st, fl = ft.status()[0], ft.fleet_status()["fleet"][0]
    assert (st["state"], st["last_state"], st["done_step"]) == (T.TERMINATE, T.WAITING, 224)
    assert (fl["n_started"], fl["n_restarted"], fl["n_adopted"]) == (42, 36, 0)
    assert ft.n_thrown.cpu().numpy().sum() == 79 and not _adoptions(hists, 0)
    assert not ft.ctl_on.cpu().numpy().any()


def test_parity_interrupt13():
    """reassign(13) under the 1..5 draw: the second formation commits at step
    137 onto 13 open auctioneers with 28 queued bids, which the new
    formation's first auction throws away; COMPLETE."""
    cs = D.case("interrupt13_draw")
    ft, oracles, recs, hists = _teacher_forced(_lat_batch([cs]), 341)
    assert _n_adopt(hists, 0) == {62: 13, 178: 13} and _commit_steps(recs, 0) == [21, 137]
    before = recs[137][0]["before"]
    assert before["open"].all() and before["queued"].sum() == 28
    assert ft.n_thrown.cpu().numpy()[0].sum() == 28
    st = ft.status()[0]
    assert (st["state"], st["done_step"]) == (T.COMPLETE, 338)


def test_parity_chord_ring_ten_ticks_per_step():
    """Every 33 steps under draw seed 2: adoptions at steps 42 and 74."""
    cs = D.case("chord13_t10")
    ft, oracles, recs, hists = _teacher_forced(_lat_batch([cs]), 78)
    assert _n_adopt(hists, 0) == {42: 13, 74: 13}
    assert ft.fleet_status()["fleet"][0]["n_restarted"] == 0


def test_parity_two_ticks_per_step_and_forced_commits():
    """The chord ring at 2 ticks per step, every 80 steps, three swarms of one
    launch: the ring under the draw (adoptions at steps 87-89); the two
    formations with a commit forced at step 40 under the draw (14 publications
    in flight, adoptions at 106-109) and with every link at 5 ticks (9 in
    flight, adoptions at 127-128). fidx ends at the second formation."""
    a, b, c = range(3)
    bt = _lat_batch([D.case("chord13_t2"), D.case("commit13"), D.case("commit13", 5)])
    assert bt["max_lat"] == 5
    force = {D.COMMIT13_AT: lambda ft, oracles: [_force_commit(x)(ft, oracles) for x in (b, c)]}
    ft, oracles, recs, hists = _teacher_forced(bt, D.COMMIT13_STEPS, force=force)
    # (swarm a flies its one formation as both of the batch's two)
    assert {s: k for s, k in _n_adopt(hists, a).items() if s < 100} == {87: 1, 88: 6, 89: 6}
    assert _n_adopt(hists, b) == {106: 1, 107: 5, 108: 5, 109: 2}
    assert _n_adopt(hists, c) == {127: 9, 128: 4}
    for x, fly, queued in ((b, 14, 3), (c, 9, 4)):
        before = recs[D.COMMIT13_AT][x]["before"]
        assert recs[D.COMMIT13_AT][x]["committed"] and before["open"].all()
        assert sum(before["inflight"]) == fly and before["queued"].sum() == queued
        assert ft.n_thrown.cpu().numpy()[x].sum() == 22
    # (formations 0; 1, 2; 3, 4 of the batch's table)
    assert ft.fidx.cpu().numpy().tolist() == [0, 2, 4]
    assert [int(x) for x in ft.status()["per_vehicle"][[b, c]]] == [0, 0]


def test_parity_ring65_second_wave():
    """n = 65 under the 1..4 draw: adoptions over steps 56-59, per-vehicle
    rows in between."""
    cs = D.case("ring65_draw")
    ft, oracles, recs, hists = _teacher_forced(_lat_batch([cs]), 60)
    assert _n_adopt(hists, 0) == {56: 2, 57: 7, 58: 12, 59: 13}
    assert ft.status()[0]["per_vehicle"] == 1
    assert [s for s, row in enumerate(recs) if row[0]["per_vehicle"]] == [56, 57, 58, 59]


def test_parity_near128_and_interrupt128():
    """n = 128 under the 1..3 draw. near128: 36 vehicles adopt at steps 16-17,
    92 flag INVALID. interrupt128: the commit forced at step 7 finds 128 open
    auctioneers, 15 queued bids and 121 publications in flight."""
    a, b = 0, 1
    bt = _lat_batch([D.case("near128_draw"), D.case("interrupt128_draw")])
    ft, oracles, recs, hists = _teacher_forced(bt, 18, force={K.INTERRUPT128_AT: _force_commit(b)})
    assert _n_adopt(hists, a) == {16: 23, 17: 13}
    fl = ft.fleet_status()["fleet"]
    assert (fl[a]["n_adopted"], fl[a]["n_invalid"]) == (36, 92)
    assert ft.status()[a]["per_vehicle"] == 1
    before = recs[K.INTERRUPT128_AT][b]["before"]
    fly = np.array(before["inflight"])
    assert recs[K.INTERRUPT128_AT][b]["committed"] and before["open"].all()
    assert before["queued"].sum() == 15 and fly.sum() == 121
    assert fly[:64].any() and fly[64:].any()
    assert ft.fidx.cpu().numpy()[b] == 2  # the second formation of the second case


# ---- latency 1, chunks ----

def _flown(bt, edges, latency="case", force=None):
    import torch
    ft = _trial(bt, latency=latency)
    hs = []
    for x, y in zip(edges[:-1], edges[1:]):
        if force and x in force:
            force[x](ft)
        hs.append(ft.run(y - x, history=True))
    torch.cuda.synchronize()
    return _state(ft), {k: torch.cat([h[k] for h in hs]).cpu().numpy() for k in hs[0]}


def _gpu_commit(*swarms):
    """The forced commit on the GPU's status alone (no restatement flies)."""
    from test_gpu_fleet_trial import _write_ts

    def f(ft):
        for b in swarms:
            _write_ts(ft, b, commit=1, formation=1)
    return f


def _assert_same(ref, got, what=""):
    for x, y in zip(ref, got):
        assert x.keys() == y.keys()
        for k in x:
            np.testing.assert_array_equal(_bits(x[k]), _bits(y[k]), err_msg=f"{what}: {k}")


@pytest.mark.parametrize("names,edges,forced", [
    (("stagger13_t2",), (0, 80), None),
    (("interrupt13",), (0, 345), None),
    (("near128", "interrupt128"), (0, K.INTERRUPT128_AT, 18), 1),
])
def test_every_link_at_one_tick_equals_the_existing_entry(names, edges, forced):
    """acl_fleet_delay_trial_batch with every link at 1 tick against
    acl_fleet_trial_batch on the same GPU: state, outputs, statuses, records
    and histories bit for bit (the workspaces are layouts of their own)."""
    bt = _lat_batch([D.case("ones", x) for x in names])
    force = {K.INTERRUPT128_AT: _gpu_commit(forced)} if forced is not None else None
    with_lat = _flown(bt, edges, force=force)
    without = _flown(bt, edges, latency=None, force=force)
    _assert_same(with_lat, without)
    assert with_lat[0]["adopt_step"].max() > 0


def test_chunks_equal_step_by_step():
    """The forced-commit swarms (the draw, and every link at 5 ticks), 150
    steps: one call per side of the forced commit, and a split at the steps
    around the commit, an auto-auction and between two adoptions, equal the
    step-by-step run bit for bit. Publications are in flight at every one of
    these boundaries."""
    bt = _lat_batch([D.case("commit13"), D.case("commit13", 5)])
    force = {D.COMMIT13_AT: _gpu_commit(0, 1)}
    steps = D.COMMIT13_STEPS
    ref = _flown(bt, list(range(steps + 1)), force=force)
    assert set(ref[0]["adopt_step"].ravel().tolist()) == {106, 107, 108, 109, 127, 128}
    for edges in ([0, 40, steps], [0, 33, 40, 41, 45, 51, 108, 128, steps]):
        _assert_same(ref, _flown(bt, edges, force=force), str(edges))


# ---- BAD_INPUT, argument errors, ValueErrors ----

def test_bad_latency_a_bad_row_and_a_finished_trial_beside_good_swarms():
    """Six swarms of the chord ring, 40 steps into the first auction. Then
    swarm 1 gets a 0 and swarm 3 max_lat + 1 off the diagonal, swarm 4 a row
    that is no permutation; swarm 5 finished at step 0 (a formation outside the
    table). The flagged swarms are untouched byte for byte, the finished one
    stays finished, swarms 0 and 2 fly as they do alone (a bad value on the
    diagonal is ignored)."""
    import torch
    cs = D.case("chord13_t2")
    bt = _lat_batch([cs] * 5, fseq_extra=[((99,), cs)])
    ft = _trial(bt)
    ft.run(40)
    lat = bt["lat"].copy()
    lat[1, 3, 7] = 0
    lat[3, 12, 0] = 6
    lat[0, 4, 4] = 0
    lat[2, 9, 9] = 200
    ft.latency.copy_(_t(lat, np.uint8))  # (the constructor refuses such entries)
    rows = ft.Pt.cpu().numpy().view(np.uint16).copy()
    good = rows.copy()
    rows[4, 4, 9] = rows[4, 4, 2]  # vehicle 4's own row names a vehicle twice
    ft.Pt.copy_(_u16(rows))
    before = _state(ft)
    h = ft.run(6, history=True)
    after = _state(ft)
    fl = ft.fleet_status()["fleet"]
    assert fl["flags"].tolist() == [0, FT.BAD_INPUT, 0, FT.BAD_INPUT, FT.BAD_INPUT, 0]
    for b in (1, 3, 4, 5):
        # (the finished trial: what flies and the fleet; its supervisor is the base entry's)
        keys = STATE if b != 5 else ("q", "vel", "P", "fidx", "ctl_on", "adopt_step", "Rt") + \
            FLEET_KEYS
        for k in keys:
            if k not in ("fst", "_status"):
                np.testing.assert_array_equal(_bits(after[k][b]), _bits(before[k][b]),
                                              err_msg=f"swarm {b}: {k}")
        assert not h["vflags"].cpu().numpy()[:, b].any()
    for b in (1, 3, 4):
        assert not h["q"].cpu().numpy()[:, b].any()
    st = ft.status()
    assert (st[5]["state"], st[5]["done_step"]) == (T.TERMINATE, 0) and tuple(fl[5]) == (0,) * 8
    alone = _trial(_lat_batch([cs]))
    alone.run(46)
    ref = _state(alone)
    for b in (0, 2):
        for k in STATE:
            if k != "fidx":  # (swarm b flies the batch's b-th copy of the formation)
                np.testing.assert_array_equal(_bits(after[k][b]), _bits(ref[k][0]),
                                              err_msg=f"swarm {b}: {k}")
        assert after["fidx"][b] == b
    assert ref["open"][0].all()  # (inside the auction: 31 to 89)
    # repaired: the next call flies the swarms on
    ft.latency.copy_(_t(bt["lat"], np.uint8))
    ft.Pt.copy_(_u16(good))
    ft.run(2)
    torch.cuda.synchronize()
    assert ft.fleet_status()["fleet"]["flags"].tolist() == [0] * 6
    ticks = before["ts"].view(st.dtype).reshape(-1)["ticks"]
    # steps 40 .. 47 tick at 40, 42, 44 and 46; the flagged swarms missed all but the last
    assert ft.status()["ticks"].tolist()[:5] == [ticks[0] + 4, ticks[1] + 1, ticks[2] + 4,
                                                 ticks[3] + 1, ticks[4] + 1]


def test_argument_errors_of_the_c_entries():
    from aclswarm_amd import _lib as L
    from aclswarm_amd import engine
    cs = D.case("chord13_t2")
    ft = _trial(_lat_batch([cs]))
    ft.run(1)
    F = ft.table.struct()
    lib = L.lib()
    n, cap = 13, ft.queue_cap

    def err(d, F=F):
        assert lib.acl_fleet_delay_trial_batch(ct.byref(F), ct.byref(d), None) == 1
        msg = lib.acl_last_error()
        assert msg.startswith(b"acl_fleet_delay_trial_batch: ")
        return msg

    def err_init(d, n=n):
        assert lib.acl_fleet_delay_trial_init(ct.byref(d), n, None) == 1
        msg = lib.acl_last_error()
        assert msg.startswith(b"acl_fleet_delay_trial_init: ")
        return msg
    before = _state(ft)
    assert ft.ws.numel() == lib.acl_fleet_delay_trial_workspace_bytes(n, 1, cap, 5)
    assert ft.ws.numel() > lib.acl_fleet_trial_workspace_bytes(n, 1, cap)
    for bad in (0, 65):
        assert lib.acl_fleet_delay_trial_workspace_bytes(n, 1, cap, bad) == 0
    for e in (err, err_init):
        d = ft._args(1)
        d.lat = None
        assert b"lat is NULL" in e(d)
        for bad in (0, 65, -1):
            d = ft._args(1)
            d.max_lat = bad
            assert b"max_lat out of range [1, 64]" in e(d)
        d = ft._args(1)
        d.base.workspace_bytes -= 1
        assert b"acl_fleet_delay_trial_workspace_bytes" in e(d)
        d = ft._args(1)  # a workspace of the entry without latency is too small
        d.base.workspace_bytes = lib.acl_fleet_trial_workspace_bytes(n, 1, cap)
        assert b"workspace_bytes" in e(d)
        d = ft._args(1)
        d.max_lat = 6  # (larger logs than the workspace holds)
        assert b"workspace_bytes" in e(d)
        # the base entry's checks
        d = ft._args(1)
        d.base.ticks_per_step = 0
        assert b"ticks_per_step" in e(d)
        d = ft._args(1)
        d.base.queue_cap = 0
        assert b"queue_cap" in e(d)
        d = ft._args(1)
        d.base.adopt_step = None
        assert b"NULL" in e(d)
        d = ft._args(1)
        d.base.tp.ep.auction_latency = 3
        assert b"auction_latency" in e(d)
    T129 = engine.FormationTable.from_host([np.zeros((129, 3))], [C.chord_ring(129)], None,
                                           device=_dev())
    assert b"n out of range [1, 128]" in err(ft._args(1), T129.struct())
    assert b"n out of range [1, 128]" in err_init(ft._args(1), 129)
    assert lib.acl_fleet_delay_trial_batch(ct.byref(F), None, None) == 1
    assert lib.acl_fleet_delay_trial_init(None, n, None) == 1
    d = ft._args(0)
    d.base.fseq, d.lat = None, None
    assert lib.acl_fleet_delay_trial_batch(ct.byref(F), ct.byref(d), None) == 0  # steps = 0
    after = _state(ft)
    for k in before:
        np.testing.assert_array_equal(_bits(before[k]), _bits(after[k]), err_msg=k)  # nothing ran


def test_fleet_trial_latency_value_errors():
    """The ValueErrors of engine.FleetAuction's latency arguments, before
    anything is allocated."""
    import torch
    from aclswarm_amd import engine
    cs = D.case("chord13_t2")
    bt = _lat_batch([cs])
    ft = _trial(bt)
    q, fseq, lat = _t(bt["q"], np.float64), _t(bt["fseq"], np.int32), ft.latency

    def make(**kw):
        return engine.FleetTrial(ft.table, fseq, q, q, **kw)
    with pytest.raises(ValueError, match="max_latency is given without latency"):
        make(max_latency=4)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="out of range"):
            make(latency=bad)
    with pytest.raises(ValueError, match="latency must be a contiguous"):
        make(latency=lat.to(torch.int32))
    with pytest.raises(ValueError, match="latency must be a contiguous"):
        make(latency=lat[0])
    with pytest.raises(ValueError, match="latency must be a contiguous"):
        make(latency=lat.cpu())
    with pytest.raises(ValueError, match="max_latency = 4 must be at least"):
        make(latency=lat, max_latency=4)
    with pytest.raises(ValueError, match="max_latency = 65"):
        make(latency=3, max_latency=65)
    ok = make(latency=3, max_latency=7)
    assert ok.max_latency == 7 and ok.latency.shape == (1, 13, 13) and (ok.latency == 3).all()
    ok.run(1)
    assert ok.workspace_bytes() == ok.ws.numel() > make().workspace_bytes()
    assert make().latency is None
