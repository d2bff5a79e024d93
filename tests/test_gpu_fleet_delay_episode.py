"""GPU parity of acl_fleet_delay_episode_batch (episodes on the message-level
auction with per-link latency) against the plain-Python restatement
tests/fleet_delay_episode_oracle.py.

Teacher-forced exactly as tests/test_gpu_fleet_episode.py (whose helpers and
tolerances these are): one control step per call; before step k the
restatement takes the GPU's q and vel, at START steps the GPU's Rt (bits
pinned to acl_vehicle_start_batch's); after it every fleet state and output
array, adopt_step, P, both status structs and the step's flags are bit-exact,
u within 1e-5 relative, CA flags exact, q / vel within 1e-9. Then: every link
at 1 tick against acl_fleet_episode_batch on the same GPU, chunked calls with
bids in flight at the boundaries, a swarm with a bad latency entry between
good ones, the argument errors. Same-n cases fly as the swarms of one launch."""
import ctypes as ct

import numpy as np
import pytest

import fleet_auction_cases as C
import fleet_auction_oracle as FO
import fleet_delay_episode_cases as D
from test_gpu_fleet_episode import (BAD, CLEAN, FLEET_KEYS, Q_ATOL, STATE, U_RTOL, _assert_same,
                                    _bits, _check_rt, _dev, _raised, _state, _t, _u16, _write_q)

pytestmark = pytest.mark.gpu


def _episode(cases, latency="case", max_latency=None, queue_cap=None):
    """The cases (one n, ticks_per_step, max_iter, set of episode parameters)
    as the swarms of one FleetEpisode. latency "case": the cases' matrices;
    None: the entry without latency; else handed on as it is."""
    from aclswarm_amd import _lib as L
    from aclswarm_amd import engine
    c0 = cases[0]
    assert all((c.n, c.T, c.max_iter, c.ep) == (c0.n, c0.T, c0.max_iter, c0.ep) for c in cases)
    T = engine.FormationTable.from_host([c.p for c in cases], [c.adj for c in cases],
                                        [c.gains for c in cases], device=_dev())
    ep = L.default_episode_params()
    ep.auction_every, ep.bufflen = c0.ep["auction_every"], c0.ep["bufflen"]
    if isinstance(latency, str):
        latency = _t(np.stack([c.lat for c in cases]), np.uint8)
        max_latency = max(c.max_lat for c in cases) if max_latency is None else max_latency
    fe = engine.FleetEpisode(T, _t(np.arange(len(cases)), np.int32),
                             _t(np.stack([c.q0 for c in cases]), np.float64),
                             _t(np.stack([c.vel0 for c in cases]), np.float64),
                             Pt=_u16(np.stack([c.Pt for c in cases])), params=ep,
                             queue_cap=queue_cap, max_iter=c0.max_iter, ticks_per_step=c0.T,
                             latency=latency, max_latency=max_latency)
    for b, c in enumerate(cases):
        for v in c.invalid0:
            fe.invalid[b, v] = 1
    return fe


def _teacher_forced(cases, steps):
    """Flies the cases step by step on the GPU and on the restatement.
    Returns (fe, oracles, records [step][swarm], histories [step] of numpy)."""
    fe = _episode(cases)
    every = cases[0].ep["auction_every"]
    oracles = [c.oracle() for c in cases]
    recs, hists = [], []
    for s in range(steps):
        _write_q(fe, cases, s)
        before = _state(fe)
        h = fe.run(1, history=True)
        got = _state(fe)
        h = {k: v.cpu().numpy()[0] for k, v in h.items()}
        h["P"] = h["P"].view(np.uint16)
        hists.append(h)
        st = fe.status()
        if s % every == 0:
            cmd = np.stack([o.auto_cmd() for o in oracles])
            _check_rt(fe, cmd, before["q"], before["Pt"], got["Rt"])
        row = []
        for b, o in enumerate(oracles):
            what = f"{cases[b].name} (swarm {b}) step {s}"
            o.q, o.vel = before["q"][b].copy(), before["vel"][b].copy()
            r = o.step(Rt=got["Rt"][b], sup=(h["u"][b], h["ca"][b]))
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
            assert {k: int(st["ticks"][k][b]) for k in r["status"]} == r["status"], what
            assert {k: int(st["fleet"][k][b]) for k in o.fst} == o.fst, what
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


def _consensus(hists, b):
    return {s: int(((h["vflags"][b] & FO.V_CONSENSUS) != 0).sum()) for s, h in enumerate(hists)
            if (h["vflags"][b] & FO.V_CONSENSUS).any()}


def test_parity_n13_draw_uniform5_and_stale():
    """ring13 under the draw, ring13 with every link at 5 ticks and stale13
    under the draw as the three swarms of one launch, 48 steps. The edges, on
    the GPU's own run: adoptions at steps 11 and 22; nobody adopts at 5 ticks,
    where the auto-auctions of steps 12 and 24 restart 13 open auctioneers
    with 9 and 10 publications in flight; stale13 adopts at step 47."""
    cases = [D.case("ring13_draw"), D.case("ring13_u5"), D.case("stale13_draw")]
    fe, oracles, recs, hists = _teacher_forced(cases, 48)
    r0 = _raised(hists, 0)
    assert {s: r0[s] for s in r0 if s < 30} == {0: [FO.V_STARTED], 11: [CLEAN],
                                                12: [FO.V_STARTED], 22: [CLEAN],
                                                24: [FO.V_STARTED]}
    assert all(v == [FO.V_STARTED] for v in _raised(hists, 1).values())
    for s, fly in ((12, 9), (24, 10)):
        before = recs[s][1]["before"]
        assert before["open"].all() and sum(before["inflight"]) == fly
    assert _raised(hists, 2) == {0: [FO.V_STARTED], 12: [FO.V_STARTED], 23: [BAD],
                                 36: [FO.V_STARTED], 47: [CLEAN]}
    st = fe.status()["fleet"]
    assert st[1]["n_adopted"] == 0 and st[1]["n_restarted"] == 39
    assert (st[2]["n_restarted"], st[2]["n_invalid"], st[2]["n_flushed"]) == (12, 13, 14)
    assert (fe.adopt_step.cpu().numpy()[2] == 47).all()


def test_parity_restart_with_start_bids_in_flight():
    """Every link at 8 ticks, 2 ticks per step, an auto-auction every 3 steps:
    13 / 26 / 35 publications in flight at the restarts of steps 3 / 6 / 9."""
    fe, oracles, recs, hists = _teacher_forced([D.case("restart13_u8")], 12)
    assert [sum(recs[s][0]["before"]["inflight"]) for s in (3, 6, 9)] == [13, 26, 35]
    f = fe.status()["fleet"][0]
    assert (f["n_started"], f["n_restarted"], f["n_consensus"], f["ticks_run"]) == (52, 39, 0, 24)
    assert fe.open.cpu().numpy().all()


def test_parity_rings12_components():
    fe, oracles, recs, hists = _teacher_forced([D.case("rings12_draw")], 26)
    assert _raised(hists, 0) == {0: [FO.V_STARTED], 10: [BAD], 12: [FO.V_STARTED], 22: [BAD],
                                 24: [FO.V_STARTED]}
    f = fe.status()["fleet"][0]
    assert (f["n_started"], f["n_restarted"], f["n_flushed"]) == (23, 5, 13)
    assert f["n_adopted"] == 0 and f["n_invalid"] == 12


def test_parity_ring65_second_wave():
    """n = 65, links at 1..4 ticks, max_iter 32: the second wave of the new
    loops with one live lane; consensus spread over steps 10-14."""
    cs = D.case("ring65_draw")
    fe, oracles, recs, hists = _teacher_forced([cs], cs.steps)
    assert _consensus(hists, 0) == D.RING65_CONSENSUS
    dt = fe.done_tick.cpu().numpy()
    assert (int(dt.min()), int(dt.max())) == D.RING65_DONE_TICK
    f = fe.status()["fleet"][0]
    assert (f["n_invalid"], f["n_adopted"], f["ticks_run"]) == (65, 0, D.RING65_TICKS)


def test_parity_odd_last128():
    """n = 128 (the fleet kernel's 16-wave instantiation), links at 1..3
    ticks: 128 consensus, all INVALID, per-vehicle rows from step 0."""
    cs = D.case("odd_last128_draw")
    fe, oracles, recs, hists = _teacher_forced([cs], 8)
    st = fe.status()
    f = st["fleet"][0]
    assert (f["n_consensus"], f["n_invalid"], f["n_adopted"]) == (128, 128, 0)
    assert st["episode"]["per_vehicle"][0] == 1 and all(row[0]["per_vehicle"] for row in recs)


def _flown(cases, steps, cuts, latency="case"):
    import torch
    fe = _episode(cases, latency=latency)
    hs = []
    edges = [0] + list(cuts) + [steps]
    assert all(s in edges for c in cases for s in c.q_at)
    for a, b in zip(edges[:-1], edges[1:]):
        _write_q(fe, cases, a)
        hs.append(fe.run(b - a, history=True))
    torch.cuda.synchronize()
    hist = {k: torch.cat([h[k] for h in hs]).cpu().numpy() for k in hs[0]}
    return _state(fe), hist


@pytest.mark.parametrize("names,steps,cuts", [
    (("ring13", "stale13"), 48, (12, 36)),
    (("ring13_t2",), 45, (37,)),
    (("ring65",), 45, ()),
    (("odd_last128", "odd_last128_col"), 8, (2,)),
])
def test_every_link_at_one_tick_equals_the_existing_entry(names, steps, cuts):
    """acl_fleet_delay_episode_batch with every link at 1 tick against
    acl_fleet_episode_batch on the same GPU: state, outputs, statuses and
    histories bit for bit (the workspaces are layouts of their own)."""
    cases = [D.case("ones", x) for x in names]
    with_lat = _flown(cases, steps, cuts)
    without = _flown(cases, steps, cuts, latency=None)
    _assert_same(with_lat, without)
    assert with_lat[0]["fst"].any()


@pytest.mark.parametrize("names,steps,cuts", [
    (("ring13_draw", "ring13_u5", "stale13_draw"), 48, ((12, 36), (5, 12, 13, 25, 36, 40))),
    (("restart13_u8",), 12, ((), (4, 7))),
    (("odd_last128_draw",), 8, ((), (5,))),
])
def test_chunks_equal_step_by_step(names, steps, cuts):
    """One call of k steps equals k calls of one step, bit for bit: state,
    histories, statuses. Bids are in flight at the boundaries: under the draw
    at nearly every step; at 8 ticks per link and 2 ticks per step at all."""
    cases = [D.case(x) for x in names]
    edges = sorted(set(range(1, steps)))
    ref = _flown(cases, steps, edges)
    for c in cuts:
        _assert_same(ref, _flown(cases, steps, c))


def test_bad_latency_swarm_is_untouched_between_good_ones():
    """Swarm 1 holds a 0 and swarm 3 max_lat + 1 off the diagonal:
    ACL_FLEET_BAD_INPUT, nothing of their state changes. Swarms 0, 2 and 4 fly
    as they do alone; a bad value on the diagonal is ignored."""
    import torch
    cs = D.case("ring13_draw")
    fe = _episode([cs] * 5)
    assert fe.max_latency == 5
    lat = np.stack([cs.lat] * 5)
    lat[1, 3, 7] = 0
    lat[3, 12, 0] = 6
    lat[0, 4, 4] = 0
    lat[4, 9, 9] = 200
    fe.latency.copy_(_t(lat, np.uint8))  # (the constructor refuses such entries)
    before = _state(fe)
    h = fe.run(14, history=True)
    after = _state(fe)
    st = fe.status()
    alone = _episode([cs])
    ha = alone.run(14, history=True)
    ref = _state(alone)
    for b in (1, 3):
        assert st["fleet"][b]["flags"] == 0x4
        assert tuple(st["fleet"][b])[1:] == (0,) * 7
        for k in STATE:
            if k not in ("fst", "_status"):
                np.testing.assert_array_equal(_bits(after[k][b]), _bits(before[k][b]), err_msg=k)
        for k in h:
            assert not h[k].cpu().numpy()[:, b].any(), k
    for b in (0, 2, 4):
        assert st["fleet"][b] == alone.status()["fleet"][0]
        for k in STATE:
            np.testing.assert_array_equal(_bits(after[k][b]), _bits(ref[k][0]), err_msg=k)
        for k in h:
            np.testing.assert_array_equal(_bits(h[k].cpu().numpy()[:, b]),
                                          _bits(ha[k].cpu().numpy()[:, 0]), err_msg=k)
    assert st["fleet"][0]["n_adopted"] == 13  # (step 11)
    # the repaired matrix: the next call flies the swarms
    fe.latency.copy_(_t(np.stack([cs.lat] * 5), np.uint8))
    fe.run(2)
    torch.cuda.synchronize()
    assert (fe.status()["fleet"]["flags"] == 0).all()
    assert not torch.equal(fe.q[1], _t(before["q"][1], np.float64))


def test_argument_errors_of_the_c_entry():
    from aclswarm_amd import _lib as L
    from aclswarm_amd import engine
    cs = D.case("ring13_draw")
    fe = _episode([cs])
    fe.run(1)
    F = fe.table.struct()
    lib = L.lib()

    def args():
        d = L.FleetDelayEpisodeArgs()
        a = d.base
        a.B, a.step0, a.steps, a.ticks_per_step = 1, 1, 1, 10
        a.max_iter, a.queue_cap = 0, fe.queue_cap
        for k in ("fidx", "q", "vel", "P", "adopt_step", "est", "ring_u", "ring_ca", "fst") + \
                fe.FLEET_KEYS:
            setattr(a, k, getattr(fe, k).data_ptr())
        a.status = fe._status.data_ptr()
        a.workspace, a.workspace_bytes = fe.ws.data_ptr(), fe.ws.numel()
        a.cntrl, a.safety, a.ep = fe.cntrl, fe.safety, fe.ep
        d.lat, d.max_lat = fe.latency.data_ptr(), fe.max_latency
        return d

    def err(d, F=F):
        assert lib.acl_fleet_delay_episode_batch(ct.byref(F), ct.byref(d), None) == 1
        msg = lib.acl_last_error()
        assert msg.startswith(b"acl_fleet_delay_episode_batch: ")
        return msg
    before = _state(fe)
    assert fe.ws.numel() == lib.acl_fleet_delay_episode_workspace_bytes(13, 1, fe.queue_cap, 5)
    assert fe.ws.numel() > lib.acl_fleet_episode_workspace_bytes(13, 1, fe.queue_cap)
    for bad in (0, 65):
        assert lib.acl_fleet_delay_episode_workspace_bytes(13, 1, fe.queue_cap, bad) == 0
    d = args()
    d.lat = None
    assert b"lat is NULL" in err(d)
    for bad in (0, 65, -1):
        d = args()
        d.max_lat = bad
        assert b"max_lat out of range [1, 64]" in err(d)
    d = args()
    d.base.workspace_bytes -= 1
    assert b"acl_fleet_delay_episode_workspace_bytes" in err(d)
    d = args()  # a workspace of the entry without latency is too small
    d.base.workspace_bytes = lib.acl_fleet_episode_workspace_bytes(13, 1, fe.queue_cap)
    assert b"workspace_bytes" in err(d)
    d = args()
    d.max_lat = 6  # (larger logs than the workspace holds)
    assert b"workspace_bytes" in err(d)
    # the base entry's checks
    d = args()
    d.base.ticks_per_step = 0
    assert b"ticks_per_step" in err(d)
    d = args()
    d.base.adopt_step = None
    assert b"NULL" in err(d)
    d = args()
    d.base.ep.auction_latency = 3
    assert b"auction_latency" in err(d)
    d = args()
    d.base.ep.assignment = 1
    assert b"assignment" in err(d)
    T129 = engine.FormationTable.from_host([np.zeros((129, 3))], [C.chord_ring(129)], None,
                                           device=_dev())
    assert b"n out of range [1, 128]" in err(args(), T129.struct())
    assert lib.acl_fleet_delay_episode_batch(ct.byref(F), None, None) == 1
    d = args()
    d.base.steps, d.lat = 0, None
    assert lib.acl_fleet_delay_episode_batch(ct.byref(F), ct.byref(d), None) == 0  # nothing to do
    _assert_same([before], [_state(fe)])  # nothing ran


def test_fleet_episode_latency_value_errors():
    """The ValueErrors of engine.FleetAuction's latency arguments, before
    anything runs."""
    import torch
    from aclswarm_amd import engine
    cs = D.case("ring13_draw")
    fe = _episode([cs])
    q, lat = fe.q, fe.latency

    def make(**kw):
        return engine.FleetEpisode(fe.table, fe.fidx, q, q, **kw)
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
    with pytest.raises(ValueError, match="must be an int"):
        make(latency=3, max_latency=4.0)
    ok = make(latency=3, max_latency=7)
    assert ok.max_latency == 7 and ok.latency.shape == (1, 13, 13) and (ok.latency == 3).all()
    ok.run(1)
    assert ok.workspace_bytes() == ok.ws.numel()
    assert make().latency is None and make().workspace_bytes() < ok.workspace_bytes()
