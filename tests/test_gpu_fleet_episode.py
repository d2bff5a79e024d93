"""GPU parity of acl_fleet_episode_batch (closed-loop episodes on the
message-level auction) against the plain-Python restatement
tests/fleet_episode_oracle.py.

Teacher-forced, one control step per call: before step k the restatement
takes the GPU's q and vel, at START steps the GPU's Rt (whose bits are pinned
to acl_vehicle_start_batch's); after it every fleet state and output array,
adopt_step, P, both status structs and the step's flags are bit-exact, and
the existing episode tolerances hold: u within 1e-5 relative, CA flags exact,
q / vel within 1e-9, the supervisor's flags exact from the recorded commands.
Then one call of all steps, and a split that cuts an auction in flight,
against the step-by-step run, bit for bit. Same-n cases fly as the swarms of
one launch."""
import ctypes as ct
import functools

import numpy as np
import pytest

import fleet_auction_cases as C
import fleet_auction_oracle as FO
import fleet_episode_cases as K

pytestmark = pytest.mark.gpu

U_RTOL = 1e-5  # as tests/test_gpu_episode.py
Q_ATOL = 1e-9

FLEET_KEYS = C.STATE_KEYS + ("queue_len",)
STATE = ("q", "vel", "P", "adopt_step", "est", "fst", "ring_u", "ring_ca", "_status", "Rt") + \
    FLEET_KEYS
CLEAN = FO.V_CONSENSUS | FO.V_ADOPTED
BAD = FO.V_CONSENSUS | FO.V_INVALID


def _dev():
    import torch
    return torch.device("cuda:0")


def _t(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dt)).to(_dev())


def _u16(a):
    return _t(np.ascontiguousarray(a, np.uint16).view(np.int16), np.int16)


def _episode(cases, queue_cap=None, fidx=None, Pt=None):
    """The cases (one n, one ticks_per_step, one set of episode parameters) as
    the swarms of one FleetEpisode."""
    from aclswarm_amd import _lib as L
    from aclswarm_amd import engine
    c0 = cases[0]
    assert all((c.n, c.T, c.max_iter, c.ep) == (c0.n, c0.T, c0.max_iter, c0.ep) for c in cases)
    T = engine.FormationTable.from_host([c.p for c in cases], [c.adj for c in cases],
                                        [c.gains for c in cases], device=_dev())
    ep = L.default_episode_params()
    ep.auction_every, ep.bufflen = c0.ep["auction_every"], c0.ep["bufflen"]
    fidx = np.arange(len(cases)) if fidx is None else fidx
    Pt = np.stack([c.Pt for c in cases]) if Pt is None else Pt
    fe = engine.FleetEpisode(T, _t(fidx, np.int32), _t(np.stack([c.q0 for c in cases]), np.float64),
                             _t(np.stack([c.vel0 for c in cases]), np.float64), Pt=_u16(Pt),
                             params=ep, queue_cap=queue_cap, max_iter=c0.max_iter,
                             ticks_per_step=c0.T)
    for b, c in enumerate(cases):
        for v in c.invalid0:
            fe.invalid[b, v] = 1
    return fe


def _write_q(fe, cases, s):
    """The snapshots the caller writes into q before step s."""
    for b, c in enumerate(cases):
        if s in c.q_at:
            fe.q[b] = _t(c.q_at[s], np.float64)


def _state(fe):
    import torch
    torch.cuda.synchronize()
    d = {k: getattr(fe, k).cpu().numpy() for k in STATE}
    d["Pt"] = d["Pt"].view(np.uint16).astype(np.int64)
    d["P"] = d["P"].view(np.uint16)
    return d


def _check_rt(fe, cmd, q, rows_before, Rt):
    """The Rt the step wrote for every started vehicle has the bits of
    engine.vehicle_start for the same row and snapshot
    (tests/test_gpu_fleet_auction.py::_check_rt)."""
    import torch
    from aclswarm_amd import engine
    bs, vs = np.nonzero(cmd == FO.START)
    if not len(bs):
        return
    out = engine.vehicle_start(fe.table, _t(fe.fidx.cpu().numpy()[bs], np.int32),
                               _t(vs, np.int32), _t(q, np.float64), _u16(rows_before[bs, vs]),
                               qidx=_t(bs, np.int32), want_bid=False)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(Rt[bs, vs].view(np.uint64),
                                  out["Rt"].cpu().numpy().view(np.uint64))
    assert not out["flags"].cpu().numpy().any()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize]) if a.dtype.kind == "f" else a


def _teacher_forced(cases, steps):
    """Flies the cases step by step on the GPU and on the restatement.
    Returns (fe, oracles, records [step][swarm], histories [step] of numpy)."""
    import torch
    fe = _episode(cases)
    B, n = len(cases), cases[0].n
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
            assert (e["n_auctions"], e["n_invalid"], e["n_skipped"], e["n_disagree"],
                    e["pending_step"], e["n_restarted"]) == (0,) * 6, what
        recs.append(row)
    return fe, oracles, recs, hists


def _raised(hists, b):
    return {s: sorted(set(int(x) for x in h["vflags"][b] if x)) for s, h in enumerate(hists)
            if h["vflags"][b].any()}


def _solve_P(fe, b, q, P_in):
    """acl_solve_batch's P_out of swarm b's formation from q with P_in."""
    import torch
    from aclswarm_amd import engine
    n = fe.n
    out = engine.solve(fe.table, fe.fidx[b:b + 1].clone(), _t(q[None], np.float64),
                       torch.zeros((1, n, 3), dtype=torch.float64, device=_dev()),
                       _u16(P_in[None]), do_control=False, early_exit=False)
    torch.cuda.synchronize()
    assert out["status"].cpu().numpy().view(np.uint32)[0, 0] & 0x3 == 0x3  # VALID | AGREE
    return out["P_out"].cpu().numpy().view(np.uint16)[0]


def test_parity_n13_clean_and_stale():
    """ring13 and stale13 as the two swarms of one launch, 48 steps: the
    clean ring adopts in step 7 and restarts at 12; the stale sequence stalls,
    restarts seeded with the stale START bids, flushes, then runs clean."""
    cases = [K.case("ring13"), K.case("stale13")]
    fe, oracles, recs, hists = _teacher_forced(cases, 48)
    # the edges, on the GPU's own run
    assert _raised(hists, 0) == {0: [FO.V_STARTED], 7: [CLEAN], 12: [FO.V_STARTED], 19: [CLEAN],
                                 24: [FO.V_STARTED], 31: [CLEAN], 36: [FO.V_STARTED],
                                 43: [CLEAN]}
    assert _raised(hists, 1) == {0: [FO.V_STARTED], 12: [FO.V_STARTED], 19: [BAD],
                                 36: [FO.V_STARTED], 43: [CLEAN]}
    st = fe.status()
    f = st["fleet"][1]
    assert (f["n_restarted"], f["n_invalid"], f["n_flushed"]) == (12, 13, 14)
    assert (f["n_started"], f["n_adopted"], f["ticks_run"]) == (38, 13, 11 + 78 + 78)
    assert st["fleet"][0]["n_restarted"] == 0 and st["fleet"][0]["n_adopted"] == 4 * 13
    assert (st["episode"]["per_vehicle"] == 0).all()
    assert (fe.adopt_step.cpu().numpy() == 43).all()
    assert (recs[24][1]["cmd"] == FO.FLUSH).all() and recs[1][1]["status"]["ticks_run"] == 1
    assert oracles[1].fleet.n_thrown.sum() > 0
    # ring13: the adopted tables are acl_solve_batch's from the q the auction started from
    P0 = np.arange(13, dtype=np.uint16)
    np.testing.assert_array_equal(hists[7]["P"][0], _solve_P(fe, 0, cases[0].q0, P0))
    np.testing.assert_array_equal(hists[19]["P"][0],
                                  _solve_P(fe, 0, hists[11]["q"][0], hists[11]["P"][0]))


def test_parity_ring13_two_ticks_per_step_mixed_rows():
    """Adoptions in steps 36, 37 and 38: the swarm flies mixed rows
    (per_vehicle = 1, the directed walk) for two steps and returns to one
    table."""
    fe, oracles, recs, hists = _teacher_forced([K.case("ring13_t2")], 45)
    assert _raised(hists, 0) == {0: [FO.V_STARTED], 36: [CLEAN], 37: [CLEAN], 38: [CLEAN]}
    assert [int((h["vflags"][0] & FO.V_ADOPTED != 0).sum()) for h in hists[36:39]] == [5, 4, 4]
    assert [s for s, row in enumerate(recs) if row[0]["per_vehicle"]] == [36, 37]
    assert sorted(set(fe.adopt_step.cpu().numpy().ravel().tolist())) == [36, 37, 38]
    assert fe.status()["episode"]["per_vehicle"][0] == 0


def test_parity_rings12_components():
    fe, oracles, recs, hists = _teacher_forced([K.case("rings12")], 26)
    assert _raised(hists, 0) == {0: [FO.V_STARTED], 4: [BAD], 12: [FO.V_STARTED], 16: [BAD],
                                 24: [FO.V_STARTED]}
    assert recs[12][0]["cmd"].tolist() == [FO.START] * 6 + [FO.FLUSH] * 6
    f = fe.status()["fleet"][0]
    assert (f["n_started"], f["n_restarted"], f["n_flushed"]) == (23, 5, 13)
    assert f["n_adopted"] == 0 and f["n_invalid"] == 12
    # step 24: the rings have swapped roles (ring A, invalid since step 16,
    # flushes; ring B starts)
    assert recs[24][0]["cmd"].tolist() == [FO.FLUSH] * 6 + [FO.START] * 6
    assert fe.open.cpu().numpy()[0].tolist() == [0] * 6 + [1] * 6


def test_parity_ring65_second_wave():
    """n = 65: the second wave of every new loop, the fleet kernel inside the
    step loop; adoptions spread over steps 36-38."""
    cs = K.case("ring65")
    fe, oracles, recs, hists = _teacher_forced([cs], 45)
    assert sorted(s for s, h in enumerate(hists) if (h["vflags"][0] & FO.V_ADOPTED).any()) == \
        [36, 37, 38]
    assert [s for s, row in enumerate(recs) if row[0]["per_vehicle"]] == [36, 37]
    dt = fe.done_tick.cpu().numpy()
    assert (dt.min(), dt.max()) == (365, 389)
    f = fe.status()["fleet"][0]
    assert f["n_adopted"] == 65 and f["ticks_run"] == 390
    np.testing.assert_array_equal(hists[38]["P"][0],
                                  _solve_P(fe, 0, cs.q0, np.arange(65, dtype=np.uint16)))


def test_parity_odd_last128_row_and_column():
    """n = 128 (the fleet kernel's 16-wave instantiation): only vehicle 127's
    row, or only the last two columns, differ from the identity, and the swarm
    must fly per-vehicle rows from step 0 -- u of the odd vehicles is the
    check of the uniformity test's last row and last columns."""
    cases = [K.case("odd_last128"), K.case("odd_last128_col")]
    fe, oracles, recs, hists = _teacher_forced(cases, 8)
    st = fe.status()
    assert (st["episode"]["per_vehicle"] == 1).all()
    assert all(row[b]["per_vehicle"] for row in recs for b in (0, 1))
    for b in (0, 1):
        f = st["fleet"][b]
        assert (f["ticks_run"], f["n_invalid"], f["n_adopted"]) == (48, 128, 0)
    np.testing.assert_array_equal(fe.Pt.cpu().numpy().view(np.uint16),
                                  np.stack([c.Pt for c in cases]))


@functools.lru_cache(maxsize=None)
def _stepwise(names, steps):
    """The step-by-step run the chunked runs are compared with: (final
    state, concatenated histories)."""
    import torch
    cases = [K.case(x) for x in names]
    fe = _episode(cases)
    hs = []
    for s in range(steps):
        _write_q(fe, cases, s)
        hs.append(fe.run(1, history=True))
    torch.cuda.synchronize()
    hist = {k: torch.cat([h[k] for h in hs]).cpu().numpy() for k in hs[0]}
    return _state(fe), hist


def _chunked(names, steps, cuts):
    import torch
    cases = [K.case(x) for x in names]
    fe = _episode(cases)
    hs = []
    edges = [0] + list(cuts) + [steps]
    assert all(s in edges for c in cases for s in c.q_at)
    for a, b in zip(edges[:-1], edges[1:]):
        _write_q(fe, cases, a)
        hs.append(fe.run(b - a, history=True))
    torch.cuda.synchronize()
    hist = {k: torch.cat([h[k] for h in hs]).cpu().numpy() for k in hs[0]}
    return _state(fe), hist


def _assert_same(a, b):
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for k in x:
            np.testing.assert_array_equal(_bits(x[k]), _bits(y[k]), err_msg=k)


@pytest.mark.parametrize("names,steps,cuts", [
    (("ring13", "stale13"), 48, ((12, 36), (5, 12, 15, 36, 40))),
    (("ring13_t2",), 45, ((), (37,))),
    (("odd_last128", "odd_last128_col"), 8, ((), (2,))),
])
def test_chunks_equal_step_by_step(names, steps, cuts):
    """One call of all steps (or, where the caller writes q between chunks,
    the longest chunks that allows) equals the step-by-step run bit for bit:
    state, histories, statuses. So does a split that cuts an auction in
    flight (steps 5, 15, 40 at n = 13; 37, between two adoptions, at two
    ticks per step; 2 at n = 128)."""
    ref = _stepwise(names, steps)
    for c in cuts:
        _assert_same(ref, _chunked(names, steps, c))


def test_bad_input_swarms_are_untouched_beside_healthy_ones():
    """fidx out of range (swarm 0) and a row that is no permutation (swarm 2):
    ACL_FLEET_BAD_INPUT, nothing of their state changes; swarms 1 and 3 fly as
    they do alone."""
    import torch
    cs = K.case("ring13")
    n = 13
    rows = np.stack([cs.Pt] * 4)
    rows[2, 4, 9] = 2  # vehicle 4's own row names vehicle 2 twice
    fe = _episode([cs] * 4, fidx=np.array([9, 1, 2, 3]))
    fe.Pt.copy_(_u16(rows))  # (the constructor refuses such rows: the caller's rewrite)
    before = _state(fe)
    h = fe.run(10, history=True)
    after = _state(fe)
    st = fe.status()
    alone = _episode([cs])
    ha = alone.run(10, history=True)
    ref = _state(alone)
    for b in (0, 2):
        assert st["fleet"][b]["flags"] == 0x4
        assert tuple(st["fleet"][b])[1:] == (0,) * 7
        for k in STATE:
            if k not in ("fst", "_status"):
                np.testing.assert_array_equal(_bits(after[k][b]), _bits(before[k][b]), err_msg=k)
        assert not h["vflags"].cpu().numpy()[:, b].any()
    for b in (1, 3):
        assert st["fleet"][b] == alone.status()["fleet"][0]
        for k in STATE:
            np.testing.assert_array_equal(_bits(after[k][b]), _bits(ref[k][0]), err_msg=k)
        for k in h:
            np.testing.assert_array_equal(_bits(h[k].cpu().numpy()[:, b]),
                                          _bits(ha[k].cpu().numpy()[:, 0]), err_msg=k)
    assert st["fleet"][1]["n_adopted"] == 13
    # repaired rows and fidx: the next call flies the swarms
    fe.Pt.copy_(_u16(np.stack([cs.Pt] * 4)))
    fe.fidx.copy_(_t(np.arange(4), np.int32))
    fe.run(2)
    torch.cuda.synchronize()
    st = fe.status()
    assert (st["fleet"]["flags"] == 0).all()
    assert (st["fleet"]["n_started"][[0, 2]] == 0).all()  # no auto-auction step in 10, 11
    assert not torch.equal(fe.q[0], _t(before["q"][0], np.float64))
    with pytest.raises(ValueError, match="permutation"):
        _episode([cs], Pt=rows[2:3])


def test_argument_errors_of_the_c_entry():
    from aclswarm_amd import _lib as L
    fe = _episode([K.case("ring13")])
    fe.run(1)
    F = fe.table.struct()
    lib = L.lib()

    def args():
        a = L.FleetEpisodeArgs()
        a.B, a.step0, a.steps, a.ticks_per_step = 1, 1, 1, 10
        a.max_iter, a.queue_cap = 0, fe.queue_cap
        for k in ("fidx", "q", "vel", "P", "adopt_step", "est", "ring_u", "ring_ca", "fst") + \
                fe.FLEET_KEYS:
            setattr(a, k, getattr(fe, k).data_ptr())
        a.status = fe._status.data_ptr()
        a.workspace, a.workspace_bytes = fe.ws.data_ptr(), fe.ws.numel()
        a.cntrl, a.safety, a.ep = fe.cntrl, fe.safety, fe.ep
        return a

    def err(a, F=F):
        assert lib.acl_fleet_episode_batch(ct.byref(F), ct.byref(a), None) == 1  # INVALID_ARG
        return lib.acl_last_error()
    before = _state(fe)
    a = args()
    a.ticks_per_step = 0
    assert b"ticks_per_step" in err(a)
    a = args()
    a.adopt_step = None
    assert b"NULL" in err(a)
    a = args()
    a.ep.auction_latency = 3
    assert b"auction_latency" in err(a)
    a.ep.auction_latency = 0  # (a.ep is fe.ep's copy: ctypes copies nested structures)
    a = args()
    a.ep.assignment = 1
    assert b"assignment" in err(a)
    a = args()
    a.workspace_bytes -= 1
    assert b"workspace_bytes" in err(a)
    import torch
    from aclswarm_amd import engine
    T129 = engine.FormationTable.from_host([np.zeros((129, 3))], [C.chord_ring(129)], None,
                                           device=_dev())
    assert b"n out of range [1, 128]" in err(args(), T129.struct())
    _assert_same([before], [_state(fe)])  # nothing ran
    assert fe.ep.auction_latency == 0 and fe.ep.assignment == 0


def test_overflow_with_a_small_queue_is_sticky():
    """queue_cap = 2 at n = 13: bids are dropped exactly as in the restatement
    with the same capacity, and ACL_FLEET_OVERFLOW stays set in the episode's
    status after steps that drop nothing."""
    cs = K.case("ring13")
    fe = _episode([cs], queue_cap=2)
    o = cs.oracle(queue_cap=2)
    seen = []
    for s in range(14):
        before = _state(fe)
        h = fe.run(1, history=True)
        got = _state(fe)
        o.q, o.vel = before["q"][0].copy(), before["vel"][0].copy()
        r = o.step(Rt=got["Rt"][0])
        st = fe.status()
        seen.append(bool(st["ticks"]["flags"][0] & FO.OVERFLOW))
        assert seen[-1] == bool(r["status"]["flags"] & FO.OVERFLOW)
        np.testing.assert_array_equal(h["vflags"].cpu().numpy()[0, 0], r["raised"])
        np.testing.assert_array_equal(got["queue_len"][0], o.fleet.queue_len())
        assert {k: int(st["fleet"][k][0]) for k in o.fst} == o.fst
    assert seen[0] and not seen[-1]  # dropped in step 0; the last step dropped nothing
    assert fe.status()["fleet"]["flags"][0] == FO.OVERFLOW
    assert (fe.vflags.cpu().numpy() & FO.V_OVERFLOW).any()
    assert (fe.queue_len.cpu().numpy() <= 2).all()
