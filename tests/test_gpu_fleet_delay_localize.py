"""GPU parity of acl_fleet_delay_localize_batch (fleet localization with table
latency in whole rounds and outages of the own state feed) against the
plain-Python restatement tests/fleet_delay_localize_oracle.py.

Bar: everything bit for bit after every call -- stamp, est (as u64 bits),
round, n_lost, n_missed and the status records; at n <= 13 also the
publication log, byte for byte. The shapes are the smallest at which the
kernel can go wrong: n = 1, a non-multiple of anything (6, 12, 13), one slot
full (64), the second mask word (65) and the size limit (128); a log that
wraps, tables in flight across a call boundary, and the largest latency."""
import numpy as np
import pytest

import fleet_auction_cases as C
import fleet_delay_localize_cases as DC
import fleet_delay_localize_oracle as DG
import fleet_localize_cases as GC
import fleet_localize_oracle as GO
import fleet_loss_cases as LC
import fleet_loss_oracle as LO
import helpers as H
import test_gpu_fleet_auction as G
import test_gpu_fleet_localize as TL

pytestmark = pytest.mark.gpu


def _loc(adjs, Pts=None, fidx=None, loss=None, seeds=None, tlat=0, max_tlat=None, feed=None,
         fill=None):
    """engine.FleetLocalization on the new entry over the formations adjs, and
    the restatement's trackers. tlat: an int or a list of [n][n] per swarm;
    feed: None or a list of [n] per swarm; fill: a byte the workspace is filled
    with instead of zero."""
    import torch
    from aclswarm_amd import engine
    fidx = np.arange(len(adjs)) if fidx is None else np.asarray(fidx)
    B, n = len(fidx), len(adjs[0])
    T = G._table([TL._Form(a) for a in adjs])
    kw = {}
    if loss is not None:
        kw["loss"] = G._u16(np.stack([LO.loss_matrix(n, m) for m in loss]))
    if seeds is not None:
        kw["loss_seed"] = G._t(np.array(seeds, np.uint32).view(np.int32), np.int32)
    if feed is not None:
        kw["feed_loss"] = G._u16(np.stack([DG.feed_vector(n, f) for f in feed]))
    tl = tlat if isinstance(tlat, int) else G._t(np.stack(tlat), np.uint8)
    Pt = None if Pts is None else G._u16(np.stack(Pts))
    loc = engine.FleetLocalization(T, G._t(fidx, np.int32), Pt=Pt, table_latency=tl,
                                   max_table_latency=max_tlat, **kw)
    if fill is not None:
        from aclswarm_amd import _lib as L
        nbytes = int(L.lib().acl_fleet_delay_localize_workspace_bytes(n, B, loc.max_table_latency))
        loc.loc_ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=loc.device)
    trs = [DG.DelayedTrackers(adjs[fidx[b]], Pt=None if Pts is None else Pts[b],
                              loss=0 if loss is None else loss[b],
                              seed=0 if seeds is None else seeds[b],
                              tlat=tlat if isinstance(tlat, int) else tlat[b],
                              max_tlat=loc.max_table_latency,
                              feed_loss=0 if feed is None else feed[b])
           for b in range(B)]
    return loc, trs


def _got(loc):
    d = TL._got(loc)
    d["n_missed"] = None if loc.n_missed is None else loc.n_missed.cpu().numpy()
    d["log"] = None if loc.loc_ws is None else loc.loc_ws.cpu().numpy().reshape(loc.B, -1)
    return d


def _compare(loc, trs, exps, what, skip=(), log=True):
    got = _got(loc)
    for b, tr in enumerate(trs):
        if b in skip:
            continue
        w = f"swarm {b} {what}"
        np.testing.assert_array_equal(got["stamp"][b], tr.stamps(), err_msg=f"{w}: stamp")
        np.testing.assert_array_equal(got["est"][b].view(np.uint64), tr.est().view(np.uint64),
                                      err_msg=f"{w}: est")
        assert got["round"][b] == tr.round, w
        if got["n_lost"] is not None:
            np.testing.assert_array_equal(got["n_lost"][b], tr.n_lost, err_msg=f"{w}: n_lost")
        np.testing.assert_array_equal(got["n_missed"][b], tr.n_missed, err_msg=f"{w}: n_missed")
        assert {k: int(got["status"][k][b]) for k in exps[b]} == exps[b], w
        if log and tr.n <= 13:
            assert got["log"][b].tobytes() == tr.log_bytes(), f"{w}: log"
    return got


def _run(loc, trs, rounds, q, what="", skip=(), log=True):
    q = np.asarray(q, np.float64)
    loc.run(rounds, G._t(q, np.float64))
    exps = [tr.run(rounds, q[b] if q.ndim == 3 else q[:, b]) if b not in skip else None
            for b, tr in enumerate(trs)]
    return _compare(loc, trs, exps, what, skip, log)


_traj = TL._traj


def test_a_single_vehicle():
    loc, trs = _loc([np.zeros((1, 1), np.uint8)] * 2, tlat=3, max_tlat=3, feed=[[0], [0xFFFF]],
                    seeds=[1, 2])
    got = _run(loc, trs, 5, _traj(2, 1, 5, 1))
    assert got["stamp"].reshape(-1).tolist() == [5, 0] and got["n_missed"].tolist() == [[0], [5]]
    got = _run(loc, trs, 0, np.zeros((2, 1, 3)), "no round")
    assert got["round"].tolist() == [5, 5] and (got["status"]["rounds_run"] == 0).all()


def test_swarm6_and_the_two_rings():
    _, adj, _, q0 = H.swarm6()
    tl = [DC.tlat_draw(6, 70 + b, 2) for b in range(3)]
    loc, trs = _loc([adj[0], adj[1], adj[2]], tlat=tl, max_tlat=2)
    _run(loc, trs, 1, np.stack([q0] * 3), "round 0")
    got = _run(loc, trs, 11, _traj(3, 6, 11, 3), "rounds 1-11")
    assert (got["status"]["n_unknown"] == 0).all()
    loc, trs = _loc([C.two_rings(6)] * 2, tlat=1)
    got = _run(loc, trs, 9, _traj(2, 12, 9, 5))
    assert (got["status"]["n_unknown"] == 72).all() and not got["est"][:, :6, 6:].any()
    assert (got["status"]["max_age"] == 5).all()  # three hops at two rounds each


@pytest.mark.parametrize("split", [None, 5])
def test_chord_ring_13_the_mixed_batch(split):
    """B = 8: a drawn latency matrix per swarm in 0..3 and every link at 7 on
    swarm 7, loss_matrices13(), feed thresholds in {0, 8192, 0xFFFF}; 24
    rounds in one call, and as 5 + 19: the log (8 slots) wraps and tables are
    in flight across the boundary."""
    adj, tl, ms, seeds, fd = DC.mixed13()
    loc, trs = _loc([adj] * 8, loss=ms, seeds=seeds, tlat=tl, max_tlat=DC.MIXED_MAX_TLAT, feed=fd)
    traj = _traj(8, 13, DC.MIXED_ROUNDS, 20)
    if split:
        _run(loc, trs, split, traj[:split], "call 0")
        got = _run(loc, trs, DC.MIXED_ROUNDS - split, traj[split:], "call 1")
    else:
        got = _run(loc, trs, DC.MIXED_ROUNDS, traj)
    assert got["n_lost"][0].sum() == 0 and (got["n_lost"][1:].sum(axis=1) > 0).all()
    assert got["n_missed"][0].sum() == 0 and (got["n_missed"][1:].sum(axis=1) > 0).all()
    # every link at 7: after 24 rounds the tables of rounds 0..16 have arrived: three hops
    assert got["status"]["n_unknown"][7] > 0


def test_chord_ring_13_known_after_k_d_plus_one_rounds():
    """Reduction 3 on the device: every link at d = 0, 1, 2, 3 (swarm d)."""
    tl = [np.full((13, 13), d) for d in range(4)]
    loc, trs = _loc([C.chord_ring(13)] * 4, tlat=tl, max_tlat=3)
    traj = _traj(4, 13, 24, 7)
    got = _run(loc, trs, 11, traj[:11], "call 0")
    assert (got["status"]["n_unknown"] > 0).tolist() == [False, True, True, True]
    got = _run(loc, trs, 13, traj[11:], "call 1")
    assert got["status"]["n_unknown"].tolist() == [0, 0, 0, 0]
    assert got["status"]["max_age"].tolist() == [DC.KNOWN_AFTER_AT[d][1] for d in range(4)]


@pytest.mark.parametrize("n,max_tlat,rounds", [(64, 2, 12), (65, 2, 12), (128, 2, 12)])
def test_chord_ring_at_wavefront_boundaries(n, max_tlat, rounds):
    """One slot full, the second mask word, and the size limit, B = 4:
    latencies drawn in 0..2; lossless, thresholds 256 and 4096 on every link,
    and a drawn matrix; feed thresholds drawn on swarms 1..3. Two calls,
    2 max_tlat + 8 rounds in all."""
    assert rounds <= 2 * max_tlat + 8
    loss = [0, 256, 4096, LC.loss_draw(n, 7 * n, density=0.3)]
    tl = [DC.tlat_draw(n, 500 + n + b, max_tlat) for b in range(4)]
    fd = [np.zeros(n, np.int64)] + [DC.feed_draw(n, 600 + n + b) for b in range(1, 4)]
    loc, trs = _loc([C.chord_ring(n)] * 4, loss=loss, seeds=[3, 4, 5, 6], tlat=tl,
                    max_tlat=max_tlat, feed=fd)
    traj = _traj(4, n, rounds, n)
    _run(loc, trs, 3, traj[:3], "call 0")
    got = _run(loc, trs, rounds - 3, traj[3:], "call 1")
    assert got["n_lost"][0].sum() == 0 and (got["n_lost"][1:].sum(axis=1) > 0).all()
    assert got["n_missed"][0].sum() == 0 and (got["n_missed"][1:].sum(axis=1) > 0).all()
    assert (loss[3] == LO.DEAD).any()


def test_latency_zero_equals_the_existing_entry():
    """Reduction 1 on the same GPU, byte for byte: asymmetric rows at n = 13
    and the ring of 65, lossless and at threshold 4096, from a workspace filled
    with 0xA5 bytes."""
    for adj, Pt, rounds in ((C.chord_ring(13), np.asarray(C.random_rows(13).Pt), 9),
                            (C.chord_ring(65), None, 12)):
        n = len(adj)
        Pts = None if Pt is None else [Pt] * 2
        traj = _traj(2, n, rounds, 90)
        for loss, seeds in ((None, None), ([4096, 4096], [7, 0xDEADBEEF])):
            a, _ = _loc([adj] * 2, Pts=Pts, loss=loss, seeds=seeds, tlat=0, max_tlat=3, fill=0xA5)
            b, trs = TL._loc([adj] * 2, Pts=Pts, loss=loss, seeds=seeds)
            for lo, hi in ((0, 4), (4, rounds)):
                a.run(hi - lo, G._t(traj[lo:hi], np.float64))
                TL._run(b, trs, hi - lo, traj[lo:hi])
                ga, gb = TL._got(a), TL._got(b)
                for k in ("stamp", "est", "round", "status") + (("n_lost",) if loss else ()):
                    assert ga[k].tobytes() == gb[k].tobytes(), (n, loss, k)
            assert loss is None or ga["n_lost"].sum() > 0
            assert not a.n_missed.any().item()


def test_moving_in_from_the_existing_entry():
    """Three rounds on the existing entry, then the new one at latency 2 on the
    same state with a fresh workspace and every link dead: the first two rounds
    deliver nothing and count nothing."""
    n = 13
    a, trs = _loc([C.chord_ring(n)] * 2, loss=[0, 0], seeds=[1, 2], tlat=2)
    b, _ = TL._loc([C.chord_ring(n)] * 2, loss=[0, 0], seeds=[1, 2])
    traj = _traj(2, n, 9, 33)
    for tr in trs:
        tr.delayed = False
        tr.run(3, traj[:3, trs.index(tr)])
        tr.delayed = True
    b.run(3, G._t(traj[:3], np.float64))
    for k in ("stamp", "est", "round"):
        getattr(a, k).copy_(getattr(b, k))
    before = TL._got(b)["stamp"]
    a.loss = LO.DEAD
    for tr in trs:
        tr.loss = LO.loss_matrix(n, LO.DEAD)
    got = _run(a, trs, 2, traj[3:5], "rounds 3-4")
    assert not got["n_lost"].any()
    off = ~np.eye(n, dtype=bool)
    np.testing.assert_array_equal(got["stamp"][:, off], before[:, off])
    got = _run(a, trs, 1, traj[5:6], "round 5")
    assert (got["n_lost"].sum(axis=1) == int(C.chord_ring(n).sum())).all()
    a.loss = 0
    for tr in trs:
        tr.loss = LO.loss_matrix(n, 0)
    got = _run(a, trs, 3, traj[6:], "rounds 6-8")
    assert (got["stamp"][:, off].max(axis=1) == 7).all()  # a neighbour's table of round 6


def test_rows_rewritten_between_calls_with_tables_in_flight():
    """A table published under the old rows is taken iff the receiver
    subscribes at delivery."""
    sc = C.random_rows(13)
    Pts = [GC.identity(13), np.asarray(sc.Pt)]
    loc, trs = _loc([C.chord_ring(13)] * 2, Pts=Pts, tlat=2)
    _run(loc, trs, 4, _traj(2, 13, 4, 50), "call 0")
    new = [np.asarray(C.random_rows(13, 77).Pt), GC.identity(13)]
    new[1][0, 0], new[1][0, 6] = 6, 0
    loc.Pt.copy_(G._u16(np.stack(new)))
    for tr, P in zip(trs, new):
        tr.Pt = P.copy()
        tr.taken_trace = []
    assert trs[1].subscribed(0) == [5, 6, 7]
    got = _run(loc, trs, 1, _traj(2, 13, 1, 60), "call 1")
    # round 4 delivers the tables of round 2, published under the old rows, to the new subscribers
    assert sorted((u, P) for r, w, u, P in trs[1].taken_trace if w == 0) == [(5, 2), (6, 2), (7, 2)]
    assert got["stamp"][1, 0, 5] == 3 and got["stamp"][1, 0, 7] == 3 and got["stamp"][1, 0, 6] == 3
    _run(loc, trs, 7, _traj(2, 13, 7, 70), "call 2")


def test_a_latency_above_max_tlat_and_a_bad_fidx_leave_the_swarm_untouched():
    adj, tl, ms, seeds, fd = DC.mixed13()
    tl = [t.copy() for t in tl[:5]]
    loc, trs = _loc([adj], fidx=np.zeros(5, np.int32), loss=ms[:5], seeds=seeds[:5], tlat=tl,
                    max_tlat=3, feed=fd[3:8])
    _run(loc, trs, 5, _traj(5, 13, 5, 30), "call 0")
    before = _got(loc)
    loc.table_latency[1, 3, 9] = 4          # above max_tlat, off the diagonal
    loc.table_latency[2, 5, 5] = 200        # on the diagonal: ignored
    trs[2].tlat[5, 5] = 200
    loc.fidx[4] = 1                         # F = 1
    got = _run(loc, trs, 6, _traj(5, 13, 6, 40), "call 1", skip=(1, 4))
    for b in (1, 4):
        for k in ("stamp", "est", "round", "n_lost", "n_missed", "log"):
            assert got[k][b].tobytes() == before[k][b].tobytes(), (b, k)
        assert tuple(got["status"][b]) == (0, 0, 0, GO.BAD_INPUT)
    assert got["round"].tolist() == [11, 5, 11, 11, 5]
    # put right, the swarms go on from where they stood
    loc.table_latency[1, 3, 9] = 3
    trs[1].tlat[3, 9] = 3
    loc.fidx[4] = 0
    _run(loc, trs, 4, _traj(5, 13, 4, 45), "call 2")


def test_tlat_changed_between_two_calls_the_matrix_of_the_due_round_decides():
    tl = [np.full((13, 13), 3), DC.tlat_draw(13, 81, 3)]
    loc, trs = _loc([C.chord_ring(13)] * 2, loss=[256, 4096], seeds=[8, 9], tlat=tl, max_tlat=3)
    _run(loc, trs, 6, _traj(2, 13, 6, 51), "call 0")
    new = [np.full((13, 13), 1), DC.tlat_draw(13, 82, 3)]
    loc.table_latency.copy_(G._t(np.stack(new), np.uint8))
    for tr, t in zip(trs, new):
        tr.tlat = t.copy()
        tr.taken_trace = []
    _run(loc, trs, 1, _traj(2, 13, 1, 52), "call 1")
    # round 6 at latency 1 takes the tables of round 5; those of rounds 3 and 4 are never taken
    assert {P for r, w, u, P in trs[0].taken_trace} | {5} == {5}
    _run(loc, trs, 5, _traj(2, 13, 5, 53), "call 2")


def test_engine_rejections():
    import torch
    from aclswarm_amd import engine
    T = G._table([TL._Form(C.chord_ring(13))])
    fidx = G._t(np.zeros(2), np.int32)
    q = G._t(np.zeros((2, 13, 3)), np.float64)
    t8 = torch.zeros((2, 13, 13), dtype=torch.uint8, device=q.device)
    f16 = torch.zeros((2, 13), dtype=torch.int16, device=q.device)
    for kw in (dict(table_latency=-1), dict(table_latency=8), dict(table_latency=0.5),
               dict(table_latency=True), dict(table_latency=t8[0]), dict(table_latency=t8.cpu()),
               dict(table_latency=t8.to(torch.int32)), dict(table_latency=3, max_table_latency=2),
               dict(max_table_latency=8), dict(max_table_latency=-1), dict(max_table_latency=1.0),
               dict(feed_loss=-1), dict(feed_loss=65536), dict(feed_loss=0.5),
               dict(feed_loss=f16[0]), dict(feed_loss=f16.cpu()),
               dict(feed_loss=f16.to(torch.int32)), dict(loss_seed=3),
               dict(table_latency=1, loss_seed=-1)):
        with pytest.raises(ValueError):
            engine.FleetLocalization(T, fidx, **kw)
    plain = engine.FleetLocalization(T, fidx)
    assert plain.table_latency is None and plain.n_missed is None and plain.loc_ws is None
    loc = engine.FleetLocalization(T, fidx, table_latency=t8, feed_loss=f16, loss_seed=5)
    assert loc.max_table_latency == 7 and loc._feed_seed.tolist() == [5, 6]
    assert engine.FleetLocalization(T, fidx, feed_loss=9).max_table_latency == 0
    for rounds, qq in ((-1, q), (2, q[0]), (2, q.to(torch.float32)), (2, q.cpu()), (2, None)):
        with pytest.raises(ValueError):
            loc.run(rounds, qq)
    loc.table_latency = t8[0]
    with pytest.raises(ValueError):
        loc.run(1, q)
    torch.cuda.synchronize()
    assert not loc.round.any().item() and not loc.stamp.any().item() and loc.loc_ws is None
