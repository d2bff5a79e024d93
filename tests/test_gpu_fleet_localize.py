"""GPU parity of acl_fleet_localize_batch (per-vehicle position estimates by
gossip: B swarms of VehicleTrackers advanced round by round in one launch)
against the plain-Python restatement tests/fleet_localize_oracle.py.

Bar: everything bit for bit after every call -- stamp, est (as u64 bits),
round, n_lost and the status records. The shapes are the smallest at which the
kernel can go wrong: n = 1, a non-multiple of anything (6, 12, 13), one slot
full (64), the second mask word (65) and the size limit (128)."""
import numpy as np
import pytest

import fleet_auction_cases as C
import fleet_localize_cases as GC
import fleet_localize_oracle as GO
import fleet_loss_cases as LC
import fleet_loss_oracle as LO
import helpers as H
import test_gpu_fleet_auction as G

pytestmark = pytest.mark.gpu


class _Form:
    def __init__(self, adj):
        self.adj = np.asarray(adj, np.uint8)
        self.n = len(self.adj)
        self.p = C.points(np.random.RandomState(self.n), self.n)


def _loc(adjs, Pts=None, fidx=None, loss=None, seeds=None):
    """engine.FleetLocalization over the formations adjs (swarm b flies
    formation fidx[b]; None: b) and the restatement's trackers."""
    from aclswarm_amd import engine
    fidx = np.arange(len(adjs)) if fidx is None else np.asarray(fidx)
    B, n = len(fidx), len(adjs[0])
    T = G._table([_Form(a) for a in adjs])
    kw = {}
    if loss is not None:
        kw = dict(loss=G._u16(np.stack([LO.loss_matrix(n, m) for m in loss])),
                  loss_seed=G._t(np.array(seeds, np.uint32).view(np.int32), np.int32))
    Pt = None if Pts is None else G._u16(np.stack(Pts))
    loc = engine.FleetLocalization(T, G._t(fidx, np.int32), Pt=Pt, **kw)
    trs = [GO.Trackers(adjs[fidx[b]], Pt=None if Pts is None else Pts[b],
                       loss=0 if loss is None else loss[b], seed=0 if seeds is None else seeds[b])
           for b in range(B)]
    return loc, trs


def _got(loc):
    import torch
    torch.cuda.synchronize()
    d = dict(stamp=loc.stamp.cpu().numpy(), est=loc.est.cpu().numpy(),
             round=loc.round.cpu().numpy(), status=loc.status())
    d["n_lost"] = None if loc.n_lost is None else loc.n_lost.cpu().numpy()
    return d


def _compare(loc, trs, exps, what, skip=()):
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
        assert {k: int(got["status"][k][b]) for k in exps[b]} == exps[b], w
    return got


def _run(loc, trs, rounds, q, what="", skip=()):
    """One call on the device and on the restatements. q: [B][n][3] or
    [rounds][B][n][3]."""
    q = np.asarray(q, np.float64)
    loc.run(rounds, G._t(q, np.float64))
    exps = [tr.run(rounds, q[b] if q.ndim == 3 else q[:, b]) if b not in skip else None
            for b, tr in enumerate(trs)]
    return _compare(loc, trs, exps, what, skip)


def _traj(B, n, rounds, seed):
    """[rounds][B][n][3]: an independent trajectory per swarm."""
    return np.stack([GC.trajectory(n, rounds, seed + b) for b in range(B)], axis=1)


def test_a_single_vehicle():
    loc, trs = _loc([np.zeros((1, 1), np.uint8)] * 2)
    got = _run(loc, trs, 3, _traj(2, 1, 3, 1))
    assert got["stamp"].reshape(-1).tolist() == [3, 3] and (got["status"]["max_age"] == 0).all()
    got = _run(loc, trs, 0, np.zeros((2, 1, 3)), "no round")
    assert got["round"].tolist() == [3, 3] and (got["status"]["rounds_run"] == 0).all()


def test_swarm6_and_the_two_rings():
    _, adj, _, q0 = H.swarm6()
    loc, trs = _loc([adj[0], adj[1], adj[2]])
    _run(loc, trs, 1, np.stack([q0] * 3), "round 0")
    got = _run(loc, trs, 4, _traj(3, 6, 4, 3), "rounds 1-4")
    assert (got["status"]["n_unknown"] == 0).all()
    loc, trs = _loc([C.two_rings(6)] * 2)
    got = _run(loc, trs, 9, _traj(2, 12, 9, 5))
    assert (got["status"]["n_unknown"] == 72).all() and not got["est"][:, :6, 6:].any()


@pytest.mark.parametrize("split", [None, 5])
def test_chord_ring_13_a_loss_matrix_per_swarm(split):
    """B = 8, thresholds in {0, 256, 4096, 0xFFFF}: 24 rounds in one call, and
    as 5 + 19."""
    ms, seeds = GC.loss_matrices13()
    loc, trs = _loc([C.chord_ring(13)] * 8, loss=ms, seeds=seeds)
    traj = _traj(8, 13, 24, 20)
    if split:
        _run(loc, trs, split, traj[:split], "call 0")
        got = _run(loc, trs, 24 - split, traj[split:], "call 1")
    else:
        got = _run(loc, trs, 24, traj)
    nl = got["n_lost"].sum(axis=1)
    assert nl[0] == 0 and (nl[1:] > 0).all()
    assert any((m == LO.DEAD).any() for m in ms) and any((m == 256).any() for m in ms)
    assert got["status"]["max_age"].max() > 5  # staler than the lossless diameter


def test_ring_loss_totals_through_the_constructor():
    """The CPU suite's pinned figures: threshold 4096 on every link as an int,
    loss_seed = 0 (swarm b: seed b), 24 rounds from round 0."""
    from aclswarm_amd import engine
    T = G._table([_Form(C.chord_ring(13))])
    loc = engine.FleetLocalization(T, G._t(np.zeros(8), np.int32), loss=GC.LOSS_THR, loss_seed=0)
    trs = [GC.ring_loss(b) for b in range(8)]
    got = _run(loc, trs, GC.LOSS_ROUNDS, np.stack([C.snapshot(np.random.RandomState(4), 13)] * 8))
    assert got["n_lost"].sum(axis=1).tolist() == GC.LOSS_TOTALS


def test_asymmetric_subscriptions_a_bad_row_and_a_bad_fidx():
    """random_rows(13) (two draws), identity rows with one vehicle's row no
    permutation, and a swarm whose fidx is out of range: it is run for three
    rounds first, then its state and round do not move."""
    scs = [C.random_rows(13), C.random_rows(13, C.ROWS_STALL_SEED)]
    bad = GC.identity(13)
    bad[4, 0] = bad[4, 1]
    big = GC.identity(13)
    big[7, 2] = 13  # out of range
    Pts = [np.asarray(scs[0].Pt), np.asarray(scs[1].Pt), bad, big, GC.identity(13)]
    fidx = np.zeros(5, np.int32)
    loc, trs = _loc([C.chord_ring(13)], Pts=Pts, fidx=fidx, loss=[0, 4096, 0, 256, 4096],
                    seeds=[1, 2, 3, 4, 5])
    got = _run(loc, trs, 3, _traj(5, 13, 3, 30), "call 0")
    assert got["status"]["flags"].tolist() == [0, 0, GO.BAD_ROW, GO.BAD_ROW, 0]
    # vehicle 4 of swarm 2 hears nobody, and its ring neighbours hear it
    assert (np.delete(got["stamp"][2, 4], 4) == 0).all()
    assert got["stamp"][2, 3, 4] == 3 and got["stamp"][2, 5, 4] == 3
    before = got
    loc.fidx[4] = 1  # F = 1
    loc.fidx[1] = -1
    got = _run(loc, trs, 6, _traj(5, 13, 6, 40), "call 1", skip=(1, 4))
    for b in (1, 4):
        for k in ("stamp", "est", "round", "n_lost"):
            np.testing.assert_array_equal(got[k][b], before[k][b], err_msg=k)
        assert tuple(got["status"][b]) == (0, 0, 0, GO.BAD_INPUT)
    assert got["round"].tolist() == [9, 3, 9, 9, 3]


def test_rows_rewritten_between_two_calls():
    sc = C.random_rows(13)
    Pts = [GC.identity(13), np.asarray(sc.Pt)]
    loc, trs = _loc([C.chord_ring(13)] * 2, Pts=Pts)
    _run(loc, trs, 2, _traj(2, 13, 2, 50), "call 0")
    new = [np.asarray(C.random_rows(13, 77).Pt), GC.identity(13)]
    new[1][0, 0], new[1][0, 6] = 6, 0
    loc.Pt.copy_(G._u16(np.stack(new)))
    for tr, P in zip(trs, new):
        tr.Pt = P.copy()
    assert trs[1].subscribed(0) == [5, 6, 7]
    got = _run(loc, trs, 1, _traj(2, 13, 1, 60), "call 1")
    assert got["stamp"][1, 0, 5] == 3 and got["stamp"][1, 0, 7] == 3
    _run(loc, trs, 7, _traj(2, 13, 7, 70), "call 2")


@pytest.mark.parametrize("n,rounds", [(64, 33), (65, 33), (128, 70)])
def test_chord_ring_at_wavefront_boundaries(n, rounds):
    """One slot, the second mask word, and the size limit, B = 4: lossless,
    thresholds 256 and 4096 on every link, and a drawn matrix; enough rounds
    for the last unknown entry of the lossless swarm to fill in."""
    loss = [0, 256, 4096, LC.loss_draw(n, 7 * n, density=0.3)]
    loc, trs = _loc([C.chord_ring(n)] * 4, loss=loss, seeds=[3, 4, 5, 6])
    traj = _traj(4, n, rounds, n)
    _run(loc, trs, 3, traj[:3], "call 0")
    got = _run(loc, trs, rounds - 3, traj[3:], "call 1")
    st = got["status"]
    assert st["n_unknown"][0] == 0 and st["max_age"][0] == GC.KNOWN_AFTER[n][1]
    assert got["n_lost"][0].sum() == 0 and (got["n_lost"][1:].sum(axis=1) > 0).all()
    assert (loss[3] == LO.DEAD).any()


def test_one_snapshot_equals_a_trajectory_of_equal_snapshots():
    ms, seeds = GC.loss_matrices13()
    q = np.stack([C.snapshot(np.random.RandomState(80 + b), 13) for b in range(8)])
    a, trs = _loc([C.chord_ring(13)] * 8, loss=ms, seeds=seeds)
    b, _ = _loc([C.chord_ring(13)] * 8, loss=ms, seeds=seeds)
    _run(a, trs, 9, q)
    b.run(9, G._t(np.stack([q] * 9), np.float64))
    ga, gb = _got(a), _got(b)
    for k in ("stamp", "est", "round", "n_lost", "status"):
        assert ga[k].tobytes() == gb[k].tobytes(), k


def test_loss_all_zero_equals_no_loss():
    """The lossy instantiation at threshold 0 against the lossless one on the
    same GPU, byte for byte, on asymmetric rows at n = 13 and on the ring of
    65."""
    for adj, Pt, rounds in ((C.chord_ring(13), np.asarray(C.random_rows(13).Pt), 7),
                            (C.chord_ring(65), None, 12)):
        n = len(adj)
        Pts = None if Pt is None else [Pt] * 2
        a, trs = _loc([adj] * 2, Pts=Pts, loss=[0, 0], seeds=[0, 0xDEADBEEF])
        b, _ = _loc([adj] * 2, Pts=Pts)
        traj = _traj(2, n, rounds, 90)
        _run(a, trs, rounds, traj)
        b.run(rounds, G._t(traj, np.float64))
        ga, gb = _got(a), _got(b)
        for k in ("stamp", "est", "round", "status"):
            assert ga[k].tobytes() == gb[k].tobytes(), k
        assert not ga["n_lost"].any() and gb["n_lost"] is None


def test_engine_rejections():
    import torch
    from aclswarm_amd import engine
    T = G._table([_Form(C.chord_ring(13))])
    fidx = G._t(np.zeros(2), np.int32)
    q = G._t(np.zeros((2, 13, 3)), np.float64)
    m = torch.full((2, 13, 13), 64, dtype=torch.int16, device=q.device)
    for kw in (dict(loss=-1), dict(loss=65536), dict(loss=0.5), dict(loss=m[0]),
               dict(loss=m.cpu()), dict(loss_seed=3), dict(loss=64, loss_seed=-1),
               dict(Pt=m[0]), dict(Pt=m.to(torch.int32))):
        with pytest.raises(ValueError):
            engine.FleetLocalization(T, fidx, **kw)
    with pytest.raises(ValueError):
        engine.FleetLocalization(T, fidx.to(torch.int64))
    loc = engine.FleetLocalization(T, fidx, loss=m, loss_seed=5)
    assert loc.loss_seed.tolist() == [5, 6]
    for rounds, qq in ((-1, q), (2, q[0]), (2, q.to(torch.float32)), (2, q.cpu()),
                       (3, torch.stack([q, q])), (True, q), (1.0, q), (2, None)):
        with pytest.raises(ValueError):
            loc.run(rounds, qq)
    torch.cuda.synchronize()
    assert not loc.round.any().item() and not loc.stamp.any().item()
