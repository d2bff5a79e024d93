"""GPU parity of acl_fleet_est_auction_batch (the lossy fleet auction whose
START reads each vehicle's own snapshot est[b][v]) against the plain-Python
restatement tests/fleet_est_oracle.py, teacher-forced with the call's own
alignments as tests/test_gpu_fleet_loss.py does (whose helpers these are);
against acl_fleet_lossy_auction_batch on the same GPU with est broadcast from
q; a swarm that alternates between the two entries on one workspace; and the
closed pair the feature exists for: a FleetLocalization and a FleetAuction that
share Pt.

Bar: everything bit for bit after every call -- every state and output array
tests/test_gpu_fleet_loss.py compares, n_lost and the statuses; the Rt of every
started vehicle has the bits of engine.vehicle_start on that vehicle's own
snapshot."""
import numpy as np
import pytest

import fleet_auction_cases as C
import fleet_auction_oracle as FO
import fleet_delay_cases as DC
import fleet_est_oracle as EO
import fleet_localize_cases as GC
import fleet_localize_oracle as GO
import fleet_loss_cases as LC
import test_gpu_fleet_auction as G
import test_gpu_fleet_delay as GD
import test_gpu_fleet_loss as GL

pytestmark = pytest.mark.gpu


def _broadcast(q):
    """est[b][v] = q[b] for every v."""
    B, n = q.shape[:2]
    return np.ascontiguousarray(np.broadcast_to(q[:, None], (B, n, n, 3)))


def _check_rt(fa, cmd, est, rows_before, Rt):
    """The Rt the call wrote for every started vehicle has the bits of
    engine.vehicle_start for the same row on the vehicle's own snapshot:
    S = B n snapshots, qidx = b n + v."""
    import torch
    from aclswarm_amd import engine
    B, n = est.shape[:2]
    ks = [(b, v) for b in range(B) for v in range(n)
          if cmd[b, v] == FO.START and sorted(rows_before[b, v].tolist()) == list(range(n))]
    if not ks:
        return 0
    bs = np.array([b for b, _ in ks])
    vs = np.array([v for _, v in ks])
    out = engine.vehicle_start(fa.table, G._t(fa.fidx.cpu().numpy()[bs], np.int32),
                               G._t(vs, np.int32), G._t(est.reshape(B * n, n, 3), np.float64),
                               G._u16(rows_before[bs, vs]), qidx=G._t(bs * n + vs, np.int32),
                               want_bid=False)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(Rt[bs, vs].view(np.uint64),
                                  out["Rt"].cpu().numpy().view(np.uint64))
    assert not out["flags"].cpu().numpy().any()
    return len(ks)


def _call(fa, fleets, lcs, ticks, cmd, est, what):
    """One call on the device and on the restatements; cmd None: carry on."""
    rows_before = np.stack([fl.Pt.copy() for fl in fleets])
    fa.run(ticks, cmd=None if cmd is None else G._t(cmd, np.uint8),
           est=None if est is None else G._t(est, np.float64))
    Rt = G._state(fa)["Rt"]
    if cmd is not None:
        _check_rt(fa, cmd, est, rows_before, Rt)
    exps = [fl.run(ticks, cmd=None if cmd is None else cmd[b], Rt=Rt[b],
                   est=None if est is None else est[b]) for b, fl in enumerate(fleets)]
    GL._compare(fa, lcs, fleets, exps, what)
    return exps


def _run_parity(lcs, queue_cap=None):
    """fleet_loss's call plan with est broadcast from each window's q."""
    max_iter = lcs[0].max_iter
    fa = GL._fleet(lcs, queue_cap=queue_cap, max_iter=max_iter)
    fleets = [GC.EstCase(lc).fleet(queue_cap) for lc in lcs]
    calls, budget = GD._calls(lcs)
    for ci, (ticks, issue) in enumerate(calls):
        cmd, q = GD._commands(lcs, issue, fleets)
        exps = _call(fa, fleets, lcs, ticks, cmd, _broadcast(q), f"call {ci}")
        assert all(e["flags"] & FO.QUIESCENT for e in exps) or ticks < budget
    return fa, fleets


@pytest.mark.parametrize("key", [("item5", "swarm6"), ("item5", "ring13"), ("matrices13",),
                                 ("wrap13",)], ids=lambda k: "-".join(str(x) for x in k))
def test_a_est_broadcast_from_q_on_the_loss_batches(key):
    """(a): with est[b][v] = q[b] the committed loss batches give the lossy
    restatement's figures."""
    lcs = getattr(LC, key[0])(*key[1:])
    fa, fleets = _run_parity(lcs)
    want = {("item5", "swarm6"): list(zip(LC.ITEM5_OPEN["swarm6"], LC.ITEM5_LOST["swarm6"])),
            ("item5", "ring13"): list(zip(LC.ITEM5_OPEN["ring13"], LC.ITEM5_LOST["ring13"])),
            ("matrices13",): [f[1:] for f in LC.MATRIX_FIGURES],
            ("wrap13",): [f[1:] for f in LC.WRAP_FIGURES]}[key]
    assert [LC.figures(fl, [])[1:] for fl in fleets] == want


def test_a_dead_links_and_loss_before_capacity():
    lc, u = LC.dead_link()
    fa, fleets = _run_parity([lc])
    assert GL._n_lost(fa)[0][LC.DEAD_W] == 2
    fa, fleets = _run_parity([LC.dead_into_3()], queue_cap=2)
    assert GL._n_lost(fa)[0][3] == 6 and fa.status()["flags"][0] == FO.QUIESCENT | FO.OVERFLOW


def _scenario_fleet(scs, **kw):
    """A clean auction on the scenarios: no latency or loss given."""
    from aclswarm_amd import engine
    return engine.FleetAuction(G._table(scs), G._t(np.arange(len(scs)), np.int32),
                               Pt=G._u16(np.stack([G._rows(sc) for sc in scs])), **kw)


class _Clean:
    """What GL._compare reads of a case."""

    def __init__(self, name):
        self.name = name


def test_b_one_round_is_enough_and_a_start_before_any_round():
    """(b): ring13 and rows13, one lossless round on fresh trackers, then the
    auction from the device's own estimates: the restatement's, which the CPU
    suite shows equal to the shared-snapshot auction. Then the same fleets
    restarted from all-zero snapshots (trackers that never ran)."""
    from aclswarm_amd import engine
    scs = [DC.SCENARIOS[k]() for k in ("ring13", "rows13")]
    n = 13
    q = np.stack([sc.windows[0][1] for sc in scs])
    fa = _scenario_fleet(scs)
    loc = engine.FleetLocalization(fa.table, fa.fidx, Pt=fa.Pt)
    loc.run(1, G._t(q, np.float64))
    est = loc.est.cpu().numpy()
    trs = [GO.Trackers(sc.adj, Pt=sc.Pt) for sc in scs]
    for b, tr in enumerate(trs):
        tr.run(1, q[b])
        np.testing.assert_array_equal(est[b].view(np.uint64), tr.est().view(np.uint64))
    assert (est == 0).all(axis=3).sum() == sum(n * (n - 1) - int(sc.adj.sum()) for sc in scs)
    fleets = [EO.EstFleet(sc.p, sc.adj, 1, Pt=sc.Pt) for sc in scs]
    names = [_Clean(sc.name) for sc in scs]
    cmd = np.ones((2, n), np.uint8)
    ticks = max(sc.ticks for sc in scs)
    exps = _call(fa, fleets, names, ticks, cmd, est, "from one round")
    assert fa.max_latency == 1 and fa.loss is None and not GL._n_lost(fa).any()
    assert all(e["flags"] & FO.QUIESCENT and e["n_open"] == 0 for e in exps)
    # the shared-snapshot auction on the lossy entry, same GPU: the same bits,
    # although every vehicle started with n - 1 - deg vehicles at the origin
    fs = _scenario_fleet(scs, loss=0)
    fs.run(ticks, q=G._t(q, np.float64), cmd=G._t(cmd, np.uint8))
    a, s = G._state(fa), G._state(fs)
    for k in a:
        np.testing.assert_array_equal(a[k], s[k], err_msg=k)
    np.testing.assert_array_equal(fa.status(), fs.status())
    np.testing.assert_array_equal(fa.ws.cpu().numpy(), fs.ws.cpu().numpy())
    # a START before any gossip round: every snapshot all zero
    zero = np.zeros((2, n, n, 3))
    exps = _call(fa, fleets, names, ticks, cmd, zero, "from zero")
    assert ((G._state(fa)["vflags"] & FO.V_STARTED) != 0).all()


def test_c_the_stale_batch_and_the_shared_snapshot_run():
    """(c): the trackers of the stale batch on the device (B = 8, a snapshot per
    round for 24 rounds, gossip loss 0 / 4096), then one clean auction from
    loc.est, beside the shared-snapshot auction on acl_fleet_lossy_auction_batch:
    swarm 0's tables are that run's, every other swarm's final prices differ."""
    from aclswarm_amd import engine
    sb, trs, runs, shared = GC.stale13()
    assert GC.stale_condition(runs, shared)  # (asserted by the CPU suite too)
    B, n = GC.STALE_B, sb.n
    T = G._table([C.Scenario("stale13", sb.p, sb.adj, [])])
    fidx = G._t(np.zeros(B), np.int32)
    loss = np.stack([np.full((n, n), x) for x in sb.loss])
    loc = engine.FleetLocalization(T, fidx, loss=G._u16(loss), loss_seed=0)
    loc.run(GC.STALE_ROUNDS, G._t(np.stack([sb.traj] * B, axis=1), np.float64))
    est = loc.est.cpu().numpy()
    for b, tr in enumerate(trs):
        np.testing.assert_array_equal(est[b].view(np.uint64), tr.est().view(np.uint64))
        np.testing.assert_array_equal(loc.n_lost.cpu().numpy()[b], tr.n_lost)
    fa = engine.FleetAuction(T, fidx)
    fleets = [sb.fleet() for _ in range(B)]
    cmd = np.ones((B, n), np.uint8)
    exps = _call(fa, fleets, [_Clean(f"stale13/{b}") for b in range(B)], sb.ticks, cmd, est,
                 "the auction")
    assert all(e["flags"] & FO.QUIESCENT and e["n_open"] == 0 for e in exps)
    fs = engine.FleetAuction(T, fidx, loss=0)
    fs.run(sb.ticks, q=G._t(np.stack([sb.q] * B), np.float64), cmd=G._t(cmd, np.uint8))
    a, s = G._state(fa), G._state(fs)
    for k in a:
        np.testing.assert_array_equal(a[k][0], s[k][0], err_msg=k)
    fp, sp = a["final_price"].view(np.uint32), s["final_price"].view(np.uint32)
    assert all(not np.array_equal(fp[b], sp[b]) for b in range(1, B))
    assert not GL._n_lost(fa).any()


@pytest.mark.parametrize("n", [64, 65, 128])
def test_rings_at_wavefront_boundaries_against_the_lossy_entry(n):
    """LC.rings(n) with est broadcast from q beside acl_fleet_lossy_auction_batch
    on the same GPU: state, outputs, statuses, n_lost and the workspace bytes."""
    lcs = LC.rings(n)
    old, new = (GL._fleet(lcs, max_iter=lcs[0].max_iter) for _ in range(2))
    cmd, q = GD._commands(lcs, {b: 0 for b in range(len(lcs))}, [None] * len(lcs))
    old.run(DC.BUDGET, q=G._t(q, np.float64), cmd=G._t(cmd, np.uint8))
    new.run(DC.BUDGET, cmd=G._t(cmd, np.uint8), est=G._t(_broadcast(q), np.float64))
    so, sn = G._state(old), G._state(new)
    for k in so:
        np.testing.assert_array_equal(sn[k], so[k], err_msg=k)
    np.testing.assert_array_equal(new.status(), old.status())
    np.testing.assert_array_equal(GL._n_lost(new), GL._n_lost(old))
    np.testing.assert_array_equal(new.ws.cpu().numpy(), old.ws.cpu().numpy())
    assert GL._figures(new) == LC.RING_FIGURES[n]


def test_a_swarm_alternates_between_the_lossy_and_the_own_estimate_entry():
    """ring13 under loss 64, seeds 1 and 3, on one workspace: START on the
    own-estimate entry (10 ticks), 25 ticks on the lossy entry, a restart on
    the lossy entry from q after the stall, then a restart from est."""
    lcs = [LC.LossCase(DC.draw("ring13"), 64, s) for s in (1, 3)]
    fa = GL._fleet(lcs)
    fleets = [GC.EstCase(lc).fleet() for lc in lcs]
    cmd, q = GD._commands(lcs, {0: 0, 1: 0}, fleets)
    est = _broadcast(q)
    est[:, :, :, 2] += np.arange(13)[None, :, None] * 0.01  # every vehicle its own picture
    _call(fa, fleets, lcs, 10, cmd, est, "call 0 (est)")
    # the lossy entry, no command
    fa.run(25)
    Rt = G._state(fa)["Rt"]
    GL._compare(fa, lcs, fleets, [fl.run(25, Rt=Rt[b]) for b, fl in enumerate(fleets)],
                "call 1 (lossy)")
    # a restart from q on the lossy entry: the restatement reads q through est = None
    fa.run(DC.BUDGET, q=G._t(q, np.float64), cmd=G._t(cmd, np.uint8))
    Rt = G._state(fa)["Rt"]
    GL._compare(fa, lcs, fleets,
                [fl.run(DC.BUDGET, q=q[b], cmd=cmd[b], Rt=Rt[b]) for b, fl in enumerate(fleets)],
                "call 2 (lossy)")
    _call(fa, fleets, lcs, DC.BUDGET, cmd, est, "call 3 (est)")
    _call(fa, fleets, lcs, 5, None, None, "call 4 (est, no command)")


def test_the_closed_pair_localization_and_auction_share_their_rows():
    """A FleetLocalization and a FleetAuction share Pt: 6 rounds, START from
    loc.est, the auction to quiescence (every vehicle adopts its table), then
    more rounds on the adopted rows; both restatements run the same way."""
    from aclswarm_amd import engine
    scs = [C.random_rows(13), C.clean_ring(13)]
    n, B = 13, 2
    fa = _scenario_fleet(scs)
    loc = engine.FleetLocalization(fa.table, fa.fidx, Pt=fa.Pt)
    assert loc.Pt is fa.Pt
    trs = [GO.Trackers(sc.adj, Pt=sc.Pt) for sc in scs]
    fleets = [EO.EstFleet(sc.p, sc.adj, 1, Pt=sc.Pt) for sc in scs]
    traj = np.stack([GC.trajectory(n, 14, 300 + b) for b in range(B)], axis=1)

    def rounds(lo, hi, what):
        loc.run(hi - lo, G._t(traj[lo:hi], np.float64))
        for b, tr in enumerate(trs):
            tr.Pt = fleets[b].Pt  # the restatements share their rows too
            st = tr.run(hi - lo, traj[lo:hi, b])
            np.testing.assert_array_equal(loc.stamp.cpu().numpy()[b], tr.stamps(), err_msg=what)
            np.testing.assert_array_equal(loc.est.cpu().numpy()[b].view(np.uint64),
                                          tr.est().view(np.uint64), err_msg=what)
            assert {k: int(loc.status()[k][b]) for k in st} == st, what

    rounds(0, 6, "before the auction")
    rows0 = [fl.Pt.copy() for fl in fleets]
    exps = _call(fa, fleets, [_Clean(sc.name) for sc in scs], max(sc.ticks for sc in scs),
                 np.ones((B, n), np.uint8), loc.est.cpu().numpy(), "the auction")
    assert all(e["flags"] & FO.QUIESCENT and e["n_open"] == 0 for e in exps)
    assert ((G._state(fa)["vflags"] & FO.V_ADOPTED) != 0).all()
    assert any((fl.Pt != r).any() for fl, r in zip(fleets, rows0))  # the gossip is rewired
    rounds(6, 14, "on the adopted rows")


def test_engine_rejections_and_the_workspace():
    import torch
    from aclswarm_amd import _lib as L
    from aclswarm_amd import engine
    sc = C.clean_ring(13)
    n, B = 13, 2
    fa = _scenario_fleet([sc, sc])
    cmd = G._t(np.ones((B, n)), np.uint8)
    est = G._t(np.zeros((B, n, n, 3)), np.float64)
    for bad in (est[0], est.to(torch.float32), est.cpu(), est[:, :, :, :2], est.transpose(1, 2)):
        with pytest.raises(ValueError):
            fa.run(5, cmd=cmd, est=bad)
    with pytest.raises(ValueError):
        fa.run(5, cmd=cmd)  # neither q nor est
    assert fa.ws is None and fa.latency is None
    fa.run(5, cmd=cmd, est=est)
    assert fa.max_latency == 1
    assert fa.ws.numel() == L.lib().acl_fleet_delay_workspace_bytes(n, B, 4 * n, 1)
    # an object that has run on the plain workspace cannot move to the delay layout
    fb = _scenario_fleet([sc, sc])
    fb.run(5, q=G._t(np.zeros((B, n, 3)), np.float64), cmd=cmd)
    with pytest.raises(ValueError):
        fb.run(5, cmd=cmd, est=est)
