"""GPU parity of acl_fleet_lossy_auction_batch (the fleet auction with seeded
per-link message loss: a second ballot in the delay delivery loop) against the
plain-Python restatement tests/fleet_loss_oracle.py, teacher-forced with the
call's own alignments as tests/test_gpu_fleet_delay.py does (whose helpers
these are); against acl_fleet_delay_auction_batch on the same GPU at loss 0;
and a swarm that moves between the two entries on one workspace.

Bar: everything bit for bit after every call -- every state and output array,
n_lost and the statuses. tests/test_fleet_loss.py asserts on the CPU that every
batch here holds a swarm that loses nothing, one that loses a bid and one that
ends with open vehicles."""
import numpy as np
import pytest

import fleet_auction_oracle as FO
import fleet_delay_cases as DC
import fleet_loss_cases as LC
import fleet_loss_oracle as LO
import test_gpu_fleet_auction as G
import test_gpu_fleet_delay as GD

pytestmark = pytest.mark.gpu


def _seeds(lcs):
    return G._t(np.array([lc.seed for lc in lcs], np.uint32).view(np.int32), np.int32)


def _fleet(lcs, queue_cap=None, max_iter=0, **kw):
    """The cases as the swarms of one engine.FleetAuction on the lossy entry.
    kw: loss / loss_seed for the constructor; default: the cases' own matrices
    and seeds, set through the attributes."""
    from aclswarm_amd import engine
    scs = [c.sc for c in lcs]
    lat = np.stack([c.lat for c in lcs])
    if not kw:
        kw = dict(loss=G._u16(np.stack([c.loss for c in lcs])), loss_seed=_seeds(lcs))
    return engine.FleetAuction(G._table(scs), G._t(np.arange(len(scs)), np.int32),
                               Pt=G._u16(np.stack([G._rows(sc) for sc in scs])),
                               queue_cap=queue_cap, max_iter=max_iter,
                               latency=G._t(lat, np.uint8),
                               max_latency=max(c.max_lat for c in lcs), **kw)


def _n_lost(fa):
    return fa.n_lost.cpu().numpy()


def _compare(fa, lcs, fleets, exps, what):
    got, st, nl = G._state(fa), fa.status(), _n_lost(fa)
    for b, lc in enumerate(lcs):
        w = f"{lc.name} (swarm {b}) {what}"
        G._assert_swarm(got, b, fleets[b], st, exps[b], w)
        np.testing.assert_array_equal(nl[b], fleets[b].n_lost, err_msg=f"{w}: n_lost")
    return got


def _run_parity(lcs, queue_cap=None, split=None, **kw):
    """Every call of the batch (fleet_delay's call plan) on the device and on
    the restatements, compared after every call. split: the first call's
    ticks are run as two calls, split ticks and the rest without a command.
    Returns (fa, fleets)."""
    scs = [c.sc for c in lcs]
    max_iter = lcs[0].max_iter
    assert all(c.max_iter == max_iter for c in lcs)
    fa = _fleet(lcs, queue_cap=queue_cap, max_iter=max_iter, **kw)
    fleets = [lc.fleet(queue_cap) for lc in lcs]
    calls, budget = GD._calls(lcs)
    for ci, (ticks, issue) in enumerate(calls):
        cmd, q = GD._commands(lcs, issue, fleets)
        rows_before = np.stack([fl.Pt.copy() for fl in fleets])
        parts = [split, ticks - split] if split and ci == 0 else [ticks]
        for pi, t in enumerate(parts):
            first = pi == 0
            fa.run(t, q=G._t(q, np.float64) if first else None,
                   cmd=G._t(cmd, np.uint8) if first else None)
            Rt = G._state(fa)["Rt"]
            if first:
                G._check_rt(fa, scs, cmd, q, rows_before, Rt)
            exps = [fleets[b].run(t, q=q[b], cmd=cmd[b] if first else None, Rt=Rt[b])
                    for b in range(len(lcs))]
            _compare(fa, lcs, fleets, exps, f"call {ci}.{pi}")
        assert all(e["flags"] & FO.QUIESCENT for e in exps) or ticks < budget
    return fa, fleets


def _figures(fa):
    st, nl = fa.status(), _n_lost(fa)
    return [(int(st["ticks_run"][b]), int(st["n_open"][b]), int(nl[b].sum()))
            for b in range(len(nl))]


@pytest.mark.parametrize("name,split", [("swarm6", None), ("ring13", None), ("ring13", 5)])
def test_mixed_batch_loss_64_seeds_0_to_7(name, split):
    """B = 8 in one launch, loss = 64 and loss_seed = 0 through the
    constructor (swarm b: seed b); ring13 again as 5 ticks and the rest."""
    lcs = LC.item5(name)
    fa, fleets = _run_parity(lcs, split=split, loss=LC.ITEM5_LOSS, loss_seed=0)
    figs = _figures(fa)
    assert [f[2] for f in figs] == LC.ITEM5_LOST[name]
    assert [f[1] for f in figs] == LC.ITEM5_OPEN[name]
    if not split:
        assert [f[0] for f in figs] == LC.ITEM5_TICKS[name]
    assert (fa.status()["flags"] == FO.QUIESCENT).all()


@pytest.mark.parametrize("n", [64, 65, 128])
def test_chord_ring_at_wavefront_boundaries(n):
    """One slot, two slots with the second mask word, and the size limit:
    B = 4, loss 16, seeds 0..3, max_iter = DC.RING_ITERS[n]."""
    fa, fleets = _run_parity(LC.rings(n))
    assert _figures(fa) == LC.RING_FIGURES[n]


def test_a_matrix_per_swarm():
    """B = 8 at n = 13, drawn thresholds in {0, 256, 4096, 0xFFFF}, among them
    the four-window stale sequence: restarts onto stalled auctions."""
    fa, fleets = _run_parity(LC.matrices13())
    assert [LC.figures(fl, [])[1:] for fl in fleets] == [f[1:] for f in LC.MATRIX_FIGURES]


def test_log_ring_wraps_under_loss():
    """max_lat = 2 (a ring of 4 entries per vehicle) under loss 256: lost
    entries do not disturb slot reuse."""
    fa, fleets = _run_parity(LC.wrap13())
    assert fa.max_latency == 2
    assert [LC.figures(fl, [])[1:] for fl in fleets] == [f[1:] for f in LC.WRAP_FIGURES]
    assert (fleets[0].n_tally == 26).all()


def test_loss_zero_equals_the_delay_entry():
    """The swarms and calls of test_gpu_fleet_delay's n = 13 batch with loss 0
    (two seeds) beside acl_fleet_delay_auction_batch on the same GPU: state,
    outputs, statuses, histories and the workspace equal after every call."""
    cases, delays = GD._n13_cases()
    B = len(cases)
    old = GD._fleet(cases)
    news = [_fleet(LC.batch(cases, 0, s)) for s in (0, 0xDEADBEEF)]
    calls, _ = GD._calls(cases, delays)
    for ci, (ticks, issue) in enumerate(calls):
        inv = old.invalid.cpu().numpy()
        cmd, q = GD._commands(cases, issue, [GD._Flags(inv[b]) for b in range(B)])
        hs = [fa.run(ticks, q=G._t(q, np.float64), cmd=G._t(cmd, np.uint8), history=True)
              for fa in [old] + news]
        so = G._state(old)
        for fa, h in zip(news, hs[1:]):
            sn = G._state(fa)
            for k in so:
                np.testing.assert_array_equal(sn[k], so[k], err_msg=f"call {ci}: {k}")
            np.testing.assert_array_equal(fa.status(), old.status())
            for k in ("biditer", "open"):
                np.testing.assert_array_equal(h[k].cpu().numpy(), hs[0][k].cpu().numpy())
            np.testing.assert_array_equal(fa.ws.cpu().numpy(), old.ws.cpu().numpy())
            assert not _n_lost(fa).any()
    assert (so["vflags"] & FO.V_CONSENSUS).any() and so["n_thrown"].sum() > 0


def test_a_swarm_moves_between_the_delay_entry_and_the_lossy_one():
    """ring13 under loss 64, seed 1 loses the bid due at tick 30. 10 ticks on
    the lossy entry, 25 on acl_fleet_delay_auction_batch (loss = None: the bid
    arrives), the rest on the lossy entry again, on one workspace; the
    restatement runs the middle call with loss 0."""
    lcs = [LC.LossCase(DC.draw("ring13"), 64, s) for s in (1, 3)]
    fa = _fleet(lcs)
    fleets = [lc.fleet() for lc in lcs]
    loss, seeds = fa.loss, fa.loss_seed
    cmd, q = GD._commands(lcs, {0: 0, 1: 0}, fleets)
    for ci, (t, lossy) in enumerate(((10, True), (25, False), (DC.BUDGET, True))):
        fa.loss = loss if lossy else None
        for fl, lc in zip(fleets, lcs):
            fl.loss = lc.loss if lossy else LO.loss_matrix(13, 0)
        fa.run(t, q=G._t(q, np.float64) if ci == 0 else None,
               cmd=G._t(cmd, np.uint8) if ci == 0 else None)
        Rt = G._state(fa)["Rt"]
        exps = [fl.run(t, q=q[b], cmd=cmd[b] if ci == 0 else None, Rt=Rt[b])
                for b, fl in enumerate(fleets)]
        _compare(fa, lcs, fleets, exps, f"call {ci}")
    assert fa.loss_seed is seeds
    # seed 1 alone would have stalled at tick 54 with one bid lost
    assert fleets[0].tick > 54


def test_dead_link_and_loss_before_capacity():
    """One dead subscribed link on swarm6: the receiver never tallies, n_lost
    counts the sender's publications. overflow6 (queue_cap 2) with every link
    into vehicle 3 dead: no V_OVERFLOW there, its n_lost counts what would have
    been appended or dropped."""
    lc, u = LC.dead_link()
    fa, fleets = _run_parity([lc])
    nl, nt = _n_lost(fa)[0], fa.n_tally.cpu().numpy()[0]
    assert nt[LC.DEAD_W] == 0 and nl[LC.DEAD_W] == 2 == nl.sum() and nt[u] >= 1
    fa, fleets = _run_parity([LC.dead_into_3()], queue_cap=2)
    vf, nl = fa.vflags.cpu().numpy()[0], _n_lost(fa)[0]
    assert not vf[3] & FO.V_OVERFLOW and vf[5] & FO.V_OVERFLOW
    assert nl[3] == 6 == nl.sum() and fa.queue_len.cpu().numpy()[0, 3] == 0
    assert fa.status()["flags"][0] == FO.QUIESCENT | FO.OVERFLOW


def test_loss_and_seed_change_between_calls():
    """40 ticks under (loss 64, seed 1 + b), then the rest under (2048,
    99 + b): the pair of the call in whose delivery phase a bid is due decides."""
    lcs = LC.batch([DC.draw("ring13")] * 2, 64, 1)
    fa = _fleet(lcs)
    fleets = [lc.fleet() for lc in lcs]
    cmd, q = GD._commands(lcs, {0: 0, 1: 0}, fleets)
    fa.run(40, q=G._t(q, np.float64), cmd=G._t(cmd, np.uint8))
    Rt = G._state(fa)["Rt"]
    exps = [fl.run(40, q=q[b], cmd=cmd[b], Rt=Rt[b]) for b, fl in enumerate(fleets)]
    _compare(fa, lcs, fleets, exps, "call 0")
    fa.loss, fa.loss_seed = 2048, 99
    for b, fl in enumerate(fleets):
        fl.loss, fl.seed = LO.loss_matrix(13, 2048), 99 + b
    fa.run(DC.BUDGET)
    exps = [fl.run(DC.BUDGET) for fl in fleets]
    _compare(fa, lcs, fleets, exps, "call 1")
    assert _n_lost(fa)[0].sum() > 1


def test_a_bad_input_swarm_keeps_its_n_lost():
    """B = 2: swarm 0 has a latency entry of 0 (ACL_FLEET_BAD_INPUT, no tick);
    its n_lost stays what the caller left there, swarm 1's grows from it."""
    lcs = LC.batch([DC.draw("ring13")] * 2, 64, 0)  # swarm 1: seed 1, one bid lost
    fa = _fleet(lcs)
    lat = np.stack([lc.lat for lc in lcs])
    lat[0, 3, 7] = 0
    fa.latency.copy_(G._t(lat, np.uint8))
    fa.n_lost.fill_(7)
    fleets = [lc.fleet() for lc in lcs]
    cmd, q = GD._commands(lcs, {0: 0, 1: 0}, fleets)
    fa.run(DC.BUDGET, q=G._t(q, np.float64), cmd=G._t(cmd, np.uint8))
    st, nl = fa.status(), _n_lost(fa)
    assert tuple(st[0]) == (0, 0, 0, 0x4) and (nl[0] == 7).all()
    assert st[1]["ticks_run"] == 54 and nl[1].sum() == 7 * 13 + 1 and nl[1][8] == 8


def test_engine_rejections_and_workspaces_on_the_device():
    """FleetEpisode and FleetTrial take loss / loss_seed as FleetAuction does:
    a malformed one raises ValueError before anything runs, and a lossy
    object's workspace is the delay entry's."""
    import torch
    from aclswarm_amd import _lib as L
    from aclswarm_amd import engine
    sc = DC.draw("ring13").sc
    n, B = 13, 2
    T = G._table([sc])
    q = G._t(np.zeros((B, n, 3)), np.float64)
    fidx = G._t(np.zeros(B), np.int32)
    fseq = G._t(np.zeros((B, 1)), np.int32)
    m = torch.full((B, n, n), 64, dtype=torch.int16, device=q.device)
    bad = [dict(loss=-1), dict(loss=65536), dict(loss=True), dict(loss=0.5),
           dict(loss=m.to(torch.int32)), dict(loss=m[0]), dict(loss=m.transpose(1, 2)),
           dict(loss=m.cpu()), dict(loss_seed=3), dict(loss=64, loss_seed=-1),
           dict(loss=64, loss_seed=1.5), dict(loss=64, loss_seed=fidx.to(torch.int64)),
           dict(loss=64, loss_seed=fidx.cpu())]
    for kw in bad:
        with pytest.raises(ValueError):
            engine.FleetEpisode(T, fidx, q, q.clone(), **kw)
        with pytest.raises(ValueError):
            engine.FleetTrial(T, fseq, q, q.clone(), **kw)
    lib = L.lib()
    fe = engine.FleetEpisode(T, fidx, q, q.clone(), loss=m, loss_seed=5)
    assert fe.max_latency == 1 and fe.loss_seed.tolist() == [5, 6]
    assert fe.workspace_bytes() == lib.acl_fleet_delay_episode_workspace_bytes(n, B, 4 * n, 1)
    ft = engine.FleetTrial(T, fseq, q, q.clone(), loss=64, latency=3)
    assert ft.workspace_bytes() == lib.acl_fleet_delay_trial_workspace_bytes(n, B, 4 * n, 3)
    assert ft.ws.numel() == ft.workspace_bytes() and not ft.n_lost.any().item()
    for ob in (fe, ft):
        with pytest.raises(ValueError):
            ob.loss = 1 << 16
        with pytest.raises(ValueError):
            ob.loss_seed = 2.0
