"""GPU parity of acl_fleet_delay_est_episode_batch (the closed loop on own
estimates whose gossip round is acl_fleet_delay_localize_batch's) against the
composed restatement tests/fleet_delay_est_episode_oracle.py.

The comparison is tests/test_gpu_fleet_est_episode.py's own, teacher-forced
step by step (its _teacher_forced, with its bars: every fleet state and output
array, the trackers, xst and the error record bit for bit, u within 1e-5
relative, CA flags exact, q / vel within 1e-9), flown on the new entry; beside
it n_missed, exact. Then chunked calls against step by step, and the reduction
to acl_fleet_est_episode_batch on the same GPU, byte for byte."""
import functools

import numpy as np
import pytest

import fleet_delay_est_episode_oracle as DXO
import fleet_delay_localize_cases as DC
import fleet_est_episode_cases as X
import fleet_loss_oracle as LO
import test_gpu_fleet_est_episode as GE
from test_gpu_fleet_episode import _bits, _t, _u16

pytestmark = pytest.mark.gpu


class _Case:
    """An fleet_est_episode_cases.EstCase with the table links of one swarm."""

    def __init__(self, cs, tlat, max_tlat, feed):
        self.cs, self.tlat, self.max_tlat = cs, np.asarray(tlat), max_tlat
        self.feed = np.asarray(feed)

    def __getattr__(self, k):
        return getattr(self.cs, k)

    def oracle(self, queue_cap=None, diag=True):
        cs = self.cs.cs
        ep = DXO.DelayEstFleetEpisode(cs.p, cs.adj, cs.gains, cs.q0, cs.vel0, cs.ep, cs.lat,
                                      loss=self.loss, seed=self.seed, Pt=cs.Pt,
                                      queue_cap=queue_cap, max_iter=cs.max_iter,
                                      ticks_per_step=cs.T, track_every=self.track_every,
                                      diag=diag, tlat=self.tlat, max_tlat=self.max_tlat,
                                      feed_loss=self.feed)
        for v in cs.invalid0:
            ep.fleet.invalid[v] = 1
        return ep


@pytest.fixture
def on_the_new_entry(monkeypatch):
    """Makes test_gpu_fleet_est_episode._episode build its FleetEstEpisode with
    the table links of the cases it is given."""
    from aclswarm_amd import engine
    plain = GE._episode
    cls = engine.FleetEstEpisode

    def episode(cases, **kw):
        links = dict(table_latency=_t(np.stack([c.tlat for c in cases]), np.uint8),
                     max_table_latency=cases[0].max_tlat,
                     feed_loss=_u16(np.stack([c.feed for c in cases])))
        monkeypatch.setattr(engine, "FleetEstEpisode", functools.partial(cls, **links))
        try:
            return plain(cases, **kw)
        finally:
            monkeypatch.setattr(engine, "FleetEstEpisode", cls)
    monkeypatch.setattr(GE, "_episode", episode)


def _ring13(B=4):
    """ring13 at track_every 2, loss 0, 0, 64 and 4096: latencies drawn in 0..2,
    vehicle 3 + b of swarm b with a dead feed, a drawn outage on swarm 3."""
    names = ("ring13_te2", "ring13_te2", "ring13_loss64", "ring13_loss4096")[:B]
    out = []
    for b, name in enumerate(names):
        feed = np.zeros(13, np.int64)
        feed[3 + b] = LO.DEAD
        if b == 3:
            feed[9:] = 8192
        out.append(_Case(X.case(name), DC.tlat_draw(13, 700 + b, 2), 2, feed))
    return out


def _missed(fe, oracles):
    got = fe.n_missed.cpu().numpy()
    for b, o in enumerate(oracles):
        np.testing.assert_array_equal(got[b], o.trackers.n_missed, err_msg=f"swarm {b}")
    return got


def test_parity_ring13_under_table_latency_and_a_dead_feed(on_the_new_entry):
    cases = _ring13()
    steps = 26
    fe, oracles, recs, hists = GE._teacher_forced(cases, steps)
    got = _missed(fe, oracles)
    assert [got[b, 3 + b] for b in range(4)] == [steps // 2] * 4 and got[3, 9:].sum() > 0
    st = fe.loc_stamp.cpu().numpy()
    for b in range(4):  # nobody ever hears of the vehicle whose feed is dead
        assert (st[b][:, 3 + b] == 0).all()
    x = fe.status()["estimates"]
    assert x["rounds_run"].tolist() == [steps // 2] * 4 and (x["n_unknown"] >= 13).all()
    # a vehicle whose feed is dead believes itself where its table began: at the origin
    assert (x["err2_own"] > 0.0).all()
    print("err2 (m^2):", [[float(x[b][k]) for k in GE.XERR] for b in range(4)],
          "adopted:", fe.status()["fleet"]["n_adopted"].tolist())


def test_parity_ring65(on_the_new_entry):
    """n = 65, B = 2: the localize kernel's other wave count under the loop."""
    feed = np.zeros(65, np.int64)
    feed[64] = LO.DEAD
    cases = [_Case(X.case("ring65_te2"), DC.tlat_draw(65, 710 + b, 2), 2, feed) for b in range(2)]
    fe, oracles, recs, hists = GE._teacher_forced(cases, 6)
    got = _missed(fe, oracles)
    assert got[:, 64].tolist() == [3, 3] and got[:, :64].sum() == 0
    assert fe.status()["estimates"]["rounds_run"].tolist() == [3, 3]


def test_chunks_equal_step_by_step(on_the_new_entry):
    """26 steps as one call per step, as one call, and as 11 + 15 (a cut
    between two rounds, tables in flight across it): state, trackers, xst,
    n_missed, the log and the histories bit for bit."""
    import torch
    cases = _ring13()

    def flown(cuts):
        fe = GE._episode(cases)
        hs = []
        edges = [0] + list(cuts) + [26]
        for a, b in zip(edges[:-1], edges[1:]):
            hs.append(fe.run(b - a, history=True))
        torch.cuda.synchronize()
        d = GE._state(fe)
        d["n_missed"], d["log"] = fe.n_missed.cpu().numpy(), fe.loc_ws.cpu().numpy()
        return d, {k: torch.cat([h[k] for h in hs]).cpu().numpy() for k in hs[0]}
    ref = flown(range(1, 26))
    for cuts in ((), (11,)):
        got = flown(cuts)
        for x, y in zip(ref, got):
            assert x.keys() == y.keys()
            for k in x:
                np.testing.assert_array_equal(_bits(x[k]), _bits(y[k]), err_msg=k)
    assert ref[1]["err2"].any() and ref[0]["n_missed"].sum() > 0


@pytest.mark.parametrize("names,steps,cut", [(("ring13_te2", "ring13_loss4096"), 16, 7),
                                             (("ring65_te2",), 6, 3)])
def test_latency_zero_equals_the_est_episode_entry(names, steps, cut):
    """The reduction on the same GPU, byte for byte: table_latency 0 and no
    feed_loss against acl_fleet_est_episode_batch, two calls each."""
    import torch
    from aclswarm_amd import engine
    cases = [X.case(k) for k in names]
    old = GE._episode(cases)
    cls = engine.FleetEstEpisode
    try:
        engine.FleetEstEpisode = functools.partial(cls, table_latency=0, max_table_latency=2)
        new = GE._episode(cases)
    finally:
        engine.FleetEstEpisode = cls
    assert new.table_latency is not None and old.table_latency is None
    for k in (cut, steps - cut):
        ho, hn = old.run(k, history=True), new.run(k, history=True)
        a, b = GE._state(old), GE._state(new)
        for key in GE.XSTATE:
            np.testing.assert_array_equal(_bits(a[key]), _bits(b[key]), err_msg=key)
        assert ho.keys() == hn.keys()
        for key in ho:
            assert torch.equal(ho[key], hn[key]), key
    assert not new.n_missed.any().item() and new.loc_ws is not None and old.loc_ws is None
    assert old.status()["estimates"]["rounds_run"].tolist() == [steps // 2] * len(cases)


def test_python_argument_errors():
    from aclswarm_amd import engine
    cs = X.case("ring13_te2")
    fe = GE._episode([cs])

    def make(**kw):
        return engine.FleetEstEpisode(fe.table, fe.fidx, fe.q, fe.vel, **kw)
    for kw in (dict(table_latency=8), dict(table_latency=-1), dict(table_latency=1.5),
               dict(table_latency=2, max_table_latency=1), dict(max_table_latency=8),
               dict(feed_loss=65536), dict(feed_loss=-1),
               dict(table_latency=fe.latency[0]), dict(feed_loss=fe.loss_seed)):
        with pytest.raises(ValueError):
            make(**kw)
    ok = make(table_latency=1, feed_loss=0xFFFF)
    assert ok.max_table_latency == 1 and ok.loc_ws is None and not ok.n_missed.any().item()
    ok.run(3)
    assert ok.n_missed.cpu().numpy().tolist() == [[2] * 13]  # rounds at steps 0 and 2
    assert not ok.loc_stamp.any().item()
