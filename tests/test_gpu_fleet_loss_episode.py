"""GPU parity of acl_fleet_lossy_episode_batch (episodes on the message-level
auction with seeded per-link message loss) against the plain-Python
restatement tests/fleet_loss_episode_oracle.py, teacher-forced step for step
exactly as tests/test_gpu_fleet_delay_episode.py (whose loop, helpers and
tolerances these are; n_lost is compared after every step as well), and with
loss 0 against acl_fleet_delay_episode_batch on the same GPU."""
import numpy as np
import pytest

import fleet_auction_oracle as FO
import fleet_delay_episode_cases as D
import fleet_loss_cases as LC
import test_gpu_fleet_delay_episode as GE
from test_gpu_fleet_episode import CLEAN, _raised, _t, _u16

pytestmark = pytest.mark.gpu


def _lossy_episode(cases, **kw):
    """test_gpu_fleet_delay_episode._episode with the cases' loss matrices and
    seeds set through the attributes."""
    fe = _EPISODE(cases, **kw)
    fe.loss = _u16(np.stack([c.loss for c in cases]))
    fe.loss_seed = _t(np.array([c.seed for c in cases], np.uint32).view(np.int32), np.int32)
    return fe


_EPISODE = GE._episode


class _Checked:
    """A case whose restatement also compares n_lost with the device's after
    every step it flies."""

    def __init__(self, cs, b, held):
        self.cs, self.b, self.held = cs, b, held

    def __getattr__(self, k):
        return getattr(self.cs, k)

    def oracle(self):
        o = self.cs.oracle()
        step, b, held = o.step, self.b, self.held

        def checked(Rt=None, sup=None):
            r = step(Rt=Rt, sup=sup)
            np.testing.assert_array_equal(held["fe"].n_lost.cpu().numpy()[b], o.fleet.n_lost,
                                          err_msg=f"{self.cs.name} step {r['step']}: n_lost")
            return r
        o.step = checked
        return o


def _teacher_forced(cases, steps, monkeypatch):
    held = {}

    def build(cs, **kw):
        held["fe"] = _lossy_episode(cs, **kw)
        return held["fe"]
    monkeypatch.setattr(GE, "_episode", build)
    return GE._teacher_forced([_Checked(c, b, held) for b, c in enumerate(cases)], steps)


def test_parity_a_lost_bid_and_the_restart_that_recovers(monkeypatch):
    """ring13/draw2 under loss 64: seed 1 loses a bid in step 3, stalls, is
    restarted at step 12 and adopts at step 23; seed 0 loses nothing before
    its adoption at step 11 (one bid each in steps 17 and 24 afterwards)."""
    cases = [LC.episode("ring13_draw"), LC.episode("ring13_draw", 64, 0)]
    fe, oracles, recs, hists = _teacher_forced(cases, 30, monkeypatch)
    assert {s: r[0]["lost"] for s, r in enumerate(recs) if r[0]["lost"]} == {3: 1}
    assert {s: r[1]["lost"] for s, r in enumerate(recs) if r[1]["lost"]} == {17: 1, 24: 1}
    assert _raised(hists, 0) == {0: [FO.V_STARTED], 12: [FO.V_STARTED], 23: [CLEAN],
                                 24: [FO.V_STARTED]}
    assert _raised(hists, 1)[11] == [CLEAN]
    before = recs[12][0]["before"]
    assert before["open"].all() and sum(before["inflight"]) == 0
    st = fe.status()["fleet"]
    assert (st[0]["n_restarted"], st[0]["n_adopted"]) == (13, 13)
    assert fe.n_lost.cpu().numpy().sum(axis=1).tolist() == [1, 2]


def test_parity_ring65_under_loss(monkeypatch):
    """n = 65 (the second wave, the second mask word), loss 64, seed 1: bids
    lost in steps 4, 7, 9 and 13; 10 vehicles reach consensus, 55 stay open."""
    cs = LC.episode_ring65()
    fe, oracles, recs, hists = _teacher_forced([cs], cs.steps, monkeypatch)
    assert {s: r[0]["lost"] for s, r in enumerate(recs) if r[0]["lost"]} == {4: 1, 7: 1, 9: 1,
                                                                            13: 1}
    f = fe.status()["fleet"][0]
    assert f["n_consensus"] == 10 and fe.open.cpu().numpy().sum() == 55


@pytest.mark.parametrize("names,steps,cuts", [(("ring13_draw", "stale13_draw"), 48, (12, 36)),
                                              (("restart13_u8",), 12, (5,))])
def test_loss_zero_equals_the_delay_entry(names, steps, cuts):
    """acl_fleet_lossy_episode_batch with loss 0 against
    acl_fleet_delay_episode_batch on the same GPU, flown in the same chunks:
    every state array and every history equal; n_lost stays 0."""
    import torch
    cases = [D.case(n) for n in names]
    want, hist0 = GE._flown(cases, steps, cuts)
    lossy = [LC.LossyEpisodeCase(c, 0, 0xDEADBEEF + b) for b, c in enumerate(cases)]
    fe = _lossy_episode(lossy)
    hs = []
    edges = [0] + list(cuts) + [steps]
    for a, b in zip(edges[:-1], edges[1:]):
        GE._write_q(fe, cases, a)
        hs.append(fe.run(b - a, history=True))
    torch.cuda.synchronize()
    got = GE._state(fe)
    for k in want:
        np.testing.assert_array_equal(GE._bits(got[k]), GE._bits(want[k]), err_msg=k)
    for k in hist0:
        np.testing.assert_array_equal(torch.cat([h[k] for h in hs]).cpu().numpy(), hist0[k],
                                      err_msg=k)
    assert not fe.n_lost.cpu().numpy().any()
