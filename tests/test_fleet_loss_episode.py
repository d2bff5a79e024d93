"""CPU suite: the restatement of acl_fleet_lossy_episode_batch
(tests/fleet_loss_episode_oracle.py). With loss 0 it is
tests/fleet_delay_episode_oracle.py record for record; under loss an auction
stalls on one lost bid and the next auto-auction's restart completes it."""
import numpy as np
import pytest

import fleet_auction_cases as C
import fleet_auction_oracle as FO
import fleet_delay_episode_cases as D
import fleet_loss_cases as LC
import test_fleet_delay_episode as TE

ZERO_CASES = ["ring13_draw", "restart13_u8"]


@pytest.mark.parametrize("name", ZERO_CASES)
@pytest.mark.parametrize("seed", [0, 0xDEADBEEF])
def test_loss_zero_is_the_delay_restatement(name, seed):
    """Every record of every step (floats bit for bit), the fleet's final
    state and the counters; nothing is counted as lost."""
    _, ref, want = D.cpu_run(name)
    cs, ep, got = LC.cpu_episode(name, 0, seed)
    assert len(got) == len(want) == cs.steps
    for r, w in zip(got, want):
        assert r["lost"] == 0
        r = {k: v for k, v in r.items() if k != "lost"}
        TE._same(r, w, f"{name} step {w['step']}")
    TE._same(C.snapshot_state(ep.fleet), C.snapshot_state(ref.fleet), name)
    assert ep.fst == ref.fst and ep.fleet.tick == ref.fleet.tick
    np.testing.assert_array_equal(ep.adopt_step, ref.adopt_step)
    np.testing.assert_array_equal(ep.q, ref.q)
    assert not ep.fleet.n_lost.any()


def test_a_lost_bid_stalls_the_auction_until_the_next_auto_auction():
    """ring13/draw2 under loss 64, seed 1. Without loss everybody adopts at
    steps 11 and 22. Here one bid is lost in step 3: nobody reaches consensus
    in the first period, the auto-auction of step 12 restarts 13 open and
    quiescent auctioneers, and that auction completes at step 23."""
    _, _, want = D.cpu_run("ring13_draw")
    assert D.adoption_steps(want) == {11: 13, 22: 13}
    cs, ep, recs = LC.cpu_episode("ring13_draw")
    assert (LC.EP_LOSS, LC.EP_SEED) == (64, 1)
    assert {r["step"]: r["lost"] for r in recs if r["lost"]} == {3: 1}
    assert D.adoption_steps(recs) == {23: 13}
    b = recs[12]["before"]
    assert b["open"].all() and sum(b["inflight"]) == 0 and not b["queued"].any()  # stalled
    assert (recs[12]["cmd"] == FO.START).all()
    assert TE._raised(recs) == {0: [FO.V_STARTED], 12: [FO.V_STARTED], 23: [TE.CLEAN],
                                24: [FO.V_STARTED]}
    f = ep.fst
    assert (f["n_started"], f["n_restarted"], f["n_adopted"]) == (39, 13, 13)
    assert ep.fleet.n_lost.sum() == 1 and (ep.adopt_step == 23).all()


def test_ring65_under_loss():
    """ring65/draw under loss 64, seed 1 (the n = 65 GPU case): bids are lost
    in steps 4, 7, 9 and 13; 10 vehicles reach consensus, 55 stay open."""
    cs, ep, recs = LC.cpu_episode("ring65_draw", LC.RING65_EP_LOSS, LC.RING65_EP_SEED)
    assert {r["step"]: r["lost"] for r in recs if r["lost"]} == {4: 1, 7: 1, 9: 1, 13: 1}
    assert ep.fst["n_consensus"] == 10 and ep.fleet.open.sum() == 55
    assert ep.fleet.n_lost.sum() == 4 and ep.fst["ticks_run"] == 143
