"""CPU suite: the restatement of acl_fleet_lossy_trial_batch
(tests/fleet_loss_trial_oracle.py). With loss 0 it is
tests/fleet_delay_trial_oracle.py record for record; under loss an auction
stalls on one lost bid and the next auto-auction completes it, and under more
loss no auction completes and the assignment timeout ends the trial.

The trial restatement takes about 2 ms per step at n = 13 (10 ticks per step),
so the 225 steps of the timeout case take well under a second."""
import numpy as np
import pytest

import fleet_auction_cases as C
import fleet_delay_trial_cases as D
import fleet_loss_cases as LC
import test_fleet_delay_trial as TT
import trial_oracle as T

ZERO_CASES = ["interrupt13_draw", "chord13_t10"]


@pytest.mark.parametrize("name", ZERO_CASES)
@pytest.mark.parametrize("seed", [0, 0xDEADBEEF])
def test_loss_zero_is_the_delay_restatement(name, seed):
    _, ref, want = D.cpu_run(name)
    cs, ft, got = LC.cpu_trial(name, 0, seed)
    assert len(got) == len(want)
    for r, w in zip(got, want):
        assert r["lost"] == 0
        r = {k: v for k, v in r.items() if k != "lost"}
        TT._same(r, w, f"{name} step {w['step']}")
    TT._same(C.snapshot_state(ft.fleet), C.snapshot_state(ref.fleet), name)
    assert ft.fst == ref.fst and ft.fleet.tick == ref.fleet.tick
    assert ft.n_auctions == ref.n_auctions
    np.testing.assert_array_equal(ft.adopt_step, ref.adopt_step)
    np.testing.assert_array_equal(ft.q, ref.q)
    TT._same(ft.sup.record(), ref.sup.record(), name)
    assert not ft.fleet.n_lost.any()


def test_a_lost_bid_stalls_the_auction_until_the_next_auto_auction():
    """chord13_t10 under loss 64, seed 1. Without loss everybody adopts at
    steps 42 and 74. Here one bid is lost in step 34: nobody adopts at step
    42, the auto-auction of step 54 restarts 13 open auctioneers, and all
    adopt at step 75."""
    _, _, want = D.cpu_run("chord13_t10")
    assert TT._adopt(want) == {42: 13, 74: 13}
    cs, ft, recs = LC.cpu_trial("chord13_t10")
    assert (LC.TR_LOSS, LC.TR_SEED) == (64, 1)
    assert {r["step"]: r["lost"] for r in recs if r["lost"]} == {34: 1}
    assert TT._adopt(recs) == {75: 13}
    b = recs[54]["before"]
    assert b["open"].all() and sum(b["inflight"]) == 0 and not b["queued"].any()  # stalled
    assert ft.fst["n_restarted"] == 13 and ft.n_auctions == 2
    assert ft.fleet.n_lost.sum() == 1 and ft.t.ctl_on.all()


def test_loss_makes_the_assignment_timeout_end_the_trial():
    """chord13_timeout under loss 1024, seed 0: each of the 6 auctions loses a
    bid and stalls, every auto-auction restarts 13 open auctioneers, nobody
    ever adopts and the supervisor's assignment timeout ends the trial at step
    224. Without loss the same trial adopts at step 42."""
    cs = LC.trial("chord13_timeout", 0, 0)
    ft0, recs0 = D.fly(cs, cs.oracle())
    assert min(TT._adopt(recs0)) == 42 and ft0.sup.state != T.TERMINATE
    cs, ft, recs = LC.cpu_trial("chord13_timeout", LC.TIMEOUT_LOSS, LC.TIMEOUT_SEED)
    assert (ft.sup.state, ft.sup.last_state) == (T.TERMINATE, T.WAITING)
    assert TT._adopt(recs) == {} and not ft.t.ctl_on.any()
    assert len(recs) == 225 and ft.sup.done_step == 224 < cs.steps - 1
    assert ft.fst["n_restarted"] == 65 and ft.fst["n_consensus"] == 0 and ft.n_auctions == 6
    lost = {r["step"]: r["lost"] for r in recs if r["lost"]}
    assert sum(lost.values()) == ft.fleet.n_lost.sum() == 15
    # every auction period (an auto-auction every 33 steps from step 21) loses a bid
    assert {(s - 21) // 33 for s in lost} == set(range(6))
