"""CPU suite: the restatement of acl_fleet_delay_episode_batch
(tests/fleet_delay_episode_oracle.py). With every link at 1 tick it is
tests/fleet_episode_oracle.py record for record on every existing case; under
latency it shows what the cases file quotes: later adoptions, auto-auctions
that restart open auctioneers with publications in flight, an auction that
never fits its period."""
import numpy as np
import pytest

import fleet_auction_cases as C
import fleet_auction_oracle as FO
import fleet_delay_episode_cases as D
import fleet_episode_cases as K

CLEAN = FO.V_CONSENSUS | FO.V_ADOPTED
BAD = FO.V_CONSENSUS | FO.V_INVALID


def _same(a, b, what):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same(a[k], b[k], f"{what}: {k}")
    elif a is None or b is None:
        assert a is None and b is None, what
    else:
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=what)


def _raised(recs):
    return {r["step"]: sorted(set(int(x) for x in r["raised"] if x)) for r in recs
            if r["raised"].any()}


def _consensus(recs):
    return {r["step"]: int(((r["raised"] & FO.V_CONSENSUS) != 0).sum()) for r in recs
            if (r["raised"] & FO.V_CONSENSUS).any()}


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_all_links_at_one_tick_is_the_existing_restatement(name):
    """Every record of every step (floats bit for bit: the same arithmetic on
    the same numbers), the fleet's final state and the counters."""
    _, ref, want = K.cpu_run(name)
    cs, ep, got = D.cpu_run("ones", name)
    assert len(got) == len(want) == cs.steps
    for r, w in zip(got, want):
        r = {k: v for k, v in r.items() if k != "before"}
        _same(r, w, f"{name} step {w['step']}")
    _same(C.snapshot_state(ep.fleet), C.snapshot_state(ref.fleet), name)
    assert ep.fst == ref.fst and ep.fleet.tick == ref.fleet.tick
    np.testing.assert_array_equal(ep.adopt_step, ref.adopt_step)
    np.testing.assert_array_equal(ep.q, ref.q)


def test_ring13_adopts_later_under_the_draw():
    _, ref, want = K.cpu_run("ring13")
    assert K.adoption_steps(want) == {7: 13, 19: 13}
    cs, ep, recs = D.cpu_run("ring13_draw")
    assert D.adoption_steps(recs) == {11: 13, 22: 13}
    assert _raised(recs) == {0: [FO.V_STARTED], 11: [CLEAN], 12: [FO.V_STARTED], 22: [CLEAN],
                             24: [FO.V_STARTED]}
    assert ep.fst["n_restarted"] == 0 and ep.fst["n_adopted"] == 26
    assert (ep.adopt_step == 22).all() and cs.max_lat == 5


def test_ring13_at_five_ticks_never_fits_its_period():
    """Every link at 5 ticks: an iteration takes 5 ticks and more, the 26
    iterations do not fit 120 ticks. The auto-auctions of steps 12 and 24
    restart 13 open auctioneers with 9 and 10 publications in flight."""
    cs, ep, recs = D.cpu_run("ring13_u5")
    assert D.adoption_steps(recs) == {} and _consensus(recs) == {}
    for s, fly in ((12, 9), (24, 10)):
        b = recs[s]["before"]
        assert b["open"].all() and sum(b["inflight"]) == fly
        assert (recs[s]["cmd"] == FO.START).all()
    assert (ep.fst["n_started"], ep.fst["n_restarted"]) == (39, 26)
    assert ep.fleet.n_thrown.sum() > 0 and ep.fst["ticks_run"] == 300
    assert (ep.adopt_step == -1).all()


def test_stale13_adopts_at_step_47_under_the_draw():
    _, ref, want = K.cpu_run("stale13")
    assert max(K.adoption_steps(want)) == 43
    cs, ep, recs = D.cpu_run("stale13_draw")
    assert D.adoption_steps(recs) == {47: 13}
    assert _raised(recs) == {0: [FO.V_STARTED], 12: [FO.V_STARTED], 23: [BAD],
                             36: [FO.V_STARTED], 47: [CLEAN]}
    f = ep.fst
    assert (f["n_started"], f["n_restarted"], f["n_flushed"], f["n_invalid"]) == (38, 12, 14, 13)
    assert (recs[24]["cmd"] == FO.FLUSH).all()


def test_restarts_with_start_bids_in_flight():
    """Every link at 8 ticks, an auto-auction every 6 ticks: no START bid has
    arrived when the next one restarts everybody. The bids stay in flight
    through the restarts: 13, 26, 35 publications at steps 3, 6, 9 (the first
    13 were delivered in step 4 and have left the logs)."""
    cs, ep, recs = D.cpu_run("restart13_u8")
    assert [sum(recs[s]["before"]["inflight"]) for s in (3, 6, 9)] == [13, 26, 35]
    assert all(recs[s]["before"]["open"].all() for s in (3, 6, 9))
    assert (ep.fst["n_started"], ep.fst["n_restarted"]) == (52, 39)
    assert ep.fst["n_consensus"] == 0 and ep.fst["ticks_run"] == 24
    # a sender's log holds at most 2 max_lat publications (the ring of the device)
    assert max(max(r["before"]["inflight"]) for r in recs) <= 2 * cs.max_lat


def test_rings12_under_the_draw():
    _, ref, want = K.cpu_run("rings12")
    assert sorted(_consensus(want)) == [4, 16]
    cs, ep, recs = D.cpu_run("rings12_draw")
    assert _raised(recs) == {0: [FO.V_STARTED], 10: [BAD], 12: [FO.V_STARTED], 22: [BAD],
                             24: [FO.V_STARTED]}
    f = ep.fst
    assert (f["n_started"], f["n_restarted"], f["n_flushed"]) == (23, 5, 13)
    assert f["n_adopted"] == 0 and f["n_invalid"] == 12


def test_ring65_consensus_spreads_over_several_steps():
    cs, ep, recs = D.cpu_run("ring65_draw")
    assert cs.max_iter == 32 and cs.steps == D.RING65_STEPS
    assert _consensus(recs) == D.RING65_CONSENSUS
    dt = ep.fleet.done_tick
    assert (int(dt.min()), int(dt.max())) == D.RING65_DONE_TICK
    f = ep.fst
    assert (f["n_consensus"], f["n_invalid"], f["n_adopted"]) == (65, 65, 0)
    assert f["ticks_run"] == D.RING65_TICKS and ep.fleet.quiescent()


def test_odd_last128_under_the_draw():
    cs, ep, recs = D.cpu_run("odd_last128_draw")
    assert cs.steps == 8 and cs.max_iter == 16 and cs.max_lat == 3
    f = ep.fst
    assert (f["n_consensus"], f["n_invalid"], f["n_adopted"]) == (128, 128, 0)
    assert ep.per_vehicle == 1 and all(r["per_vehicle"] for r in recs)
    assert sorted(_consensus(recs)) == [4, 5]
