"""CPU suite: the restatement of acl_fleet_delay_trial_batch
(tests/fleet_delay_trial_oracle.py). With every link at 1 tick it is
tests/fleet_trial_oracle.py record for record on every existing case; under
latency it shows what the cases file quotes: a trial that no longer completes,
adoptions that move, a formation change onto publications in flight."""
import numpy as np
import pytest

import fleet_auction_cases as C
import fleet_delay_trial_cases as D
import fleet_trial_cases as K
import trial_oracle as T


def _same(a, b, what):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same(a[k], b[k], f"{what}: {k}")
    elif a is None or b is None:
        assert a is None and b is None, what
    else:
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=what)


def _adopt(recs):
    return {s: len(v) for s, v in D.adoption_steps(recs).items()}


def _commits(recs):
    return [r["step"] for r in recs if r["committed"]]


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_all_links_at_one_tick_is_the_existing_restatement(name):
    """Every record of every step (floats bit for bit: the same arithmetic on
    the same numbers), the fleet's final state, the counters and the
    supervisor's record. What is in flight is counted by the model that holds
    it, so that one entry of a record is compared as a sum."""
    _, ref, want = K.cpu_run(name)
    cs, ft, got = D.cpu_run("ones", name)
    assert len(got) == len(want)
    for r, w in zip(got, want):
        what = f"{name} step {w['step']}"
        assert sum(r["before"]["inflight"]) == sum(w["before"]["inflight"]), what
        r = dict(r, before={k: v for k, v in r["before"].items() if k != "inflight"})
        w = dict(w, before={k: v for k, v in w["before"].items() if k != "inflight"})
        _same(r, w, what)
    _same(C.snapshot_state(ft.fleet), C.snapshot_state(ref.fleet), name)
    assert ft.fst == ref.fst and ft.fleet.tick == ref.fleet.tick
    assert ft.n_auctions == ref.n_auctions
    np.testing.assert_array_equal(ft.adopt_step, ref.adopt_step)
    np.testing.assert_array_equal(ft.q, ref.q)
    _same(ft.sup.record(), ref.sup.record(), name)


def test_interrupt6_no_auction_fits_its_period():
    _, ref, want = K.cpu_run("interrupt6")
    assert ref.sup.state == T.COMPLETE
    cs, ft, recs = D.cpu_run("interrupt6_draw")
    assert (ft.sup.state, ft.sup.last_state) == (T.TERMINATE, T.WAITING)
    assert _adopt(recs) == {} and not ft.t.ctl_on.any()
    f = ft.fst
    assert (f["n_started"], f["n_restarted"], f["n_consensus"]) == (42, 36, 0)
    assert ft.fleet.n_thrown.sum() == 79 and ft.n_auctions == 7
    assert ft.sup.done_step == len(recs) - 1 < cs.steps - 1


def test_interrupt13_under_the_draw():
    cs, ft, recs = D.cpu_run("interrupt13_draw")
    assert _adopt(recs) == {62: 13, 178: 13} and _commits(recs) == [21, 137]
    b = recs[137]["before"]
    assert b["open"].all() and b["queued"].sum() == 28
    assert ft.fleet.n_thrown.sum() == 28 > recs[136]["n_thrown"].sum() == 0
    assert (ft.sup.state, ft.t.fidx) == (T.COMPLETE, 1)


@pytest.mark.parametrize("lat,want", [(1, {38: 13, 71: 13}), (None, {42: 13, 74: 13}),
                                      (5, {46: 13, 79: 13})])
def test_chord_ring_ten_ticks_per_step_adoptions_move(lat, want):
    args = () if lat is None else (lat,)
    cs, ft, recs = D.cpu_run("chord13_t10", *args)
    assert _adopt(recs) == want
    assert ft.fst["n_restarted"] == 0 and ft.n_auctions == 2


@pytest.mark.parametrize("lat,want", [(1, {67: 5, 68: 4, 69: 4}), (None, {87: 1, 88: 6, 89: 6})])
def test_chord_ring_two_ticks_per_step_adoptions_move(lat, want):
    args = () if lat is None else (lat,)
    cs, ft, recs = D.cpu_run("chord13_t2", *args)
    assert _adopt(recs) == want
    pv = [r["step"] for r in recs if r["per_vehicle"]]
    assert pv == sorted(want)[:-1]  # mixed rows until the last group adopts
    assert ft.sup.state == T.FLYING


@pytest.mark.parametrize("lat,fly,queued,adopt", [
    (5, 9, 4, {127: 9, 128: 4}), (None, 14, 3, {106: 1, 107: 5, 108: 5, 109: 2})])
def test_formation_change_onto_publications_in_flight(lat, fly, queued, adopt):
    """The commit forced at step 40 finds every auctioneer open, bids queued
    and publications in flight. They stay in the logs through the commit and
    arrive over the following steps at closed auctioneers; the new formation's
    first auction throws 22 of them away."""
    args = () if lat is None else (lat,)
    cs, ft, recs = D.cpu_run("commit13", *args)
    assert _commits(recs) == [21, D.COMMIT13_AT]
    b = recs[D.COMMIT13_AT]["before"]
    assert b["open"].all() and sum(b["inflight"]) == fly and b["queued"].sum() == queued
    assert recs[D.COMMIT13_AT]["n_thrown"].sum() == 0 and not recs[D.COMMIT13_AT]["open"].any()
    assert recs[49]["n_thrown"].sum() == 0  # nobody is open until the auto-auction of step 50
    assert recs[49]["before"]["queued"].sum() > queued
    assert ft.fleet.n_thrown.sum() == 22
    assert _adopt(recs) == adopt
    assert ft.t.fidx == 1 and len(recs) == D.COMMIT13_STEPS


def test_ring65_under_the_draw():
    cs, ft, recs = D.cpu_run("ring65_draw")
    assert _adopt(recs) == {56: 2, 57: 7, 58: 12, 59: 13}
    assert ft.per_vehicle == 1 and [r["step"] for r in recs if r["per_vehicle"]] == [56, 57, 58, 59]


def test_near128_and_interrupt128_under_the_draw():
    cs, ft, recs = D.cpu_run("near128_draw")
    assert _adopt(recs) == {16: 23, 17: 13}
    assert (ft.fst["n_adopted"], ft.fst["n_invalid"]) == (36, 92) and ft.per_vehicle == 1
    cs, ft, recs = D.cpu_run("interrupt128_draw")
    b = recs[K.INTERRUPT128_AT]["before"]
    fly = np.array(b["inflight"])
    assert recs[K.INTERRUPT128_AT]["committed"] and b["open"].all()
    assert b["queued"].sum() == 15 and fly.sum() == 121 and fly[:64].any() and fly[64:].any()
    assert ft.t.fidx == 1 and ft.fleet.n_thrown.sum() == 174
