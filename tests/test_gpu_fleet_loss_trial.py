"""GPU parity of acl_fleet_lossy_trial_batch (trials on the message-level
auction with seeded per-link message loss) against the plain-Python
restatement tests/fleet_loss_trial_oracle.py, teacher-forced step for step
exactly as tests/test_gpu_fleet_delay_trial.py (whose loop, helpers and
tolerances these are; n_lost is compared after every step as well), and with
loss 0 against acl_fleet_delay_trial_batch on the same GPU."""
import numpy as np
import pytest

import fleet_delay_trial_cases as D
import fleet_loss_cases as LC
import fleet_loss_trial_oracle as LT
import test_gpu_fleet_delay_trial as GT
import trial_oracle as T
from test_gpu_fleet_trial import _state, _t, _u16

pytestmark = pytest.mark.gpu


def _loss_batch(cases):
    """test_gpu_fleet_delay_trial._lat_batch and the swarms' loss matrices and seeds."""
    bt = GT._lat_batch(cases)
    bt["loss"] = np.stack([c.loss for c in cases])
    bt["seed"] = np.array([c.seed for c in cases], np.uint32)
    return bt


_TRIAL = GT._trial


def _lossy_trial(bt):
    ft = _TRIAL(bt)
    ft.loss = _u16(bt["loss"])
    ft.loss_seed = _t(bt["seed"].view(np.int32), np.int32)
    return ft


def _teacher_forced(cases, steps, monkeypatch):
    """GT._teacher_forced on the lossy entry and restatement; every
    restatement's step also compares n_lost with the device's."""
    bt = _loss_batch(cases)
    held = {}

    def trial(b_):
        held["ft"] = _lossy_trial(b_)
        return held["ft"]

    def oracles(b_):
        c0 = b_["case"]
        out = []
        for b in range(len(b_["fseq"])):
            o = LT.LossyFleetTrial(b_["fseq"][b], b_["forms"], b_["q"][b], b_["vel"][b], c0.tp,
                                   b_["lat"][b], loss=b_["loss"][b], seed=int(b_["seed"][b]),
                                   max_iter=c0.max_iter, ticks_per_step=c0.T)

            def checked(Rt=None, sup=None, o=o, b=b, step=o.step):
                r = step(Rt=Rt, sup=sup)
                np.testing.assert_array_equal(held["ft"].n_lost.cpu().numpy()[b], o.fleet.n_lost,
                                              err_msg=f"swarm {b} step {r['step']}: n_lost")
                return r
            o.step = checked
            out.append(o)
        return out
    monkeypatch.setattr(GT, "_trial", trial)
    monkeypatch.setattr(GT, "_oracles", oracles)
    return GT._teacher_forced(bt, steps)


def test_parity_a_lost_bid_and_the_restart_that_recovers(monkeypatch):
    """chord13_t10 under loss 64: seed 1 loses a bid in step 34, stalls, is
    restarted by the auto-auction of step 54 and adopts at step 75; seed 0
    adopts at step 42 as without loss (a bid lost in step 69 stalls its second
    auction)."""
    cases = [LC.trial("chord13_t10"), LC.trial("chord13_t10", 64, 0)]
    ft, oracles, recs, hists = _teacher_forced(cases, 78, monkeypatch)
    assert {s: r[0]["lost"] for s, r in enumerate(recs) if r[0]["lost"]} == {34: 1}
    assert {s: r[1]["lost"] for s, r in enumerate(recs) if r[1]["lost"]} == {69: 1}
    assert GT._n_adopt(hists, 0) == {75: 13} and GT._n_adopt(hists, 1) == {42: 13}
    before = recs[54][0]["before"]
    assert before["open"].all() and sum(before["inflight"]) == 0
    fl = ft.fleet_status()["fleet"]
    assert (fl[0]["n_restarted"], fl[1]["n_restarted"]) == (13, 0)
    assert ft.n_lost.cpu().numpy().sum(axis=1).tolist() == [1, 1]


def test_parity_loss_ends_the_trial_by_the_assignment_timeout(monkeypatch):
    """chord13_timeout under loss 1024, seed 0: every auction stalls on a lost
    bid; TERMINATE through the assignment timeout at step 224, flown two steps
    past the trial's end."""
    cs = LC.trial("chord13_timeout", LC.TIMEOUT_LOSS, LC.TIMEOUT_SEED)
    ft, oracles, recs, hists = _teacher_forced([cs], 227, monkeypatch)
    st, fl = ft.status()[0], ft.fleet_status()["fleet"][0]
    assert (st["state"], st["last_state"], st["done_step"]) == (T.TERMINATE, T.WAITING, 224)
    assert (fl["n_restarted"], fl["n_adopted"], fl["n_consensus"]) == (65, 0, 0)
    assert ft.n_lost.cpu().numpy().sum() == 15 and not ft.ctl_on.cpu().numpy().any()


@pytest.mark.parametrize("name,steps,cut", [("interrupt13_draw", 150, 60), ("chord13_t10", 78, 40)])
def test_loss_zero_equals_the_delay_entry(name, steps, cut):
    """acl_fleet_lossy_trial_batch with loss 0 against
    acl_fleet_delay_trial_batch on the same GPU, both flown as two calls:
    every state array and every history equal; n_lost stays 0."""
    import torch
    cs = D.case(name)
    bt = _loss_batch([LC.LossyTrialCase(cs, 0, 0xDEADBEEF)])
    old, new = _TRIAL(bt), _lossy_trial(bt)
    hs = {id(ft): [ft.run(cut, history=True), ft.run(steps - cut, history=True)]
          for ft in (old, new)}
    so, sn = _state(old), _state(new)
    for k in so:
        np.testing.assert_array_equal(GT._bits(sn[k]), GT._bits(so[k]), err_msg=k)
    for k in hs[id(old)][0]:
        a, b = (torch.cat([h[k] for h in hs[id(ft)]]).cpu().numpy() for ft in (old, new))
        np.testing.assert_array_equal(a, b, err_msg=k)
    assert not new.n_lost.cpu().numpy().any()
    assert (so["adopt_step"] >= 0).all()
