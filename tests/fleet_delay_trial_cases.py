"""Cases of the trials with per-link message latency
(acl_fleet_delay_trial_batch), shared by tests/test_fleet_delay_trial.py (CPU)
and tests/test_gpu_fleet_delay_trial.py: a case of tests/fleet_trial_cases.py
(or the chord ring of 13 flown as a trial) and a latency matrix with a
committed seed (fleet_delay_cases.lat_draw / lat_uniform). A case is one swarm.

Every figure quoted below is what tests/fleet_delay_trial_oracle.py ran;
test_fleet_delay_trial.py asserts each.
  interrupt6/draw5   complete graph, 2 ticks per step, an auto-auction every
                     31 steps: no auction ever fits its period (the trial
                     completes at latency 1). TERMINATE through the assignment
                     timeout, 36 restarts, 79 thrown bids, no adoption
  interrupt13/draw5  reassign(13), 10 ticks per step, every 33 steps
  chord13_t10/draw2  the chord ring of 13, 10 ticks per step, every 33 steps:
                     adoptions at steps 42 and 74 (38 and 71 at latency 1, 46
                     and 79 with every link at 5 ticks)
  chord13_t2/draw2   2 ticks per step, every 80 steps: adoptions at steps
                     87-89 (67-69 at latency 1)
  commit13/u5, /draw2  two formations on that ring, 2 ticks per step, a commit
                     forced at step 40 onto 13 open auctioneers with 9 (14)
                     publications in flight and 3-4 queued bids; the old
                     auction's bids arrive over the following steps and 22 are
                     thrown away in the new formation's auction; adoptions at
                     steps 127-128 (106-109), fidx ends at 1
  ring65/draw        adoptions over steps 56-59, per-vehicle rows in between
  near128/draw       links at 1..3 ticks: 36 vehicles adopt at steps 16-17,
                     92 flag INVALID
  interrupt128/draw  near128 and a commit forced after three steps
"""
import functools

import fleet_auction_cases as FA
import fleet_delay_cases as DC
import fleet_delay_trial_oracle as DT
import fleet_trial_cases as K
import numpy as np
import trial_cases as TC

SEED6, SEED13 = 5, 5    # lat_draw(6, 5, 1, 5), lat_draw(13, 5, 1, 5): the interrupt cases
SEED_RING13 = 2         # lat_draw(13, 2, 1, 5): the chord ring of 13
SEED65 = 65001          # lat_draw(65, 65001, 1, 4)
SEED128 = 128001        # lat_draw(128, 128001, 1, 3)

COMMIT13_AT = 40        # the forced commit of commit13
COMMIT13_STEPS = 150


class DelayCase:
    """base: a fleet_trial_cases.Case (its own copy); lat [n][n] u8; force:
    {step: f(restatement)} applied before that step."""

    def __init__(self, name, base, lat, steps=None, force=None, max_lat=None):
        self.name, self.base, self.n = name, base, base.n
        self.forms, self.fseq, self.q, self.vel = base.forms, base.fseq, base.q, base.vel
        self.T, self.max_iter = base.T, base.max_iter
        self.tp_over, self.ep_over = base.tp_over, base.ep_over
        self.steps = base.steps if steps is None else steps
        self.force = dict(force or {})
        self.lat = np.ascontiguousarray(lat, np.uint8).reshape(self.n, self.n)
        self.max_lat = int(self.lat.max()) if max_lat is None else int(max_lat)

    @property
    def tp(self):
        return self.base.tp

    def oracle(self, lat=None):
        return DT.DelayFleetTrial(self.fseq, self.forms, self.q, self.vel, self.tp,
                                  self.lat if lat is None else lat, max_iter=self.max_iter,
                                  ticks_per_step=self.T)


def interrupt6_draw():
    return DelayCase("interrupt6/draw5", K.interrupt6(), DC.lat_draw(6, SEED6, 1, 5))


def interrupt13_draw():
    return DelayCase("interrupt13/draw5", K.interrupt13(), DC.lat_draw(13, SEED13, 1, 5))


def _chord13(name, steps, ticks_per_step, auction_every, two=False):
    """The chord ring of 13 (fleet_trial_cases.stagger13_t2's formation) as a
    trial; two: a second formation, the first one scaled."""
    sc = FA.clean_ring(13)
    forms = [K._ring_form(sc)]
    if two:
        forms.append((TC._scaled(sc.p, 1.04), sc.adj, forms[0][2]))
    return K.Case(name, forms, list(range(len(forms))), sc.windows[0][1], steps, ticks_per_step,
                  ep=dict(auction_every=auction_every))


def chord13_t10(lat=None):
    """lat None: the draw; an int: every link at that many ticks."""
    lat = DC.lat_draw(13, SEED_RING13, 1, 5) if lat is None else DC.lat_uniform(13, lat)
    return DelayCase("chord13_t10", _chord13("chord13_t10", 82, 10, 33), lat)


def chord13_t2(lat=None):
    lat = DC.lat_draw(13, SEED_RING13, 1, 5) if lat is None else DC.lat_uniform(13, lat)
    return DelayCase("chord13_t2", _chord13("chord13_t2", 92, 2, 80), lat)


def commit13(lat=None):
    lat = DC.lat_draw(13, SEED_RING13, 1, 5) if lat is None else DC.lat_uniform(13, lat)
    return DelayCase("commit13", _chord13("commit13", COMMIT13_STEPS, 2, 80, two=True), lat,
                     force={COMMIT13_AT: K.force_commit})


def ring65_draw():
    return DelayCase("ring65/draw", K.ring65(), DC.lat_draw(65, SEED65, 1, 4))


def near128_draw():
    return DelayCase("near128/draw", K.near128(), DC.lat_draw(128, SEED128, 1, 3))


def interrupt128_draw():
    return DelayCase("interrupt128/draw", K.interrupt128(), DC.lat_draw(128, SEED128, 1, 3),
                     force={K.INTERRUPT128_AT: K.force_commit})


def ones(name):
    """An existing case with every link at 1 tick: today's model step for step."""
    base = K.CASES[name]()
    force = {K.INTERRUPT128_AT: K.force_commit} if name == "interrupt128" else None
    return DelayCase(f"{name}/ones", base, DC.lat_uniform(base.n, 1), force=force)


@functools.lru_cache(maxsize=None)
def case(name, *args):
    return globals()[name](*args)


def fly(cs, ft=None):
    """A case flown on the restatement alone (the CPU oracle's alignments)
    until the trial ends or the case's steps are up, as
    fleet_trial_cases.cpu_run flies its cases. Returns (restatement, records)."""
    ft = cs.oracle() if ft is None else ft
    recs = []
    for s in range(cs.steps):
        if s in cs.force:
            cs.force[s](ft)
        recs.append(ft.step())
        if ft.t.done:
            break
    return ft, recs


@functools.lru_cache(maxsize=None)
def cpu_run(name, *args):
    """Shared by the tests, which leave it unchanged: (case, restatement, records)."""
    cs = case(name, *args)
    ft, recs = fly(cs)
    return cs, ft, recs


adoption_steps = K.adoption_steps
