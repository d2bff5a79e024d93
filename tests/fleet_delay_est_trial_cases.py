"""Cases of the trials on own estimates with tables on real links and the
encounter record (acl_fleet_delay_est_trial_batch), shared by
tests/test_fleet_delay_est_trial.py (CPU) and
tests/test_gpu_fleet_delay_est_trial.py. A case is one swarm: a
fleet_est_trial_cases.EstTrialCase (QUICK timings, forced commits) with the
table links of the swarm: tlat (an int or [n][n], receiver-major, rounds),
max_tlat, feed_loss (an int or [n]).

Every figure quoted below is what tests/fleet_delay_est_trial_oracle.py flew;
test_fleet_delay_est_trial.py asserts each.
  ring13_two at latency 2 on every link, track_every 2, forced commit at step
      14: the rounds of steps 14 and 16 deliver tables published in rounds 5
      and 6 (steps 10 and 12, under the first formation) to subscribers taken
      under the second formation's graph and the rows adopted at step 11
  crafted(n), n = 13 and 65: a chord ring whose vehicles start ON the
      formation's points, except that vehicle 1 starts 0.5 m from vehicle
      n - 1 and vehicle 2 the same 0.5 m from vehicle 3 (dyadic coordinates:
      both s2 are 0.25 bit for bit, a breach each, and the tie goes to pair
      (1, n - 1)); vehicle 4's feed is dead (it believes itself at the origin:
      once its controller runs, it is blind to its true neighbours and avoids
      ghosts near the origin); every link at 1 round. n = 13: everybody adopts
      at step 11; 48 breach, 10 blind and 7 ghost pair-steps in 16 steps.
      n = 65, max_iter 40: the first auction ends early, 10 vehicles adopt at
      step 13, 28 at step 14, 26 at step 15 and one never does, so steps 13 and
      14 run a strict subset of the controllers
"""
import functools

import numpy as np

import fleet_auction_cases as FA
import fleet_delay_est_trial_oracle as DXT
import fleet_delay_localize_cases as DC
import fleet_est_trial_cases as X
import fleet_localize_cases as GC
import fleet_loss_oracle as LO
import fleet_trial_cases as K
import helpers as H

RING13_COMMIT_AT = X.RING13_COMMIT_AT


class DelayEstTrialCase:
    """cs: an EstTrialCase; tlat: an int or [n][n]; feed: an int or [n]."""

    def __init__(self, cs, tlat=0, max_tlat=None, feed=0, name=None):
        self.cs, self.name = cs, name or cs.name
        n = cs.n
        t = np.asarray(tlat, np.int64)
        self.tlat = np.full((n, n), int(t)) if t.ndim == 0 else t.reshape(n, n).copy()
        self.max_tlat = int(self.tlat.max()) if max_tlat is None else int(max_tlat)
        f = np.asarray(feed, np.int64)
        self.feed = np.full(n, int(f)) if f.ndim == 0 else f.reshape(n).copy()

    def __getattr__(self, k):
        return getattr(self.cs, k)

    def oracle(self, diag=True, encounters=True):
        c = self.cs
        return DXT.DelayEstFleetTrial(c.fseq, c.forms, c.q, c.vel, c.tp, c.lat, loss=c.loss,
                                      seed=c.seed, max_iter=c.max_iter, ticks_per_step=c.T,
                                      track_every=c.track_every, diag=diag, tlat=self.tlat,
                                      max_tlat=self.max_tlat, feed_loss=self.feed,
                                      encounters=encounters)


def pair2():
    """n = 2: one edge, one unordered pair."""
    rng = np.random.RandomState(2)
    p = FA.points(rng, 2)
    adj = np.array([[0, 1], [1, 0]], np.uint8)
    form = (p, adj, H.synth_gains(np.random.RandomState(7), adj))
    return X.EstTrialCase("pair2", X._case("pair2", [form], [0], FA.snapshot(rng, 2), 14), 2)


def ring64_te2():
    """n = 64: the first lane slot exactly full."""
    sc = FA.clean_ring(64)
    return X.EstTrialCase("ring64_te2",
                          X._case("ring64_te2", [K._ring_form(sc)], [0], sc.windows[0][1], 6), 2)


def _dead(n, v):
    f = np.zeros(n, np.int64)
    f[v] = LO.DEAD
    return f


CRAFTED_MAX_ITER = {13: 0, 65: 40}
CRAFTED_STEPS = {13: 16, 65: 18}
CRAFTED_DEAD = 4


def crafted(n):
    """The crafted encounter case (the module's docstring)."""
    sc = FA.clean_ring(n)
    form = K._ring_form(sc)
    q = np.array(sc.p, np.float64).copy()
    q[:, :2] = np.round(q[:, :2] * 64.0) / 64.0  # dyadic: the differences below are exact
    q[1, :2] = q[n - 1, :2] + (0.5, 0.0)
    q[2, :2] = q[3, :2] - (0.5, 0.0)
    base = X.EstTrialCase(f"crafted{n}", X._case(f"crafted{n}", [form], [0], q, CRAFTED_STEPS[n],
                                                 max_iter=CRAFTED_MAX_ITER[n]), 2)
    return DelayEstTrialCase(base, 1, 1, _dead(n, CRAFTED_DEAD))


def ring13_two_lat2():
    return DelayEstTrialCase(X.case("ring13_two"), 2, 2, name="ring13_two_lat2")


def ring13_links(b, hi=2, max_tlat=2):
    """ring13_two under latencies drawn in 0..hi and vehicle 3 + b's feed dead."""
    return DelayEstTrialCase(X.case("ring13_two"), DC.tlat_draw(13, 900 + b, hi), max_tlat,
                             _dead(13, 3 + b), name=f"ring13_two_links{b}")


def ring13_loss_swarms():
    """ring13_two under fleet_localize_cases.loss_matrices13() (swarm 0) and
    under the thresholds 0 / 8192 / 0xFFFF on every link, latencies drawn in
    0..2, feed thresholds drawn from {0, 8192, 0xFFFF}."""
    ms, seeds = GC.loss_matrices13()
    out = []
    for b, (loss, seed) in enumerate([(ms[1], seeds[1]), (0, 0), (8192, 11), (LO.DEAD, 12)]):
        cs = X.EstTrialCase(f"ring13_two_l{b}", X.case("ring13_two").base, 2, loss, int(seed),
                            force={RING13_COMMIT_AT: K.force_commit})
        out.append(DelayEstTrialCase(cs, DC.tlat_draw(13, 920 + b, 2), 2,
                                     DC.feed_draw(13, 930 + b)))
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    if name in ("crafted13", "crafted65"):
        return crafted(int(name[7:]))
    if name == "ring13_two_lat2":
        return ring13_two_lat2()
    if name == "pair2":
        return DelayEstTrialCase(pair2(), 1, 1)
    if name == "ring64_te2":
        return DelayEstTrialCase(ring64_te2(), DC.tlat_draw(64, 940, 2), 2, _dead(64, 63))
    raise KeyError(name)


def fly(cs, ft, steps=None, delayed=True):
    """fleet_est_trial_cases.fly on a DelayEstFleetTrial; every record also
    holds q and vel before and after the step."""
    recs = []
    for s in range(cs.steps if steps is None else steps):
        if s in cs.force:
            cs.force[s](ft)
        q0, vel0 = ft.q.copy(), ft.vel.copy()
        r = ft.step(delayed=delayed)
        r["q0"], r["vel0"] = q0, vel0
        r["q"], r["vel"] = ft.q.copy(), ft.vel.copy()
        recs.append(r)
    return ft, recs


@functools.lru_cache(maxsize=None)
def cpu_run(name):
    """Shared by the tests, which leave it unchanged: (case, restatement, records)."""
    cs = case(name)
    ft, recs = fly(cs, cs.oracle())
    return cs, ft, recs
