"""Cases of the trials on each vehicle's own estimates
(acl_fleet_est_trial_batch), shared by tests/test_fleet_est_trial.py (CPU) and
tests/test_gpu_fleet_est_trial.py. A case is one swarm: a
fleet_trial_cases.Case with QUICK timings (the first formation commits at step
3, its first auction starts at step 4), every link at 1 tick, a loss matrix and
seed as tests/fleet_loss_cases.py takes them, track_every, and forced commits
(fleet_trial_cases.force_commit) at fixed steps, so that no case flies a swarm
to convergence. The restatements record the error figures (diag).

Every figure quoted below is what tests/fleet_est_trial_oracle.py flew;
test_fleet_est_trial.py asserts each.
  single          n = 1, K = 1, 8 steps: a lone vehicle hears no bid and never
                  adopts; 8 rounds, the error record is three zeros
  sync6_complete  n = 6, complete graphs, track_every 1, loss 0: the lossy
                  trial record for record (reduction (b)); adoptions at steps
                  9 and 18, the second formation commits at step 12 (forced)
  ring13_one      K = 1, chord ring, random start, track_every 2: loc_rows
                  equal the auctioneers' rows at every step (reduction (a));
                  adoption at step 11 on a table that is not the identity, 11
                  CA vehicle-steps of running controllers in 22 steps
  ring13_two      vehicles 2 and 4 start at each other's points: the first
                  adoption (step 11) installs rows that are not the identity
                  (the auction exchanges vehicles 3 and 5). The second
                  formation, on another chord ring (chords 3-9 and 5-11) with
                  the points scaled by 1.04, commits at step 14 (forced); its
                  auction starts at step 15 and is adopted at step 22. In
                  between the tables travel over (new graph, old assignment)
  ring13_two_loss the same under loss 4096, seed 5, 20 steps: 19 tables and 9
                  bids lost; both auctions stall on a lost bid, nobody adopts
                  and loc_rows stay the identity across the commit
  rings12_two     two disjoint rings: 72 entries unknown for the whole flight,
                  every auction INVALID, nobody adopts, loc_rows stay the
                  identity; the second formation commits at step 10 (forced)
  ring65_te2      the second wave with one live lane, 12 steps, 3 236 entries
                  unknown at the end
  near128_two     both entry slots of every lane; max_iter 40 is below the
                  graph's diameter, so only the vehicles near the chords adopt
                  (9 at step 14, 27 at step 15): the loc_rows copy runs for a
                  strict subset of the vehicles in both halves of the lane
                  range; the second formation commits at step 17 (forced)
"""
import functools

import numpy as np

import fleet_auction_cases as FA
import fleet_delay_cases as DC
import fleet_est_control_oracle as EC
import fleet_est_trial_oracle as XT
import fleet_loss_oracle as LO
import fleet_loss_trial_oracle as LT
import fleet_trial_cases as K
import helpers as H
import pyoracle as O
import trial_cases as TC

D_MARGIN, ANGLE_MARGIN = 1e-6, 1e-4  # the input condition of the collision decisions
GOSSIP_LOSS, GOSSIP_SEED = 4096, 5

SYNC6_COMMIT_AT = 12    # three steps after the first adoption (step 9)
RING13_COMMIT_AT = 14   # three steps after the first adoption (step 11)
# ring13_two: the first step whose stamps differ under the auctioneers' rows
# (the round of the commit step itself, which runs after the commit)
STAMPS_DIFFER_AT = 14
NEAR128_COMMIT_AT = 17  # two steps after the last adoptions (steps 14 and 15)


def chord_ring_b(n):
    """The ring with chords 3 - (3 + n // 2) and 5 - (5 + n // 2): another
    adjacency than fleet_auction_cases.chord_ring on the same points."""
    ring = np.zeros((n, n), np.uint8)
    for i in range(n):
        ring[i, (i + 1) % n] = ring[(i + 1) % n, i] = 1
    for a in (3, 5):
        b = a + n // 2
        ring[a, b] = ring[b, a] = 1
    return ring


class EstTrialCase:
    """base: a fleet_trial_cases.Case; every link at 1 tick; loss: an int or
    [n][n]; seed: the swarm's u32; force: {step: f(restatement)} applied before
    that step."""

    def __init__(self, name, base, track_every=2, loss=0, seed=0, force=None):
        self.name, self.base, self.n = name, base, base.n
        self.forms, self.fseq, self.q, self.vel = base.forms, base.fseq, base.q, base.vel
        self.T, self.max_iter, self.steps = base.T, base.max_iter, base.steps
        self.tp_over, self.ep_over = base.tp_over, base.ep_over
        self.lat = DC.lat_uniform(self.n, 1)
        self.max_lat = 1
        self.loss, self.seed = LO.loss_matrix(self.n, loss), int(seed)
        self.track_every = int(track_every)
        self.force = dict(force or {})

    @property
    def tp(self):
        return self.base.tp

    def oracle(self, diag=True, follow="published"):
        return XT.EstFleetTrial(self.fseq, self.forms, self.q, self.vel, self.tp, self.lat,
                                loss=self.loss, seed=self.seed, max_iter=self.max_iter,
                                ticks_per_step=self.T, track_every=self.track_every, diag=diag,
                                loc_rows_follow=follow)

    def shared(self):
        """The shared-snapshot trial of the same case."""
        return LT.LossyFleetTrial(self.fseq, self.forms, self.q, self.vel, self.tp, self.lat,
                                  loss=self.loss, seed=self.seed, max_iter=self.max_iter,
                                  ticks_per_step=self.T)


def _case(name, forms, fseq, q, steps, max_iter=0):
    return K.Case(name, forms, fseq, q, steps, 10, max_iter=max_iter, tp=K.QUICK,
                  ep=K.DEFAULT_EVERY)


def single():
    rng = np.random.RandomState(1)
    p = FA.points(rng, 1)
    adj = np.zeros((1, 1), np.uint8)
    form = (p, adj, H.synth_gains(np.random.RandomState(7), adj))
    return EstTrialCase("single", _case("single", [form], [0], FA.snapshot(rng, 1), 8), 1)


def sync6_complete():
    c = TC.two_formations(6)
    forms = list(zip(c["pts"], c["adj"], c["gains"]))
    return EstTrialCase("sync6_complete", _case("sync6_complete", forms, [0, 1], c["q"], 21), 1,
                        force={SYNC6_COMMIT_AT: K.force_commit})


def _ring13(two):
    p, rng = TC.formation_points(13)
    adj = FA.chord_ring(13)
    G = H.synth_gains(np.random.RandomState(7), adj)
    q = p + TC.START_OFFSET
    q[:, :2] += rng.normal(0, 0.05, (13, 2))
    forms = [(p, adj, G)]
    if two:
        # vehicles 2 and 4 start at each other's points (as near128): the first
        # adopted assignment is not the identity
        q[[2, 4]] = q[[4, 2]]
        adj2 = chord_ring_b(13)
        forms.append((TC._scaled(p, 1.04), adj2, H.synth_gains(np.random.RandomState(8), adj2)))
    return forms, q


def ring13_one():
    sc = FA.clean_ring(13)
    return EstTrialCase("ring13_one",
                        _case("ring13_one", [K._ring_form(sc)], [0], sc.windows[0][1], 22), 2)


def ring13_two(loss=0, seed=0):
    forms, q = _ring13(True)
    name = "ring13_two_loss" if loss else "ring13_two"
    return EstTrialCase(name, _case(name, forms, [0, 1], q, RING13_STEPS[name]), 2, loss, seed,
                        force={RING13_COMMIT_AT: K.force_commit})


# three steps past the second adoption (step 22); under loss nobody adopts
RING13_STEPS = {"ring13_two": 26, "ring13_two_loss": 20}


def ring13_two_loss():
    return ring13_two(GOSSIP_LOSS, GOSSIP_SEED)


def rings12_two():
    sc = FA.rings12()
    forms = [K._ring_form(sc), (TC._scaled(sc.p, 1.04), sc.adj, K._ring_form(sc, 8)[2])]
    return EstTrialCase("rings12_two", _case("rings12_two", forms, [0, 1], sc.windows[0][1], 16),
                        2, force={10: K.force_commit})


def ring65_te2():
    sc = FA.clean_ring(65)
    return EstTrialCase("ring65_te2",
                        _case("ring65_te2", [K._ring_form(sc)], [0], sc.windows[0][1], 12), 2)


def near128_two():
    p, adj, G, q = K._near128_forms()
    forms = [(p, adj, G), (TC._scaled(p, 1.04), adj, G)]
    return EstTrialCase("near128_two",
                        _case("near128_two", forms, [0, 1], q, NEAR128_COMMIT_AT + 3, max_iter=40),
                        2, force={NEAR128_COMMIT_AT: K.force_commit})


CASES = {f.__name__: f for f in (single, sync6_complete, ring13_one, ring13_two, ring13_two_loss,
                                 rings12_two, ring65_te2, near128_two)}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def fly(cs, ft, steps=None, own=True):
    """A case on a restatement alone (the CPU oracle's alignments); every
    record also holds q and vel before and after the step."""
    recs = []
    for s in range(cs.steps if steps is None else steps):
        if s in cs.force:
            cs.force[s](ft)
        q0, vel0 = ft.q.copy(), ft.vel.copy()
        r = ft.step() if not own else ft.step(own=True)
        r["q0"], r["vel0"] = q0, vel0
        r["q"], r["vel"] = ft.q.copy(), ft.vel.copy()
        recs.append(r)
    return ft, recs


@functools.lru_cache(maxsize=None)
def cpu_run(name, follow="published"):
    """Shared by the tests, which leave it unchanged: (case, restatement, records)."""
    cs = case(name)
    ft, recs = fly(cs, cs.oracle(follow=follow))
    return cs, ft, recs


@functools.lru_cache(maxsize=None)
def cpu_shared(name):
    """The shared-snapshot trial of the case: (restatement, records)."""
    cs = case(name)
    return fly(cs, cs.shared(), own=False)


adoption_steps = K.adoption_steps


def commit_steps(recs):
    return [r["step"] for r in recs if r["committed"]]


def condition(recs):
    """The smallest decision margins over every step and every running
    controller with a close vehicle, on the step's own table and saturated
    command: (d_margin, edge_margin, quarter_margin), inf where there is none."""
    out = [np.inf] * 3
    for r in recs:
        for v in np.nonzero(r["on"])[0]:
            m = EC.decision_margins(int(v), r["est"][v], O.saturate(r["u"][v]))
            if m is not None:
                out = [min(a, b) for a, b in zip(out, m)]
    return tuple(out)
