"""Cases of the episodes on each vehicle's own estimates
(acl_fleet_est_episode_batch), shared by tests/test_fleet_est_episode.py (CPU)
and tests/test_gpu_fleet_est_episode.py: a case of tests/fleet_episode_cases.py
with every link at 1 tick (fleet_delay_episode_cases.ones), a loss matrix and
seed as tests/fleet_loss_cases.py takes them, and track_every. A case is one
swarm; its restatement records the error figures (diag).

Every figure quoted below is what tests/fleet_est_episode_oracle.py flew;
test_fleet_est_episode.py asserts each.
  ring13/complete  every off-diagonal adjacency bit set, track_every 1, loss 0:
      the shared-snapshot episode record for record; no adoption in 30 steps,
      30 CA vehicle-steps, error record 0
  ring13/te1       adoptions at steps 7 and 19 (13 vehicles each); q equal bit
      for bit to the shared-snapshot episode's, 41 CA vehicle-steps on both sides
  ring13/te2       the same adoption steps; q differs, the final prices differ
  rings12/te2      72 entries unknown for the whole flight (two components)
  ring65/te2       12 steps, 3 236 entries unknown at the end
"""
import functools

import numpy as np

import fleet_auction_cases as C
import fleet_delay_cases as DC
import fleet_delay_episode_cases as DEC
import fleet_episode_cases as K
import fleet_est_control_oracle as EC
import fleet_est_episode_oracle as XO
import fleet_loss_cases as LC
import fleet_loss_episode_oracle as LE
import fleet_loss_oracle as LO
import pyoracle as O

D_MARGIN, ANGLE_MARGIN = 1e-6, 1e-4  # the input condition of the collision decisions


def complete(base, seed=7):
    """A fleet_episode_cases.Case on the complete graph of its points: every
    off-diagonal adjacency bit set, helpers.synth_gains on it."""
    sc = base.sc
    adj = (1 - np.eye(sc.n)).astype(np.uint8)
    full = C.Scenario(sc.name + "_complete", sc.p, adj, sc.windows)
    cs = K.Case(base.name + "_complete", full, steps=base.steps, ticks_per_step=base.T,
                auction_every=base.ep["auction_every"], max_iter=base.max_iter, seed=seed)
    return cs


def single():
    """n = 1: one vehicle, no edge."""
    rng = np.random.RandomState(1)
    sc = C.Scenario("single", C.points(rng, 1), np.zeros((1, 1), np.uint8),
                    [(np.ones(1, np.uint8), C.snapshot(rng, 1))])
    return K.Case("single", sc, steps=6, ticks_per_step=10, auction_every=3)


BASES = {"single": single, "ring13_complete": lambda: complete(K.ring13()),
         # (seed 10: adoptions at steps 5 and 11, 14 CA vehicle-steps, margins
         # 0.37 / 0.13 / 0.105; helpers.swarm6 holds a distance at d_avoid_thresh)
         "ring6_complete": lambda: complete(K.Case("ring6", C.clean_ring(6, 10), steps=14,
                                                   ticks_per_step=10, auction_every=6))}


class EstCase:
    """cs: a fleet_delay_episode_cases.DelayCase; loss: an int or [n][n];
    seed: the swarm's u32; track_every."""

    def __init__(self, name, cs, track_every=2, loss=0, seed=0, steps=None):
        self.name, self.cs = name, cs
        self.loss, self.seed = LO.loss_matrix(cs.n, loss), int(seed)
        self.track_every = int(track_every)
        self.steps = cs.steps if steps is None else steps

    def __getattr__(self, k):
        return getattr(self.cs, k)

    def oracle(self, queue_cap=None, diag=True):
        cs = self.cs
        ep = XO.EstFleetEpisode(cs.p, cs.adj, cs.gains, cs.q0, cs.vel0, cs.ep, cs.lat,
                                loss=self.loss, seed=self.seed, Pt=cs.Pt, queue_cap=queue_cap,
                                max_iter=cs.max_iter, ticks_per_step=cs.T,
                                track_every=self.track_every, diag=diag)
        for v in cs.invalid0:
            ep.fleet.invalid[v] = 1
        return ep

    def shared(self):
        """The shared-snapshot episode of the same case."""
        cs = self.cs
        ep = LE.LossyFleetEpisode(cs.p, cs.adj, cs.gains, cs.q0, cs.vel0, cs.ep, cs.lat,
                                  loss=self.loss, seed=self.seed, Pt=cs.Pt,
                                  max_iter=cs.max_iter, ticks_per_step=cs.T)
        for v in cs.invalid0:
            ep.fleet.invalid[v] = 1
        return ep


def _ones(name):
    if name in BASES:
        base = BASES[name]()
        return DEC.DelayCase(f"{name}/ones", base, DC.lat_uniform(base.n, 1))
    return DEC.ones(name)


GOSSIP_LOSS, GOSSIP_SEED = 4096, 5

# name -> (base case, track_every, loss, seed, steps)
TABLE = {
    "single": ("single", 1, 0, 0, None),
    "ring13_complete": ("ring13_complete", 1, 0, 0, None),
    "ring6_complete": ("ring6_complete", 1, 0, 0, None),
    "ring13_te1": ("ring13", 1, 0, 0, None),
    "ring13_te2": ("ring13", 2, 0, 0, None),
    "ring13_te3": ("ring13", 3, 0, 0, None),
    "ring13_loss64": ("ring13", 2, LC.EP_LOSS, LC.EP_SEED, None),
    "ring13_loss4096": ("ring13", 2, GOSSIP_LOSS, GOSSIP_SEED, None),
    "rings12_te2": ("rings12", 2, 0, 0, None),
    "ring65_te2": ("ring65", 2, 0, 0, 12),
    "odd_last128_te2": ("odd_last128", 2, 0, 0, 4),
}

# the cases the GPU parity tests fly, teacher-forced
GPU_CASES = ("single", "ring13_te1", "ring13_te2", "ring13_te3", "ring13_loss64",
             "ring13_loss4096", "rings12_te2", "ring65_te2", "odd_last128_te2",
             "ring13_complete", "ring6_complete")


@functools.lru_cache(maxsize=None)
def case(name):
    base, te, loss, seed, steps = TABLE[name]
    return EstCase(name, _ones(base), te, loss, seed, steps)


def fly(cs, ep, steps=None):
    """A case on a restatement alone (the CPU oracle's alignments)."""
    recs = []
    for s in range(cs.steps if steps is None else steps):
        if s in cs.q_at:
            ep.q = np.array(cs.q_at[s], np.float64)
        q0, vel0 = ep.q.copy(), ep.vel.copy()
        r = ep.step()
        r["q0"], r["vel0"] = q0, vel0
        r["q"], r["vel"] = ep.q.copy(), ep.vel.copy()
        recs.append(r)
    return ep, recs


@functools.lru_cache(maxsize=None)
def cpu_run(name):
    """Shared by the tests, which leave it unchanged: (case, oracle, records)."""
    cs = case(name)
    ep, recs = fly(cs, cs.oracle())
    return cs, ep, recs


@functools.lru_cache(maxsize=None)
def cpu_shared(name):
    """The shared-snapshot episode of the case: (oracle, records)."""
    cs = case(name)
    return fly(cs, cs.shared())


adoption_steps = K.adoption_steps


def condition(recs):
    """The smallest decision margins over every step and every vehicle with a
    close vehicle, on the step's own table and saturated command:
    (d_margin, edge_margin, quarter_margin), inf where there is none."""
    out = [np.inf] * 3
    for r in recs:
        for v in range(len(r["u"])):
            m = EC.decision_margins(v, r["est"][v], O.saturate(r["u"][v]))
            if m is not None:
                out = [min(a, b) for a, b in zip(out, m)]
    return tuple(out)
