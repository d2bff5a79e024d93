"""Cases of the episodes with per-link message latency
(acl_fleet_delay_episode_batch), shared by tests/test_fleet_delay_episode.py
(CPU) and tests/test_gpu_fleet_delay_episode.py: a case of
tests/fleet_episode_cases.py and a latency matrix with a committed seed
(fleet_delay_cases.lat_draw / lat_uniform). A case is one swarm.

Every figure quoted below is what tests/fleet_delay_episode_oracle.py ran;
test_fleet_delay_episode.py asserts each.
  ring13/draw2    adoptions at steps 11 and 22 (7 and 19 at latency 1)
  ring13/u5       every link at 5 ticks: nobody ever adopts; the auto-auctions
                  of steps 12 and 24 restart 13 open auctioneers with 9-10
                  publications in flight
  stale13/draw2   the last adoption at step 47 (43 at latency 1)
  restart13/u8    the chord ring, 2 ticks per step, an auto-auction every 3
                  steps, every link at 8 ticks, 12 steps: no START bid has
                  arrived when the next auto-auction restarts everybody; 13 /
                  26 / 35 publications in flight at steps 3 / 6 / 9, 39 restarts
  rings12/draw2   two components: INVALID and FLUSH alternate, later than at
                  latency 1
  ring65/draw     max_iter = fleet_delay_cases.RING_ITERS[65] = 32, links at
                  1..4 ticks, RING65_STEPS steps: consensus (INVALID) spread
                  over steps 10-14, RING65_CONSENSUS
  odd_last128/draw  links at 1..3 ticks, max_iter 16, 8 steps: 128 consensus,
                  all INVALID, per-vehicle rows from step 0
"""
import functools

import numpy as np

import fleet_auction_cases as C
import fleet_delay_cases as DC
import fleet_delay_episode_oracle as DE
import fleet_episode_cases as K

SEED13 = 2       # lat_draw(13, 2, 1, 5): ring13 and stale13
SEED12 = 2       # lat_draw(12, 2, 1, 5)
SEED65 = 65001   # lat_draw(65, 65001, 1, 4)
SEED128 = 128001  # lat_draw(128, 128001, 1, 3)

# ring65/draw as the restatement flew it. 32 iterations do not fill a table on
# the ring of 65 (every final table lacks 11 to 16 tasks, at latency 1 as
# under the draw), so the 65 vehicles reach consensus on an INVALID table and
# nobody adopts; what spreads over several steps is the consensus:
# {step: vehicles}, done_tick 109..143 (steps 7-9, done_tick 72..95 at
# latency 1). RING65_STEPS covers it.
RING65_STEPS = 16
RING65_CONSENSUS = {10: 1, 11: 13, 12: 34, 13: 9, 14: 8}
RING65_DONE_TICK = (109, 143)
RING65_TICKS = 144


class DelayCase:
    """base: a fleet_episode_cases.Case (its own copy); lat [n][n] u8."""

    def __init__(self, name, base, lat, steps=None, max_iter=None, max_lat=None):
        self.name, self.base = name, base
        self.n, self.p, self.adj, self.gains = base.n, base.p, base.adj, base.gains
        self.Pt, self.invalid0, self.q_at = base.Pt, base.invalid0, base.q_at
        self.q0, self.vel0, self.ep, self.T = base.q0, base.vel0, base.ep, base.T
        self.steps = base.steps if steps is None else steps
        self.max_iter = base.max_iter if max_iter is None else max_iter
        self.lat = np.ascontiguousarray(lat, np.uint8).reshape(self.n, self.n)
        self.max_lat = int(self.lat.max()) if max_lat is None else int(max_lat)

    def oracle(self, queue_cap=None, lat=None):
        ep = DE.DelayFleetEpisode(self.p, self.adj, self.gains, self.q0, self.vel0, self.ep,
                                  self.lat if lat is None else lat, Pt=self.Pt,
                                  queue_cap=queue_cap, max_iter=self.max_iter,
                                  ticks_per_step=self.T)
        for v in self.invalid0:
            ep.fleet.invalid[v] = 1
        return ep


def ring13_draw():
    return DelayCase("ring13/draw2", K.ring13(), DC.lat_draw(13, SEED13, 1, 5))


def ring13_u5():
    return DelayCase("ring13/u5", K.ring13(), DC.lat_uniform(13, 5))


def stale13_draw():
    return DelayCase("stale13/draw2", K.stale13(), DC.lat_draw(13, SEED13, 1, 5))


def restart13_u8():
    base = K.Case("restart13", C.clean_ring(13), steps=12, ticks_per_step=2, auction_every=3)
    return DelayCase("restart13/u8", base, DC.lat_uniform(13, 8))


def rings12_draw():
    return DelayCase("rings12/draw2", K.rings12(), DC.lat_draw(12, SEED12, 1, 5))


def ring65_draw():
    return DelayCase("ring65/draw", K.ring65(), DC.lat_draw(65, SEED65, 1, 4),
                     steps=RING65_STEPS, max_iter=DC.RING_ITERS[65])


def odd_last128_draw():
    return DelayCase("odd_last128/draw", K.odd_last128(), DC.lat_draw(128, SEED128, 1, 3))


def ones(name):
    """An existing case with every link at 1 tick: today's model step for step."""
    base = K.CASES[name]()
    return DelayCase(f"{name}/ones", base, DC.lat_uniform(base.n, 1))


CASES = {f.__name__: f for f in (ring13_draw, ring13_u5, stale13_draw, restart13_u8, rings12_draw,
                                 ring65_draw, odd_last128_draw)}


@functools.lru_cache(maxsize=None)
def case(name, *args):
    return CASES[name]() if name in CASES else globals()[name](*args)


def fly(cs, ep=None):
    """A case flown on the restatement alone (the CPU oracle's alignments), as
    fleet_episode_cases.cpu_run flies its cases. Returns (oracle, records)."""
    ep = cs.oracle() if ep is None else ep
    recs = []
    for s in range(cs.steps):
        if s in cs.q_at:
            ep.q = np.array(cs.q_at[s], np.float64)
        r = ep.step()
        r["open"] = ep.fleet.open.copy()
        r["invalid"] = ep.fleet.invalid.copy()
        r["done_tick"] = ep.fleet.done_tick.copy()
        r["tick"] = ep.fleet.tick
        recs.append(r)
    return ep, recs


@functools.lru_cache(maxsize=None)
def cpu_run(name, *args):
    """Shared by the tests, which leave it unchanged: (case, oracle, records)."""
    cs = case(name, *args)
    ep, recs = fly(cs)
    return cs, ep, recs


adoption_steps = K.adoption_steps
