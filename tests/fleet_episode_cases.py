"""Cases of the episodes on the message-level auction
(acl_fleet_episode_batch), shared by the CPU tests of the restatement
(tests/test_fleet_episode.py) and the GPU parity tests
(tests/test_gpu_fleet_episode.py). Built on tests/fleet_auction_cases.py; the
gains are helpers.synth_gains on the case's graph (parity of the arithmetic
needs no designed gains). A case is one swarm."""
import functools

import numpy as np

import episode_oracle as E
import fleet_auction_cases as C
import fleet_auction_oracle as FO
import fleet_episode_oracle as FE
import helpers as H


class Case:
    """q_at: {global step: q [n][3]} snapshots the caller writes into q before
    that step (between chunks); invalid0: vehicles that start with invalid =
    1; ep: overrides of the default episode parameters."""

    def __init__(self, name, sc, steps, ticks_per_step, auction_every, Pt=None, max_iter=0,
                 invalid0=(), q_at=None, seed=7):
        self.name, self.sc, self.n = name, sc, sc.n
        self.p, self.adj = sc.p, sc.adj
        self.steps, self.T, self.max_iter = steps, ticks_per_step, max_iter
        self.Pt = np.tile(np.arange(sc.n), (sc.n, 1)) if Pt is None else np.asarray(Pt)
        self.invalid0 = tuple(invalid0)
        self.q_at = dict(q_at or {})
        self.q0 = self.q_at.pop(0) if 0 in self.q_at else sc.windows[0][1]
        self.vel0 = np.zeros((sc.n, 3))
        self.gains = H.synth_gains(np.random.RandomState(seed), self.adj)
        # a short supervisor window, so that the predicates are evaluated
        # within the case's few steps
        self.ep = dict(E.default_params(), auction_every=auction_every, bufflen=5)

    def oracle(self, queue_cap=None):
        ep = FE.FleetEpisode(self.p, self.adj, self.gains, self.q0, self.vel0, self.ep, Pt=self.Pt,
                             queue_cap=queue_cap, max_iter=self.max_iter, ticks_per_step=self.T)
        for v in self.invalid0:
            ep.fleet.invalid[v] = 1
        return ep


def ring13():
    return Case("ring13", C.clean_ring(13), steps=30, ticks_per_step=10, auction_every=12)


def ring13_t2():
    return Case("ring13_t2", C.clean_ring(13), steps=45, ticks_per_step=2, auction_every=60)


def stale13():
    sc = C.stale_start(13)
    q1, q2, q4 = sc.windows[0][1], sc.windows[1][1], sc.windows[3][1]
    return Case("stale13", sc, steps=48, ticks_per_step=10, auction_every=12, invalid0=(3,),
                q_at={0: q1, 12: q2, 36: q4})


def rings12():
    return Case("rings12", C.rings12(), steps=26, ticks_per_step=10, auction_every=12,
                invalid0=(2,))


def ring65():
    return Case("ring65", C.clean_ring(65), steps=45, ticks_per_step=10, auction_every=45)


def _chord128(name, Pt):
    rng = np.random.RandomState(128)
    n = 128
    sc = C.Scenario(name, C.points(rng, n), C.chord_ring(n), [(np.ones(n, np.uint8),
                                                               C.snapshot(rng, n))])
    return Case(name, sc, steps=8, ticks_per_step=10, auction_every=120, Pt=Pt, max_iter=16)


def odd_last128():
    """Every vehicle holds the identity except vehicle 127, whose row swaps
    two points: only the last row of the n x n rows differs. The two points
    (0 and 126) are the ring neighbours of vehicle 127's own point, so its
    command differs from the one it would fly under the shared table."""
    Pt = np.tile(np.arange(128), (128, 1))
    Pt[127, [0, 126]] = [126, 0]
    return _chord128("odd_last128", Pt)


def odd_last128_col():
    """Vehicles 126 and 127 both hold the row that swaps points 126 and 127:
    only the last columns differ."""
    Pt = np.tile(np.arange(128), (128, 1))
    Pt[126:, [126, 127]] = [127, 126]
    return _chord128("odd_last128_col", Pt)


CASES = {f.__name__: f for f in (ring13, ring13_t2, stale13, rings12, ring65, odd_last128,
                                 odd_last128_col)}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def cpu_run(name):
    """A case flown once on the restatement alone (the CPU oracle's
    alignments), shared by the tests, which leave it unchanged. Returns
    (case, oracle, [per-step record])."""
    cs = case(name)
    ep = cs.oracle()
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
    return cs, ep, recs


def adoption_steps(recs):
    """Steps at which some vehicle adopted -> how many did."""
    out = {}
    for r in recs:
        k = int(((r["raised"] & FO.V_ADOPTED) != 0).sum())
        if k:
            out[r["step"]] = k
    return out
