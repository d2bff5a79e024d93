"""Latency cases of the fleet auction with per-link latency
(acl_fleet_delay_auction_batch), shared by tests/test_fleet_delay.py (CPU) and
tests/test_gpu_fleet_delay.py: a scenario of tests/fleet_auction_cases.py, a
latency matrix with a committed seed, max_lat, and a tick budget per window.

The budgets are not bounds anybody derived: every figure below is what
tests/fleet_delay_oracle.py ran (test_fleet_delay.py asserts each), and the
budget is a round number above it. A window with a budget must end QUIESCENT;
a window with an explicit tick count (the restart case's first) is cut short
on purpose.
"""
import functools

import numpy as np

import fleet_auction_cases as C
import fleet_auction_oracle as FO
import fleet_delay_oracle as DO


def lat_draw(n, seed, lo=1, hi=5):
    """[n][n] u8 (receiver-major), uniform in lo..hi; the diagonal too (ignored)."""
    return np.random.RandomState(seed).randint(lo, hi + 1, (n, n)).astype(np.uint8)


def lat_uniform(n, l):
    return np.full((n, n), l, np.uint8)


class DelayCase:
    def __init__(self, name, sc, lat, budget, max_lat=None, wticks=None, queue_cap=None,
                 max_iter=0):
        self.name, self.sc, self.n = name, sc, sc.n
        self.lat = np.ascontiguousarray(lat, np.uint8).reshape(sc.n, sc.n)
        self.max_lat = int(self.lat.max()) if max_lat is None else int(max_lat)
        self.budget = int(budget)
        # ticks of window k: wticks[k], or the budget (then the window must end QUIESCENT)
        self.wticks = list(wticks) if wticks else [None] * len(sc.windows)
        self.queue_cap = queue_cap
        self.max_iter = max_iter  # 0: 2 n

    def ticks(self, k):
        return self.budget if self.wticks[k] is None else self.wticks[k]

    def fleet(self, queue_cap=None):
        return DO.DelayFleet(self.sc.p, self.sc.adj, self.lat, Pt=self.sc.Pt,
                             queue_cap=self.queue_cap if queue_cap is None else queue_cap,
                             max_iter=self.max_iter)


def run_oracle(case, rt_of=None, hist=None):
    """Every window of a case on the restatement (as fleet_auction_cases.run_oracle)."""
    sc = case.sc
    fl = case.fleet()
    recs = []
    for k, (_, q) in enumerate(sc.windows):
        cmd = sc.cmd(k, fl)
        rows = fl.Pt.copy()
        Rt = rt_of(k, fl, q) if rt_of else C.align_rt(sc.p, sc.adj, q, rows)
        st = fl.run(case.ticks(k), q=q, cmd=cmd, Rt=Rt, hist=hist)
        assert case.wticks[k] is not None or st["flags"] & FO.QUIESCENT, (case.name, k, st)
        recs.append(dict(status=st, cmd=cmd, rows=rows, Rt=Rt, q=q, state=C.snapshot_state(fl)))
    return fl, recs


SCENARIOS = {
    "stale13": lambda: C.stale_start(13), "rings12": C.rings12, "rows13": C.random_rows,
    "rows13_stall": lambda: C.random_rows(13, C.ROWS_STALL_SEED),
    "ring13": lambda: C.clean_ring(13), "swarm6": C.swarm6,
}
NAMES = tuple(sorted(SCENARIOS))

# The seed of each scenario's 1..5 draw. ticks_run of every window under it, as
# the restatement ran them (test_fleet_delay.py::DRAW_TICKS asserts them):
#   swarm6 57 (36 at latency 1), ring13 119 (78), stale13 29 / 121 / 0 / 121
#   (11 / 78 / 0 / 78), rings12 99 (48), rows13 134 (78), rows13_stall 113 (it
#   stalls after 26 at latency 1 and finishes under this draw)
DRAW_SEED = {"swarm6": 1, "ring13": 2, "stale13": 3, "rings12": 4, "rows13": 5,
             "rows13_stall": 6}
BUDGET = 400


def ones(name):
    """All links at 1 tick: today's model tick for tick."""
    sc = SCENARIOS[name]()
    return DelayCase(f"{name}/ones", sc, lat_uniform(sc.n, 1), sc.ticks)


def draw(name, seed=None, hi=5, max_lat=None):
    sc = SCENARIOS[name]()
    seed = DRAW_SEED[name] if seed is None else seed
    return DelayCase(f"{name}/draw{seed}", sc, lat_draw(sc.n, seed, 1, hi), BUDGET,
                     max_lat=max_lat)


CLEAN_SEEDS = (11, 12, 13)  # the three draws of the clean swarm6 / ring13 auctions

# rows13 finishes in 78 ticks at latency 1; under this draw 7 bids are thrown
# away and all 13 vehicles stay open (quiescent after 68 ticks)
ROWS_FLIP_SEED = 115
# rows13_stall stalls after 26 ticks at latency 1; under this draw it finishes
# in 123 ticks, consensus at ticks 117-122, nothing thrown away
ROWS_STALL_FLIP_SEED = 61


def rows13_stalls():
    return draw("rows13", ROWS_FLIP_SEED)


def rows13_stall_finishes():
    return draw("rows13_stall", ROWS_STALL_FLIP_SEED)


def wrap(name="ring13", seed=21):
    """lat in {1, 2} with max_lat = 2: the publication log is a ring of 4 that
    wraps every few ticks."""
    return draw(name, seed, hi=2, max_lat=2)


def uniform64():
    """The largest ring: every link at 64 ticks, swarm6."""
    sc = C.swarm6()
    return DelayCase("swarm6/uniform64", sc, lat_uniform(6, 64), 3000)


def uniform(name, l, budget=BUDGET):
    sc = SCENARIOS[name]()
    return DelayCase(f"{name}/uniform{l}", sc, lat_uniform(sc.n, l), budget)


RESTART_SEED = 3


def restart_busy(n=13, seed=RESTART_SEED):
    """Every link at 5 ticks on the chord ring. Window 1: everybody starts and
    the call runs 3 ticks: the START bids (publication tick -1) are due at
    tick 4 and still in flight. Window 2 (first tick 3): everybody starts
    again from another snapshot, publication tick 2, due at tick 7."""
    rng = np.random.RandomState(seed)
    adj = C.chord_ring(n)
    p = C.points(rng, n)
    q1, q2 = C.snapshot(rng, n), C.snapshot(rng, n)
    sc = C.Scenario(f"restart{n}", p, adj, [(C._all(n), q1), (C._all(n), q2)])
    return DelayCase(f"restart{n}", sc, lat_uniform(n, 5), 600, wticks=[3, None])


def overflow6():
    """queue_cap = 2 on swarm6 under a 1..2 draw: bids are dropped at vehicles
    3 and 5 and the auction stalls after 8 ticks."""
    sc = C.swarm6()
    return DelayCase("swarm6/cap2", sc, lat_draw(6, 1, 1, 2), BUDGET, queue_cap=2)


# The restatement takes 11 s per swarm for the 2 n iterations of n = 128, so
# parity with it at the wavefront boundaries runs this many iterations.
RING_ITERS = {64: 32, 65: 32, 128: 16}


def ring_case(n, seed, hi=4):
    """The chord ring at a wavefront boundary, identity rows, one START
    window under a 1..hi draw, max_iter = RING_ITERS[n] (at most 145 ticks).
    With max_iter = 2 n the restatement runs 577, 576 (n = 64), 521, 585
    (65), 1026, 1027 (128) ticks for seeds 0, 1."""
    rng = np.random.RandomState(100 * n + seed)
    sc = C.Scenario(f"chord{n}/{seed}", C.points(rng, n), C.chord_ring(n),
                    [(C._all(n), C.snapshot(rng, n))])
    return DelayCase(sc.name, sc, lat_draw(n, 1000 * n + seed, 1, hi), BUDGET,
                     max_iter=RING_ITERS[n])


@functools.lru_cache(maxsize=None)
def cpu_run(key, *args):
    """A case run once on the restatement with the CPU oracle's alignments,
    shared by the tests (which leave it alone). key: a function of this
    module."""
    case = globals()[key](*args)
    fl, recs = run_oracle(case)
    return case, fl, recs
