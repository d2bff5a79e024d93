"""Scenarios of the fleet auction (acl_fleet_auction_batch) shared by the CPU
tests of the restatement (tests/test_fleet_auction.py) and the GPU parity
tests (tests/test_gpu_fleet_auction.py). A scenario is one swarm: a
formation, the vehicles' own rows and a list of windows (cmd [n], snapshot q
[n][3]); every window is one call that runs to quiescence."""
import functools

import numpy as np

import cbaa_step_oracle as S
import fleet_auction_oracle as FO
import helpers as H
import pyoracle as O


def chord_ring(n):
    """The ring with two chords of tests/test_gpu_vehicle_start.py::_graphs."""
    ring = np.zeros((n, n), np.uint8)
    for i in range(n):
        ring[i, (i + 1) % n] = ring[(i + 1) % n, i] = 1
    for a in (0, 1):
        b = a + n // 2
        ring[a, b] = ring[b, a] = 1
    return ring


def two_rings(m):
    """Two disjoint rings of m points: 0..m-1 and m..2m-1."""
    adj = np.zeros((2 * m, 2 * m), np.uint8)
    for o in (0, m):
        for i in range(m):
            adj[o + i, o + (i + 1) % m] = adj[o + (i + 1) % m, o + i] = 1
    return adj


def d_max(adj):
    return int(np.asarray(adj).sum(axis=1).max())


def window_ticks(adj):
    """Enough for any window of a scenario to reach quiescence: a clean
    auction takes at most 2 n d_max ticks (the slowest vehicle needs d_max
    ticks per iteration); a stalled or seeded one ends sooner."""
    return 2 * len(adj) * d_max(adj) + 8


def points(rng, n):
    return np.c_[rng.uniform(-n, n, (n, 2)), rng.uniform(0, 2, n)]


def snapshot(rng, n):
    return np.c_[rng.uniform(-n, n, (n, 2)), rng.uniform(0.5, 1.5, n)]


def align_rt(p, adj, q, rows):
    """Rt [n][6] of every vehicle under its own row (the CPU oracle's
    alignment, as tests/test_gpu_vehicle_start.py::_oracle composes it)."""
    n = len(q)
    out = np.zeros((n, 6))
    for v in range(n):
        R, t = O.align(n, v, q, p, adj, np.argsort(rows[v]).astype(np.uint16))
        out[v] = np.concatenate([R.reshape(4), t])
    return out


def lockstep_tables(p, adj, q, Rt, row):
    """cbaa_step_oracle.lockstep for a fleet whose vehicles all hold `row`."""
    n = len(q)
    C = np.stack([S.price_row(p, q[v], Rt[v]) for v in range(n)])
    return S.lockstep(C, adj, np.argsort(row))


class Scenario:
    def __init__(self, name, p, adj, windows, Pt=None, queue_cap=None):
        self.name, self.p, self.adj = name, np.asarray(p, np.float64), np.asarray(adj, np.uint8)
        self.n = len(self.p)
        self.windows = windows  # [(cmd [n] u8 or a callable(fleet) -> cmd, q [n][3])]
        self.Pt = Pt
        self.queue_cap = queue_cap
        self.ticks = window_ticks(self.adj)

    def fleet(self):
        return FO.Fleet(self.p, self.adj, Pt=self.Pt, queue_cap=self.queue_cap)

    def cmd(self, k, fleet):
        c = self.windows[k][0]
        return np.asarray(c(fleet) if callable(c) else c, np.uint8)


def _all(n, c=FO.START):
    return np.full(n, c, np.uint8)


def flush_flagged(fleet):
    """Window 3 of the stale-START sequence: the vehicles with an invalid
    assignment flush, nobody starts."""
    return np.where(fleet.invalid != 0, FO.FLUSH, FO.NONE).astype(np.uint8)


STALE_SEED = 11


def stale_start(n, seed=STALE_SEED, silent=3):
    """The four windows on the chord ring: all but `silent` start from q1 (a
    stall), all start from q2 (seeded with the stalled START bids), the
    flagged vehicles flush, all start from q4."""
    rng = np.random.RandomState(seed)
    adj = chord_ring(n)
    p = points(rng, n)
    q1, q2, q4 = (snapshot(rng, n) for _ in range(3))
    c1 = _all(n)
    c1[silent] = FO.NONE
    return Scenario(f"stale{n}", p, adj,
                    [(c1, q1), (_all(n), q2), (flush_flagged, q2), (_all(n), q4)])


def rings12(silent=2, seed=5):
    rng = np.random.RandomState(seed)
    n = 12
    c = _all(n)
    c[silent] = FO.NONE
    return Scenario("rings12", points(rng, n), two_rings(6), [(c, snapshot(rng, n))])


ROWS_SEED = 383     # finishes: 78 ticks, consensus at ticks 74-77, every table adopted
ROWS_STALL_SEED = 21  # a sender runs two iterations ahead: bids thrown away, a stall


def random_rows(n=13, seed=ROWS_SEED):
    rng = np.random.RandomState(seed)
    Pt = np.stack([rng.permutation(n) for _ in range(n)])
    return Scenario(f"rows{n}", points(rng, n), chord_ring(n), [(_all(n), snapshot(rng, n))],
                    Pt=Pt)


def clean_ring(n, seed=3):
    rng = np.random.RandomState(seed)
    return Scenario(f"ring{n}", points(rng, n), chord_ring(n), [(_all(n), snapshot(rng, n))])


def swarm6(queue_cap=None):
    pts, adj, _, q0 = H.swarm6()
    return Scenario("swarm6", pts[0], adj[0], [(_all(6), q0)], queue_cap=queue_cap)


def run_oracle(sc, rt_of=None):
    """Every window of a scenario on the restatement. rt_of(k, fleet, q):
    the Rt [n][6] handed to window k (default: the CPU oracle's alignment
    under the fleet's rows). Returns (fleet, [per-window record])."""
    fl = sc.fleet()
    recs = []
    for k, (_, q) in enumerate(sc.windows):
        cmd = sc.cmd(k, fl)
        rows = fl.Pt.copy()
        Rt = rt_of(k, fl, q) if rt_of else align_rt(sc.p, sc.adj, q, rows)
        st = fl.run(sc.ticks, q=q, cmd=cmd, Rt=Rt)
        recs.append(dict(status=st, cmd=cmd, rows=rows, Rt=Rt, q=q, state=snapshot_state(fl)))
    return fl, recs


STATE_KEYS = ("Pt", "open", "biditer", "invalid", "just_received", "price", "who", "final_price",
              "final_who", "done_tick", "vflags", "n_thrown", "n_tally")


def snapshot_state(fl):
    d = {k: np.array(getattr(fl, k)) for k in STATE_KEYS}
    d["queue_len"] = fl.queue_len()
    return d


@functools.lru_cache(maxsize=None)
def cpu_run(name):
    """A named scenario run once on the restatement with the CPU oracle's
    alignments, shared by the tests (which leave it alone)."""
    sc = {"stale13": lambda: stale_start(13), "rings12": rings12, "rows13": random_rows,
          "rows13_stall": lambda: random_rows(13, ROWS_STALL_SEED),
          "ring13": lambda: clean_ring(13), "swarm6": swarm6}[name]()
    fl, recs = run_oracle(sc)
    return sc, fl, recs
