"""Cases of acl_fleet_est_control_batch, shared by the CPU tests
(tests/test_fleet_est_control.py) and the GPU parity tests
(tests/test_gpu_fleet_est_control.py). A case is one swarm: a formation with
its gains, every vehicle's own table of estimates and own row.

The tables are the true positions perturbed per vehicle (so reading est[0] for
est[v] shows), with some entries never heard of (the origin); every vehicle
holds its own random row, and one vehicle holds a bad one.

condition(case) is the input condition the comparisons rest on: a difference of
1e-5 in u must not be able to flip a collision decision, so for every vehicle
with a close vehicle every |dist - d_avoid_thresh| >= 1e-6, and psi keeps 1e-4
rad from every no-fly-zone edge and from the |wrapToPi(edge - psi)| = pi/2
boundary. The seeds below were chosen on the CPU so that it holds for every
vehicle of every case; tests/test_fleet_est_control.py asserts it.
"""
import functools

import numpy as np

import fleet_auction_cases as C
import fleet_est_control_oracle as CO
import helpers as H
import pyoracle as O

D_MARGIN, ANGLE_MARGIN = 1e-6, 1e-4
SIZES = (1, 2, 6, 13, 20, 64, 65, 100, 128)


def graph(rng, n):
    """Complete up to 6 points; above, the chord ring with random extra edges
    (degrees from 2 to about n / 4: lanes with and without an edge in every
    pass of the walk)."""
    if n <= 6:
        return (np.ones((n, n)) - np.eye(n)).astype(np.uint8)
    adj = C.chord_ring(n)
    extra = np.triu(rng.uniform(size=(n, n)) < 0.12, 1)
    return (adj | extra | extra.T).astype(np.uint8)


class Case:
    """kind: 'spread' (few close vehicles), 'dense' (3-16 close, wrapped
    sectors) or 'packed' (everybody within d_avoid_thresh of everybody: the
    general resolve path from 18 vehicles on, surrounded vehicles). planes: 5
    (the ADMM block structure) or 9 (unstructured blocks). bad_row: whether
    vehicle n // 2 holds a row that is no permutation. nan: whether one
    vehicle's estimate of a far non-neighbour is NaN."""

    def __init__(self, n, kind, planes, seed, bad_row=True, nan=False):
        self.name = f"{kind}{n}_p{planes}_s{seed}"
        self.n, self.kind, self.planes, self.seed = n, kind, planes, seed
        rng = np.random.RandomState(seed)
        self.p = C.points(rng, n)
        self.adj = graph(rng, n)
        self.gains = (H.synth_gains if planes == 5 else H.random_block_gains)(rng, self.adj)
        side = {"spread": 2.2 * np.sqrt(n) + 2.0, "dense": 0.9 * np.sqrt(n) + 1.0,
                "packed": 1.0}[kind]
        if kind == "spread":
            self.q = H.random_positions(rng, n, side)
            self.q[:, 2] = rng.uniform(0.5, 1.5, n)
        else:
            self.q = H.dense_positions(rng, n, side)
        self.q[:, :2] += rng.uniform(2.0, 3.0, 2)  # nobody at the origin
        self.vel = rng.normal(0, 0.1, (n, 3))
        # every vehicle's own table: the truth perturbed, its own entry exact,
        # about one entry in seven never heard of
        self.est = self.q[None] + rng.normal(0, 0.05, (n, n, 3))
        unknown = rng.uniform(size=(n, n)) < 0.15
        for v in range(n):
            unknown[v, v] = False
            self.est[v, v] = self.q[v]
        self.est[unknown] = 0.0
        self.unknown = unknown
        self.Pt = np.stack([rng.permutation(n) for _ in range(n)]).astype(np.uint16)
        self.bad = ()
        if bad_row:
            v = n // 2
            if n == 1:
                self.Pt[v, 0] = 5  # out of range
            else:
                self.Pt[v, 0] = self.Pt[v, 1]  # a duplicate
            self.bad = (v,)
        self.nan = None
        if nan:
            self.nan = self._plant_nan()

    def _plant_nan(self):
        """The first vehicle with a good row and nobody close gets a NaN
        estimate of a vehicle that is no neighbour under its row: its command
        stays finite and its collision avoidance takes the serial path."""
        s = O.default_safety()
        for v in range(self.n):
            if v in self.bad or CO.sectors(v, self.est[v], s)["close"]:
                continue
            i = int(np.nonzero(self.Pt[v] == v)[0][0])
            nb = {int(self.Pt[v][j]) for j in range(self.n) if self.adj[i, j]}
            for j in range(self.n):
                if j != v and j not in nb:
                    self.est[v, j] = np.nan
                    return v, j
        raise AssertionError("no vehicle to plant a NaN estimate in")

    @functools.lru_cache(maxsize=None)
    def reference(self):
        """(u, u_safe, ca, status) of the restatement, computed once."""
        return CO.control_step(self.est, self.vel, self.Pt, self.p, self.adj, self.gains)


# (n, kind, planes) -> seed; every size in both gain layouts
SEEDS = {}
for _n in SIZES:
    SEEDS[(_n, "spread", 5)] = 100 + _n
    SEEDS[(_n, "spread", 9)] = 300 + _n
for _n in (6, 13, 20, 65, 100, 128):
    SEEDS[(_n, "dense", 5)] = 500 + _n
for _n in (3, 20, 40):
    SEEDS[(_n, "packed", 5)] = 700 + _n
SEEDS[(13, "dense", 9)] = 913
SEEDS[(20, "packed", 9)] = 920
NAN_CASES = ((13, "spread", 5), (100, "spread", 9))


@functools.lru_cache(maxsize=None)
def case(n, kind, planes):
    return Case(n, kind, planes, SEEDS[(n, kind, planes)], nan=(n, kind, planes) in NAN_CASES)


def all_keys():
    return sorted(SEEDS)


def condition(cs):
    """The smallest margins over the vehicles of a case that have a close
    vehicle: (d_margin, edge_margin, quarter_margin), inf where no vehicle
    has one."""
    u = cs.reference()[0]
    out = [np.inf] * 3
    for v in range(cs.n):
        if v in cs.bad:
            continue
        m = CO.decision_margins(v, cs.est[v], O.saturate(u[v]))
        if m is not None:
            out = [min(a, b) for a, b in zip(out, m)]
    return tuple(out)


def condition_holds(cs):
    d, e, q = condition(cs)
    return d >= D_MARGIN and e >= ANGLE_MARGIN and q >= ANGLE_MARGIN


def coverage(cs):
    """What a case exercises: the numbers of close vehicles per vehicle, and
    how many vehicles see a wrapped sector, a NaN, or get their command zeroed
    by collisionAvoidance."""
    u, us, ca, _ = cs.reference()
    close, wrapped, nan, zeroed = [], 0, 0, 0
    for v in range(cs.n):
        if v in cs.bad:
            continue
        sc = CO.sectors(v, cs.est[v])
        close.append(sc["close"])
        wrapped += int(sc["wrapped"])
        nan += int(sc["nan"] > 0)
        zeroed += int(ca[v] and not us[v].any() and u[v].any())
    return dict(close=close, wrapped=wrapped, nan=nan, zeroed=zeroed)
