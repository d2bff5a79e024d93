"""Cases of fleet localization (acl_fleet_localize_batch) and of the fleet
auction started from own estimates (acl_fleet_est_auction_batch), shared by the
CPU tests (tests/test_fleet_localize.py) and the GPU parity tests
(tests/test_gpu_fleet_localize.py, tests/test_gpu_fleet_est.py).

Every figure quoted below is what the restatements (tests/fleet_localize_oracle.py,
tests/fleet_est_oracle.py) ran; the CPU tests assert each.

  chord_ring(13), identity rows, lossless   everybody known after 6 rounds,
      max_age 5; chord_ring(64) after 31, chord_ring(65) after 32,
      chord_ring(128) after 63
  two_rings(6)   72 entries stay at stamp 0 with zero positions for ever
  chord_ring(13), threshold 4096 on every link, seeds 0..7, 24 rounds
      tables lost: LOSS_TOTALS
  the stale batch (stale13): B = 8 on chord_ring(13), gossip loss 0 for swarm 0
      and 4096 with seeds 1..7 for the others, a snapshot drawn per round for
      24 rounds, then one clean auction on lossless links from the estimates
"""
import functools

import numpy as np

import fleet_auction_cases as C
import fleet_auction_oracle as FO
import fleet_est_oracle as EO
import fleet_localize_oracle as GO
import fleet_loss_cases as LC
import fleet_loss_oracle as LO

# n: (rounds until everybody is known, max_age from then on)
KNOWN_AFTER = {13: (6, 5), 64: (31, 30), 65: (32, 31), 128: (63, 62)}
LOSS_THR, LOSS_ROUNDS = 4096, 24
LOSS_TOTALS = [45, 53, 44, 46, 43, 49, 44, 52]  # seeds 0..7


def trajectory(n, rounds, seed):
    """[rounds][n][3]: an independent fleet_auction_cases.snapshot per round."""
    rng = np.random.RandomState(seed)
    return np.stack([C.snapshot(rng, n) for _ in range(rounds)])


def identity(n):
    return np.tile(np.arange(n), (n, 1))


def ring_loss(seed):
    """chord_ring(13) under LOSS_THR on every link, from round 0."""
    return GO.Trackers(C.chord_ring(13), loss=LOSS_THR, seed=seed)


MATRIX_SEED = 900


def loss_matrices13():
    """B = 8 on chord_ring(13): a drawn matrix per swarm, thresholds in {0, 256,
    4096, 0xFFFF} on about a third of the links (swarm 0: none), seeds 40 + b."""
    ms = [LC.loss_draw(13, MATRIX_SEED + b, density=0.35) for b in range(8)]
    ms[0][:] = 0
    return ms, [40 + b for b in range(8)]


class EstCase:
    """A fleet_loss_cases.LossCase whose fleet is the own-estimate one."""

    def __init__(self, lc):
        self.lc = lc

    def __getattr__(self, k):
        return getattr(self.lc, k)

    def fleet(self, queue_cap=None):
        lc = self.lc
        return EO.EstFleet(lc.sc.p, lc.sc.adj, lc.lat, loss=lc.loss, seed=lc.seed, Pt=lc.sc.Pt,
                           queue_cap=lc.queue_cap if queue_cap is None else queue_cap,
                           max_iter=lc.max_iter)


# ---- the stale batch of the own-estimate auction ----
STALE_B, STALE_ROUNDS, STALE_SEED = 8, 24, 611


class StaleBatch:
    """What test (c) and the GPU tests share: the formation, the trajectory,
    every swarm's trackers after the 24 rounds, and the auctions."""

    def __init__(self):
        rng = np.random.RandomState(STALE_SEED)
        n = self.n = 13
        self.adj = C.chord_ring(n)
        self.p = C.points(rng, n)
        self.traj = trajectory(n, STALE_ROUNDS, STALE_SEED + 1)
        self.q = self.traj[-1]  # the shared snapshot: the true positions of the last round
        self.loss = [0] + [LOSS_THR] * (STALE_B - 1)
        self.seeds = list(range(STALE_B))
        self.ticks = C.window_ticks(self.adj)

    def trackers(self):
        out = []
        for b in range(STALE_B):
            tr = GO.Trackers(self.adj, loss=self.loss[b], seed=self.seeds[b])
            tr.run(STALE_ROUNDS, self.traj)
            out.append(tr)
        return out

    def fleet(self):
        """A clean auction: every link 1 tick, nothing lost."""
        return EO.EstFleet(self.p, self.adj, 1, loss=0, seed=0)

    def auction(self, est):
        """START everybody from est [n][n][3] and run to quiescence."""
        fl = self.fleet()
        rows = fl.Pt.copy()
        st = fl.run(self.ticks, cmd=C._all(self.n), Rt=EO.align_rt(self.p, self.adj, est, rows),
                    est=est)
        assert st["flags"] & FO.QUIESCENT
        return fl, st

    def shared(self):
        """The shared-snapshot auction on the lossy restatement."""
        fl = LO.LossyFleet(self.p, self.adj, 1, loss=0, seed=0)
        st = fl.run(self.ticks, q=self.q, cmd=C._all(self.n),
                    Rt=C.align_rt(self.p, self.adj, self.q, fl.Pt.copy()))
        assert st["flags"] & FO.QUIESCENT
        return fl, st


@functools.lru_cache(maxsize=None)
def stale13():
    """(batch, trackers [B], own-estimate auctions [(fleet, status)], the
    shared-snapshot auction), run once and left alone by the tests."""
    sb = StaleBatch()
    trs = sb.trackers()
    return sb, trs, [sb.auction(tr.est()) for tr in trs], sb.shared()


def stale_condition(runs, shared):
    """Swarm 0's tables equal the shared-snapshot run's; every other swarm's
    final prices differ from it."""
    fl0 = shared[0]
    same = all(np.array_equal(np.array(getattr(runs[0][0], k)), np.array(getattr(fl0, k)))
               for k in C.STATE_KEYS)
    return same and all(
        not np.array_equal(fl.final_price.view(np.uint32), fl0.final_price.view(np.uint32))
        for fl, _ in runs[1:])
