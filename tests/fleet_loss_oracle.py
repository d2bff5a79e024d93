"""Plain-Python restatement of the fleet auction with seeded per-link message
loss (acl_fleet_lossy_auction_batch, include/aclswarm_amd.h):
fleet_delay_oracle's DelayFleet with one sentence of delivery changed. A bid
that is due at a receiver that subscribes to its sender is lost iff

    loss[w][u] == 0xFFFF  or  (link_hash(seed, w, u, P, iter) >> 16) < loss[w][u]

and otherwise appended or dropped for capacity as before. Nothing else differs.

TEST INFRASTRUCTURE ONLY: imported by tests/, never by the product package.
"""
import numpy as np

import fleet_auction_oracle as FO
import fleet_delay_oracle as DO

M32 = 0xFFFFFFFF
DEAD = 0xFFFF


def link_hash(seed, w, u, P, it):
    """The header's link_hash in plain integers modulo 2^32."""
    h = seed & M32
    for word in ((w << 16) | u, P & M32, it & M32):
        h = ((h ^ word) * 0x9E3779B1) & M32
        h ^= h >> 15
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def is_lost(thr, seed, w, u, P, it):
    return thr == DEAD or (link_hash(seed, w, u, P, it) >> 16) < thr


def loss_matrix(n, loss):
    """An int (every link) or [n][n] (receiver-major) as an [n][n] int array."""
    loss = np.asarray(loss, np.int64)
    m = np.full((n, n), int(loss)) if loss.ndim == 0 else loss.reshape(n, n).copy()
    assert m.min() >= 0 and m.max() <= DEAD
    return m


class LossyFleet(DO.DelayFleet):
    """One swarm. loss and seed are attributes: the caller may replace them
    between runs, and the values of the run in whose delivery phase a bid is
    due decide its fate."""

    def __init__(self, p, adj, lat, loss=0, seed=0, Pt=None, queue_cap=None, max_iter=0):
        super().__init__(p, adj, lat, Pt=Pt, queue_cap=queue_cap, max_iter=max_iter)
        self.loss = loss_matrix(self.n, loss)
        self.seed = int(seed) & M32
        self.n_lost = np.zeros(self.n, np.int32)
        self.lost_trace = None  # a list: receives (tick, receiver, sender, publication tick, iter)

    def _deliver(self):
        T = self.tick
        overflow = False
        subs = [self.subscribed(w) for w in range(self.n)]
        for u in range(self.n):  # ascending sender id, its bids in publication order
            for P, it, pr, wh in self.log[u]:
                for w in range(self.n):
                    if u not in subs[w] or P + self.lat[w][u] != T:
                        continue
                    if is_lost(int(self.loss[w][u]), self.seed, w, u, P, it):
                        self.n_lost[w] += 1  # before the capacity test: no slot, no flag
                        if self.lost_trace is not None:
                            self.lost_trace.append((T, w, u, P, it))
                        continue
                    if len(self.queue[w]) >= self.cap:
                        self.vflags[w] |= FO.V_OVERFLOW
                        overflow = True
                        continue
                    self.queue[w].append((u, it, pr, wh))
                    self.max_queue = max(self.max_queue, len(self.queue[w]))
                    if self.trace is not None:
                        self.trace.append((T, w, u, P, it))
            self.log[u] = [e for e in self.log[u] if e[0] + self.reach[u] > T]
        return overflow
