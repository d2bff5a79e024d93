"""Plain-Python restatement of the fleet auction with per-link message latency
(acl_fleet_delay_auction_batch, include/aclswarm_amd.h): fleet_auction_oracle's
Fleet with delivery replaced. Everything but delivery -- commands, buckets,
processBid, the tally, consensus and adoption -- is the base class's.

TEST INFRASTRUCTURE ONLY: imported by tests/, never by the product package.

lat[w][u] is the number of ticks from sender u's publication to receiver w's
queue (receiver-major, the diagonal ignored). A bid published by the
processing phase of tick T has publication tick T; one published by a START
command of a call whose first tick is T0 has publication tick T0 - 1; a bid
with publication tick P reaches w's queue in the delivery phase of tick
P + lat[w][u], if w subscribes to u at that moment.
"""
import numpy as np

import fleet_auction_oracle as FO


class DelayFleet(FO.Fleet):
    """One swarm. lat: an int (uniform) or [n][n] (receiver-major)."""

    def __init__(self, p, adj, lat, Pt=None, queue_cap=None, max_iter=0):
        super().__init__(p, adj, Pt=Pt, queue_cap=queue_cap, max_iter=max_iter)
        n = self.n
        lat = np.asarray(lat, np.int64)
        self.lat = np.full((n, n), int(lat)) if lat.ndim == 0 else lat.reshape(n, n).copy()
        np.fill_diagonal(self.lat, 1)  # ignored by the model; 1 keeps reach right at n = 1
        assert self.lat.min() >= 1
        self.reach = self.lat.max(axis=0)  # per sender: its slowest link
        # per sender: [(publication tick, iter, price, who)] in publication order,
        # kept until the delivery phase of tick P + reach has run
        self.log = [[] for _ in range(n)]
        self._in_command = False
        self.last_pub = np.full(n, -1, np.int64)  # per sender: its newest publication tick
        self.trace = None  # a list: receives (tick, receiver, sender, publication tick, iter)

    def _publish(self, v):
        P = self.tick - 1 if self._in_command else self.tick
        self.log[v].append((P, int(self.biditer[v]), self.price[v].copy(), self.who[v].copy()))
        self.last_pub[v] = P

    def command(self, v, c, q, Rt):
        self._in_command = True
        try:
            super().command(v, c, q, Rt)
        finally:
            self._in_command = False

    def quiescent(self):
        return not any(self.log) and not any(
            self.open[v] and self.queue[v] for v in range(self.n))

    def _deliver(self):
        T = self.tick
        overflow = False
        subs = [self.subscribed(w) for w in range(self.n)]
        for u in range(self.n):  # ascending sender id, its bids in publication order
            for P, it, pr, wh in self.log[u]:
                for w in range(self.n):
                    if u not in subs[w] or P + self.lat[w][u] != T:
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
