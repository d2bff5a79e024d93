"""Plain-Python restatement of fleet localization on real links
(acl_fleet_delay_localize_batch, include/aclswarm_amd.h):
fleet_localize_oracle.Trackers with two sentences of one_round changed. A
receiver takes the table its sender published tlat[w][u] rounds ago, if the
publication log still (or already) holds it, and loses it by the hash of the
publication round; a vehicle whose feed is out in a round does not sense.

TEST INFRASTRUCTURE ONLY: imported by tests/, never by the product package.
"""
import numpy as np

import fleet_localize_oracle as GO
import fleet_loss_oracle as LO

FEED_ITER = 0xFFFFFFFE  # the iter word of a feed outage: no bid or table has it
MAX_TLAT = 7


def tlat_matrix(n, tlat):
    """An int (every link) or [n][n] (receiver-major) as an [n][n] int array."""
    t = np.asarray(tlat, np.int64)
    return np.full((n, n), int(t)) if t.ndim == 0 else t.reshape(n, n).copy()


def feed_vector(n, feed):
    f = np.asarray(feed, np.int64)
    v = np.full(n, int(f)) if f.ndim == 0 else f.reshape(n).copy()
    assert v.min() >= 0 and v.max() <= LO.DEAD
    return v


class DelayedTrackers(GO.Trackers):
    """One swarm. tlat, feed_loss, loss, seed and Pt are attributes the caller
    may rewrite between runs; max_tlat is fixed (it sizes the log). log: slot
    -> (publication round, the published tables), max_tlat + 1 slots; empty: a
    zero-filled workspace. delayed = False runs the rounds of
    acl_fleet_localize_batch instead (the log stands still)."""

    def __init__(self, adj, Pt=None, loss=0, seed=0, tlat=0, max_tlat=None, feed_loss=0):
        super().__init__(adj, Pt=Pt, loss=loss, seed=seed)
        self.tlat = tlat_matrix(self.n, tlat)
        self.max_tlat = int(self.tlat.max()) if max_tlat is None else int(max_tlat)
        assert 0 <= self.max_tlat <= MAX_TLAT
        self.feed_loss = feed_vector(self.n, feed_loss)
        self.n_missed = [0] * self.n
        self.log = {}
        self.delayed = True
        self.taken_trace = None  # a list: receives (round, receiver, sender, publication round)

    def bad_tlat(self):
        off = self.tlat[~np.eye(self.n, dtype=bool)]
        return bool(off.size) and (int(off.max()) > self.max_tlat or int(off.min()) < 0)

    def feed_out(self, w, r):
        return LO.is_lost(int(self.feed_loss[w]), self.seed, w, w, r, FEED_ITER) \
            if self.feed_loss[w] else False

    def one_round(self, q):
        if not self.delayed:
            return super().one_round(q)
        assert not self.bad_tlat()  # (such a swarm is untouched: the caller does not run it)
        n, r, M1 = self.n, self.round, self.max_tlat + 1
        for w in range(n):  # 1. sense, unless the feed is out
            if self.feed_out(w, r):
                self.n_missed[w] += 1
            else:
                self.tab[w][w] = (r + 1, tuple(float(x) for x in q[w]))
        self.log[r % M1] = (r, [dict(t) for t in self.tab])  # 2. publish, by copy
        for w in range(n):  # 3. merge what is due
            senders = self.subscribed(w)
            if self.order is not None:
                senders = self.order(w, senders)
            got = []
            for u in senders:
                P = r - (0 if u == w else int(self.tlat[w][u]))
                slot = self.log.get(P % M1)
                if P < 0 or slot is None or slot[0] != P:
                    continue  # no such table: not delivered, not lost
                if LO.is_lost(int(self.loss[w][u]), self.seed, w, u, P, GO.GOSSIP_ITER):
                    self.n_lost[w] += 1
                    if self.lost_trace is not None:
                        self.lost_trace.append((r, w, u))
                    continue
                got.append((u, slot[1][u]))
                if self.taken_trace is not None:
                    self.taken_trace.append((r, w, u, P))
            for i in range(n):
                best, who = self.tab[w][i], -1  # its own stays on ties
                for u, pub in got:
                    e = pub[i]
                    if e[0] > best[0] or (who >= 0 and e[0] == best[0] and u < who):
                        best, who = e, u
                self.tab[w][i] = best
        self.round = r + 1

    def log_bytes(self):
        """The swarm's part of the workspace as the header lays it out."""
        n, M1 = self.n, self.max_tlat + 1
        tags = np.zeros(8, np.int32)
        est = np.zeros((M1, n, n, 3), np.float64)
        st = np.zeros((M1, n, n), np.int32)
        for s, (P, pub) in self.log.items():
            tags[s] = P + 1
            for w in range(n):
                for i in range(n):
                    st[s, w, i] = pub[w][i][0]
                    est[s, w, i] = pub[w][i][1]
        raw = tags.tobytes() + est.tobytes() + st.tobytes()
        return raw + b"\0" * (-len(raw) % 8)
