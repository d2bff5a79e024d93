"""Plain-Python restatement of the fleet localization model
(acl_fleet_localize_batch, include/aclswarm_amd.h): one swarm of n
VehicleTrackers (localization_ros.cpp, vehicle_tracker.cpp), each a table of
(stamp, position) per vehicle held in dicts and lists, advanced round by round:
sense, publish, merge the subscribed neighbours' published tables entry by
entry iff the stamp is strictly later (vehicle_tracker.cpp:31-45).

TEST INFRASTRUCTURE ONLY: imported by tests/, never by the product package.
"""
import numpy as np

import fleet_loss_oracle as LO

BAD_INPUT, BAD_ROW = 0x4, 0x8
GOSSIP_ITER = 0xFFFFFFFF  # the iter word of a table's link_hash: no bid has it


class Trackers:
    """One swarm. adj [n][n]; Pt [n][n]: vehicle w's own row, formation point
    -> vehicle (None: identity), an attribute the caller may rewrite between
    runs, like loss ([n][n] or an int) and seed. order: the order in which a
    receiver visits its senders (None: ascending id); the result must not
    depend on it."""

    def __init__(self, adj, Pt=None, loss=0, seed=0):
        self.adj = np.asarray(adj)
        n = self.n = len(self.adj)
        self.Pt = (np.tile(np.arange(n), (n, 1)) if Pt is None else
                   np.array(Pt, np.int64).reshape(n, n))
        self.loss = LO.loss_matrix(n, loss)
        self.seed = int(seed) & LO.M32
        # tab[w][i] = (stamp, (x, y, z)); stamp 0: never heard
        self.tab = [{i: (0, (0.0, 0.0, 0.0)) for i in range(n)} for _ in range(n)]
        self.round = 0
        self.n_lost = [0] * n
        self.order = None
        self.lost_trace = None  # a list: receives (round, receiver, sender)

    def _point(self, w):
        row = self.Pt[w]
        if sorted(row.tolist()) != list(range(self.n)):
            return None
        return int(np.where(row == w)[0][0])

    def subscribed(self, w):
        i = self._point(w)
        if i is None:
            return []
        return sorted({int(self.Pt[w][j]) for j in range(self.n) if self.adj[i][j]})

    def one_round(self, q):
        n, r = self.n, self.round
        for w in range(n):  # 1. sense
            self.tab[w][w] = (r + 1, tuple(float(x) for x in q[w]))
        pub = [dict(t) for t in self.tab]  # 2. publish
        for w in range(n):  # 3. merge
            senders = self.subscribed(w)
            if self.order is not None:
                senders = self.order(w, senders)
            got = []
            for u in senders:
                if LO.is_lost(int(self.loss[w][u]), self.seed, w, u, r, GOSSIP_ITER):
                    self.n_lost[w] += 1
                    if self.lost_trace is not None:
                        self.lost_trace.append((r, w, u))
                    continue
                got.append(u)
            for i in range(n):
                best, who = self.tab[w][i], -1  # its own stays on ties
                for u in got:
                    e = pub[u][i]
                    # strictly later; among equally late senders the lowest id
                    if e[0] > best[0] or (who >= 0 and e[0] == best[0] and u < who):
                        best, who = e, u
                self.tab[w][i] = best
        self.round = r + 1

    def run(self, rounds, q):
        """q [n][3] (the same snapshot every round) or [rounds][n][3].
        Returns the status dict of the call."""
        q = np.asarray(q, np.float64)
        for t in range(rounds):
            self.one_round(q if q.ndim == 2 else q[t])
        return self.status(rounds)

    # -- what the kernel hands back --
    def stamps(self):
        return np.array([[self.tab[w][i][0] for i in range(self.n)] for w in range(self.n)],
                        np.int32)

    def est(self):
        return np.array([[self.tab[w][i][1] for i in range(self.n)] for w in range(self.n)],
                        np.float64).reshape(self.n, self.n, 3)

    def status(self, rounds_run=0):
        st = self.stamps()
        known = st != 0
        bad = any(self._point(w) is None for w in range(self.n))
        return dict(rounds_run=rounds_run, n_unknown=int((~known).sum()),
                    max_age=int((self.round - st[known]).max()) if known.any() else 0,
                    flags=BAD_ROW if bad else 0)


BAD_FIDX_STATUS = dict(rounds_run=0, n_unknown=0, max_age=0, flags=BAD_INPUT)
