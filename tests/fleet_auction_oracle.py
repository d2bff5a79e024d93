"""Plain-Python restatement of the fleet auction model (acl_fleet_auction_batch,
include/aclswarm_amd.h): one swarm of n reference Auctioneers with their
receive queues (deques) and START / current / next buckets (dicts), advanced
tick by tick.

TEST INFRASTRUCTURE ONLY: imported by tests/, never by the product package.

The tallies and price rows are oracle/cbaa_step_oracle.py's (step, price_row);
the alignment Rt of a starting vehicle is an input (the tests compute it with
the CPU oracle, or hand over the device's after checking its bits). Restates
  flush      auctioneer.cpp:66-74      start      :78-120
  tick       :139-160                  processBid :182-306
  shouldUseAssignment :310-321         isValidAssignment :325-343
  bidIterComplete :419-437             reset      :448-465
  subscriptions: connectToNeighbors, coordination_ros.cpp:392-428.
"""
from collections import deque

import numpy as np

import cbaa_step_oracle as S

NONE, START, FLUSH = 0, 1, 2
QUIESCENT, OVERFLOW = 0x1, 0x2
V_STARTED, V_BAD_ROW, V_CONSENSUS, V_ADOPTED, V_INVALID, V_OVERFLOW = (
    0x01, 0x02, 0x04, 0x08, 0x10, 0x20)


class Fleet:
    """One swarm. p [n][3], adj [n][n] (adj[i][j] = adjmat(i, j)); Pt [n][n]:
    vehicle v's own row, formation point -> vehicle (None: identity)."""

    def __init__(self, p, adj, Pt=None, queue_cap=None, max_iter=0):
        self.p = np.asarray(p, np.float64)
        self.adj = np.asarray(adj)
        n = self.n = self.p.shape[0]
        self.cap = 4 * n if queue_cap is None else int(queue_cap)
        self.max_iter = max_iter if max_iter > 0 else 2 * n
        self.Pt = (np.tile(np.arange(n), (n, 1)) if Pt is None else
                   np.array(Pt, np.int64).reshape(n, n))
        self.open = np.zeros(n, np.uint8)
        self.invalid = np.zeros(n, np.uint8)
        self.just_received = np.ones(n, np.uint8)
        self.biditer = np.zeros(n, np.int32)
        self.price = np.zeros((n, n), np.float32)
        self.who = np.full((n, n), -1, np.int32)
        self.Rt = np.zeros((n, 6))
        self.qv = np.zeros((n, 3))
        self.final_price = np.zeros((n, n), np.float32)
        self.final_who = np.full((n, n), -1, np.int32)
        self.done_tick = np.full(n, -1, np.int32)
        self.vflags = np.zeros(n, np.int32)
        self.n_thrown = np.zeros(n, np.int32)
        self.n_tally = np.zeros(n, np.int32)
        self.zero = [dict() for _ in range(n)]
        self.curr = [dict() for _ in range(n)]
        self.next = [dict() for _ in range(n)]
        self.queue = [deque() for _ in range(n)]
        self.inflight = [[] for _ in range(n)]  # per sender: [(iter, price, who)] in order
        self.tick = 0
        self.max_queue = 0  # the longest queue seen

    # -- helpers --
    def _point(self, w):
        """The point of w under its own row; None when the row is no permutation."""
        row = self.Pt[w]
        if sorted(row.tolist()) != list(range(self.n)):
            return None
        return int(np.where(row == w)[0][0])

    def subscribed(self, w):
        i = self._point(w)
        if i is None:
            return set()
        return {int(self.Pt[w][j]) for j in range(self.n) if self.adj[i][j]}

    def _reset(self, v):
        self.open[v] = 0
        self.biditer[v] = 0
        self.price[v] = 0.0
        self.who[v] = -1
        self.curr[v] = {}
        self.next[v] = {}

    def _publish(self, v):
        self.inflight[v].append((int(self.biditer[v]), self.price[v].copy(), self.who[v].copy()))

    def queue_len(self):
        return np.array([len(x) for x in self.queue], np.int32)

    def quiescent(self):
        return not any(self.inflight) and not any(
            self.open[v] and self.queue[v] for v in range(self.n))

    # -- the model --
    def command(self, v, c, q, Rt):
        if c == FLUSH:
            self._reset(v)
            self.zero[v] = {}
            self.queue[v].clear()
            self.invalid[v] = 0
        elif c == START:
            self._reset(v)
            if self._point(v) is None:
                self.vflags[v] |= V_BAD_ROW
                return
            self.curr[v] = self.zero[v]
            self.zero[v] = {}
            self.Rt[v] = Rt[v]
            self.qv[v] = q[v]
            row = S.price_row(self.p, self.qv[v], self.Rt[v])
            self.price[v], self.who[v], _, _ = S.step(v, True, self.price[v], self.who[v], [], row)
            self.open[v] = 1
            self.vflags[v] |= V_STARTED
            self._publish(v)

    def _deliver(self):
        overflow = False
        subs = [self.subscribed(w) for w in range(self.n)]
        for u in range(self.n):  # ascending sender id
            for it, pr, wh in self.inflight[u]:
                for w in range(self.n):
                    if u not in subs[w]:
                        continue
                    if len(self.queue[w]) >= self.cap:
                        self.vflags[w] |= V_OVERFLOW
                        overflow = True
                        continue
                    self.queue[w].append((u, it, pr, wh))
                    self.max_queue = max(self.max_queue, len(self.queue[w]))
            self.inflight[u] = []
        return overflow

    def _process(self, v):
        n = self.n
        u, it, pr, wh = self.queue[v].popleft()
        if it == 0:
            self.zero[v].setdefault(u, (pr, wh))
        if it == self.biditer[v]:
            self.curr[v].setdefault(u, (pr, wh))
        elif it == self.biditer[v] + 1:
            self.next[v].setdefault(u, (pr, wh))
        else:
            self.n_thrown[v] += 1
        if not self.subscribed(v) <= set(self.curr[v]):
            return
        cands = dict(self.curr[v])
        cands.setdefault(v, (self.price[v].copy(), self.who[v].copy()))
        cl = [(k, t[0], t[1]) for k, t in sorted(cands.items())]
        row = S.price_row(self.p, self.qv[v], self.Rt[v])
        self.price[v], self.who[v], _, _ = S.step(v, False, self.price[v], self.who[v], cl, row)
        self.n_tally[v] += 1
        self.biditer[v] += 1
        self.curr[v] = self.next[v]
        self.next[v] = {}
        if self.biditer[v] == 1:
            self.zero[v] = {}
        if self.biditer[v] >= self.max_iter:
            self.final_price[v] = self.price[v]
            self.final_who[v] = self.who[v]
            self.done_tick[v] = self.tick
            self.vflags[v] |= V_CONSENSUS
            if sorted(self.who[v].tolist()) == list(range(n)):
                if self.just_received[v] or (self.who[v] != self.Pt[v]).any():
                    self.just_received[v] = 0
                    self.Pt[v] = self.who[v]
                    self.vflags[v] |= V_ADOPTED
            else:
                self.invalid[v] = 1
                self.vflags[v] |= V_INVALID
            self._reset(v)
        else:
            self._publish(v)

    def run(self, ticks, q=None, cmd=None, Rt=None, hist=None):
        """Commands, then up to `ticks` ticks. hist: a list that receives one
        (biditer, open) copy per tick (rows past quiescence repeat the last).
        Returns the status dict of the call."""
        if cmd is not None:
            for v in range(self.n):
                if cmd[v] in (START, FLUSH):
                    self.command(v, int(cmd[v]), q, Rt)
        t = 0
        overflow = False
        while t < ticks and not self.quiescent():
            overflow |= self._deliver()
            for v in range(self.n):
                if self.open[v] and self.queue[v]:
                    self._process(v)
            self.tick += 1
            t += 1
            if hist is not None:
                hist.append((self.biditer.copy(), self.open.copy()))
        if hist is not None:
            for _ in range(t, ticks):
                hist.append((self.biditer.copy(), self.open.copy()))
        return dict(ticks_run=t, n_open=int(self.open.sum()),
                    n_queued=int(self.queue_len().sum()),
                    flags=(QUIESCENT if self.quiescent() else 0) | (OVERFLOW if overflow else 0))
