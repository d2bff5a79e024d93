"""Plain-Python restatement of the fleet auction started from each vehicle's
own estimates (acl_fleet_est_auction_batch, include/aclswarm_amd.h):
fleet_loss_oracle's LossyFleet with one sentence changed. A START of vehicle v
reads snapshot est[v] wherever the lossy fleet reads q: the alignment handed in
(Rt[v]) is the one to est[v]'s rows under the vehicle's own row, and row v of
est[v] is the start position it stores and prices from.

TEST INFRASTRUCTURE ONLY: imported by tests/, never by the product package.
"""
import numpy as np

import fleet_loss_oracle as LO
import pyoracle as O


def align_rt(p, adj, est, rows):
    """Rt [n][6] of every vehicle under its own row from its own snapshot
    est[v] (the CPU oracle's alignment, as fleet_auction_cases.align_rt)."""
    n = len(rows)
    out = np.zeros((n, 6))
    for v in range(n):
        if sorted(np.asarray(rows[v]).tolist()) != list(range(n)):
            continue  # a bad row starts nothing
        R, t = O.align(n, v, np.ascontiguousarray(est[v], np.float64), p, adj,
                       np.argsort(rows[v]).astype(np.uint16))
        out[v] = np.concatenate([R.reshape(4), t])
    return out


class EstFleet(LO.LossyFleet):
    """One swarm. run(..., est=) takes est [n][n][3]; with est None every
    vehicle's snapshot is q (the lossy fleet's call, through this class's
    command)."""

    _est = None

    def command(self, v, c, q, Rt):
        super().command(v, c, None if self._est is None else self._est[v], Rt)

    def run(self, ticks, q=None, cmd=None, Rt=None, hist=None, est=None):
        if est is None and q is not None:
            est = np.broadcast_to(np.asarray(q, np.float64), (self.n, self.n, 3))
        self._est = None if est is None else np.asarray(est, np.float64)
        return super().run(ticks, q=None, cmd=cmd, Rt=Rt, hist=hist)
