"""Plain-Python restatement of acl_fleet_delay_est_trial_batch
(include/aclswarm_amd.h): fleet_est_trial_oracle.EstFleetTrial whose
VehicleTrackers are fleet_delay_localize_oracle.DelayedTrackers -- the gossip
round of stage 2 takes tables whole rounds late and a vehicle's own feed may be
out -- the same move as fleet_delay_est_episode_oracle.py. gossip() hands the
trackers the adjacency of the formation the swarm flies from this step on, the
localization rows, and the fleet's loss and seed of the moment, as before; the
publication log is the trackers' own and no commit touches it, so a table
published under the old formation is delivered, when due, to whoever subscribes
to its sender in the delivery round.

Beside it the encounter record of the header, in numpy float64 with the
header's expression order: encounter_record (one step) and EncounterLog (the
accumulation across steps).

TEST INFRASTRUCTURE ONLY: imported by tests/, never by the product package.
"""
import numpy as np

import fleet_delay_localize_oracle as DG
import fleet_est_trial_oracle as XT
import pyoracle as O

NONE = 0xFFFF


def _s2(d):
    """dx * dx + dy * dy, one IEEE operation each."""
    dx, dy = np.float64(d[0]), np.float64(d[1])
    return np.float64(np.float64(dx * dx) + np.float64(dy * dy))


def _cand(s2, thr):
    """collisionAvoidance's candidate test: !(sqrt(s2) > thr), NaN included."""
    with np.errstate(invalid="ignore"):
        return not (np.sqrt(np.float64(s2)) > np.float64(thr))


def encounter_record(q, est, on, safety=None):
    """One step. q [n][3] true, est [n][n][3] the tables the step's control
    reads, on [n]: whose controller runs this step. Returns dict(sep2, i, j,
    n_breach, n_blind, n_ghost, blind [n], ghost [n])."""
    s = safety or O.default_safety()
    q = np.asarray(q, np.float64)
    est = np.asarray(est, np.float64)
    n = len(q)
    keep2 = np.float64(s.r_keep_out) * np.float64(s.r_keep_out)
    best, bi, bj, breach = np.float64(np.inf), NONE, NONE, 0
    for i in range(n):
        for j in range(i + 1, n):
            x = _s2(q[j] - q[i])
            # ascending (i, j): strict < keeps the lowest pair among equals; an
            # infinite value names the lowest pair that holds it
            if x < best or (x == best and bi == NONE):
                best, bi, bj = x, i, j
            if x < keep2:
                breach += 1
    blind, ghost = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for v in range(n):
        if not on[v]:
            continue
        for j in range(n):
            if j == v:
                continue
            ct = _cand(_s2(q[j] - q[v]), s.d_avoid_thresh)
            ce = _cand(_s2(est[v][j] - est[v][v]), s.d_avoid_thresh)
            blind[v] += ct and not ce
            ghost[v] += (not ct) and ce
    return dict(sep2=best, i=bi, j=bj, n_breach=breach, n_blind=int(blind.sum()),
                n_ghost=int(ghost.sum()), blind=blind, ghost=ghost)


class EncounterLog:
    """enc[b], enc_blind[b] and enc_ghost[b] of one swarm."""

    def __init__(self, n):
        self.status = dict(sep2_min=np.float64(np.inf), step=-1, i=NONE, j=NONE, n_breach=0,
                           n_blind=0, n_ghost=0)
        self.blind, self.ghost = np.zeros(n, np.int32), np.zeros(n, np.int32)

    def add(self, step, rec):
        st = self.status
        if rec["sep2"] < st["sep2_min"]:  # strictly: the earliest step keeps the record
            st.update(sep2_min=rec["sep2"], step=int(step), i=rec["i"], j=rec["j"])
        for k in ("n_breach", "n_blind", "n_ghost"):
            st[k] += rec[k]
        self.blind += rec["blind"]
        self.ghost += rec["ghost"]


class DelayEstFleetTrial(XT.EstFleetTrial):
    """One swarm. tlat: an int or [n][n]; max_tlat; feed_loss: an int or [n];
    encounters: whether the record is kept; the other arguments are
    EstFleetTrial's."""

    def __init__(self, *args, tlat=0, max_tlat=None, feed_loss=0, encounters=True, **kw):
        super().__init__(*args, **kw)
        tr = self.trackers
        self.trackers = DG.DelayedTrackers(tr.adj, Pt=self.loc_rows, loss=tr.loss, seed=tr.seed,
                                           tlat=tlat, max_tlat=max_tlat, feed_loss=feed_loss)
        self.enc = EncounterLog(self.n) if encounters else None

    def step(self, Rt=None, sup=None, own=True, delayed=True):
        """EstFleetTrial.step. delayed=False: the step of
        acl_fleet_est_trial_batch (tables within the round, no record; the log
        stands still). The record also holds enc, the step's encounter_record
        (None without the record, for a finished trial, or when not delayed)."""
        q0 = self.q.copy()
        self.trackers.delayed = bool(delayed)
        r = super().step(Rt=Rt, sup=sup, own=own)
        r["enc"] = None
        if own and delayed and self.enc is not None and r["live"]:
            # est: the tables after the step's round; ctl_on: after the hand-off
            r["enc"] = encounter_record(q0, r["est"], r["ctl_on"], self.s)
            self.enc.add(r["step"], r["enc"])
        return r
