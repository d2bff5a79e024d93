"""Plain-Python restatement of acl_fleet_est_episode_batch
(include/aclswarm_amd.h): fleet_loss_episode_oracle.LossyFleetEpisode in which
no vehicle reads the shared snapshot. The swarm's auctioneers are a
fleet_est_oracle.EstFleet, its VehicleTrackers a fleet_localize_oracle.Trackers
whose rows, loss matrix and seed follow the fleet's. Per control step s, in the
model's order:
  0. if s % track_every == 0, one gossip round on the true q;
  1. every vehicle's own autoauctionCb;
  2. ticks_per_step ticks of the EstFleet: a START of vehicle v reads its own
     table (the alignment handed in is fleet_est_oracle.align_rt's);
  3. the hand-off;
  4. fleet_est_control_oracle.control_step on the tables;
  5. (diag) the estimate-error record;
  6. episode_oracle.make_safe_traj and the Supervisor on the true q.

TEST INFRASTRUCTURE ONLY: imported by tests/, never by the product package.
"""
import numpy as np

import episode_oracle as E
import fleet_auction_oracle as FO
import fleet_est_control_oracle as EC
import fleet_est_oracle as EO
import fleet_localize_oracle as GO
import fleet_loss_episode_oracle as LE


def err2_record(est, stamps, q, Pt, adj):
    """The three maxima of step 5: (own, nbr, all) of
    d2(v, j) = (dx dx + dy dy) + dz dz with d = est[v][j] - q[j], in Python
    floats (IEEE doubles, one operation each). Every maximum starts from +0.0
    and takes d2 > m only."""
    n = len(q)

    def d2(v, j):
        dx = float(est[v][j][0]) - float(q[j][0])
        dy = float(est[v][j][1]) - float(q[j][1])
        dz = float(est[v][j][2]) - float(q[j][2])
        return (dx * dx + dy * dy) + dz * dz
    own = nbr = every = 0.0
    for v in range(n):
        row = [int(x) for x in Pt[v]]
        x = d2(v, v)
        if x > own:
            own = x
        i = row.index(v)
        for jj in range(n):
            if adj[i][jj]:
                x = d2(v, row[jj])
                if x > nbr:
                    nbr = x
        for j in range(n):
            if j != v and stamps[v][j] != 0:
                x = d2(v, j)
                if x > every:
                    every = x
    return own, nbr, every


class EstFleetEpisode(LE.LossyFleetEpisode):
    """One swarm. track_every >= 1; diag: whether step 5 runs; the other
    arguments are LossyFleetEpisode's."""

    def __init__(self, p, adj, gains, q, vel, ep, lat, loss=0, seed=0, Pt=None, queue_cap=None,
                 max_iter=0, ticks_per_step=10, g=None, s=None, track_every=2, diag=False):
        assert track_every >= 1
        super().__init__(p, adj, gains, q, vel, ep, lat, loss=loss, seed=seed, Pt=Pt,
                         queue_cap=queue_cap, max_iter=max_iter, ticks_per_step=ticks_per_step,
                         g=g, s=s)
        self.fleet = EO.EstFleet(self.p, self.adj, lat, loss=loss, seed=seed, Pt=Pt,
                                 queue_cap=queue_cap, max_iter=max_iter)
        self.P = self.points()
        self.track_every, self.diag = int(track_every), bool(diag)
        self.trackers = GO.Trackers(self.adj, Pt=self.fleet.Pt, loss=self.fleet.loss,
                                    seed=self.fleet.seed)
        self.xst = dict(rounds_run=0, n_unknown=0, max_age=0, flags=0, err2_own=0.0,
                        err2_nbr=0.0, err2_all=0.0)

    def gossip(self):
        """Stage 0: one round under the fleet's rows, loss and seed of the moment."""
        tr, fl = self.trackers, self.fleet
        tr.Pt = np.array(fl.Pt, np.int64)
        tr.loss, tr.seed = fl.loss, fl.seed
        st = tr.run(1, self.q)
        self.xst["rounds_run"] += st["rounds_run"]
        self.xst["n_unknown"], self.xst["max_age"] = st["n_unknown"], st["max_age"]
        return st

    def step(self, Rt=None, sup=None, own=True):
        """One control step; Rt and sup as FleetEpisode.step takes them.
        own=False: the step of acl_fleet_lossy_episode_batch (the shared
        snapshot; the trackers stand still). The record also holds the tables
        the step flew (est, stamps), the localize status of its round (loc,
        None without one), the control status (cst) and err2 (None without
        diag)."""
        if not own:
            return super().step(Rt=Rt, sup=sup)
        fl, s = self.fleet, self.step_no
        snap = dict(open=fl.open.copy(), queued=fl.queue_len(), inflight=self.in_flight())
        lost0 = int(fl.n_lost.sum())
        loc = self.gossip() if s % self.track_every == 0 else None
        est, stamps = self.trackers.est(), self.trackers.stamps()
        cmd = None
        if s % self.ep["auction_every"] == 0:
            cmd = self.auto_cmd()
            start = cmd == FO.START
            self.fst["n_started"] += int(start.sum())
            self.fst["n_restarted"] += int((start & (fl.open != 0)).sum())
            self.fst["n_flushed"] += int((cmd == FO.FLUSH).sum())
            if Rt is None:
                Rt = EO.align_rt(self.p, self.adj, est, fl.Pt)
        fl.vflags[:] = 0
        st = fl.run(self.T, cmd=cmd, Rt=Rt, est=est)
        raised = fl.vflags.copy()
        self.vflags |= raised
        fl.vflags[:] = self.vflags
        self.fst["ticks_run"] += st["ticks_run"]
        self.fst["flags"] |= st["flags"] & FO.OVERFLOW
        for key, bit in (("n_consensus", FO.V_CONSENSUS), ("n_adopted", FO.V_ADOPTED),
                         ("n_invalid", FO.V_INVALID)):
            self.fst[key] += int(((raised & bit) != 0).sum())
        adopted = (raised & FO.V_ADOPTED) != 0
        self.adopt_step[adopted] = s
        self.per_vehicle = int(not (fl.Pt == fl.Pt[0]).all())
        self.P = self.points()
        u, us, ca, cst = EC.control_step(est, self.vel, fl.Pt, self.p, self.adj, self.gains,
                                         self.g, self.s)
        err2 = None
        if self.diag:
            err2 = err2_record(est, stamps, self.q, fl.Pt, self.adj)
            for k, x in zip(("err2_own", "err2_nbr", "err2_all"), err2):
                if x > self.xst[k]:
                    self.xst[k] = x
        self.q, self.vel = E.make_safe_traj(self.q, self.vel, us, self.ep)
        self.n_ca_steps += int(ca.sum())
        if s % self.ep["sample_every"] == 0:
            r = self.sup.tick(*(sup if sup is not None else (u, ca)))
            if r is not None:
                if r[0] and self.converged_step < 0:
                    self.converged_step = s
                if r[1] and self.gridlock_step < 0:
                    self.gridlock_step = s
        self.step_no += 1
        return dict(step=s, cmd=cmd, status=st, raised=raised, u=u, us=us, ca=ca,
                    P=self.P.copy(), per_vehicle=self.per_vehicle, before=snap,
                    lost=int(fl.n_lost.sum()) - lost0, est=est, stamps=stamps, loc=loc, cst=cst,
                    err2=err2)
