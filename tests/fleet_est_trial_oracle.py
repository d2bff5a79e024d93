"""Plain-Python restatement of acl_fleet_est_trial_batch
(include/aclswarm_amd.h): fleet_loss_trial_oracle.LossyFleetTrial in which no
vehicle reads the shared snapshot. The swarm's auctioneers are a
fleet_est_oracle.EstFleet, its VehicleTrackers a fleet_localize_oracle.Trackers
under the adjacency of the formation the swarm flies and under loc_rows, the
vehicles' LOCALIZATION rows: the assignment each vehicle last published
(LocalizationROS::assignmentCb, localization_ros.cpp:89-97), which a commit
does not touch (formationCb, :77-85, replaces the adjacency only). Per control
step s, in the model's order:
  1. the commit and the commands of fleet_trial_oracle.FleetTrial.pre; the
     trackers and loc_rows survive;
  2. if s % track_every == 0, one gossip round on the true q, after the commit,
     subscribed under loc_rows;
  3. ticks_per_step ticks of the EstFleet: a START of vehicle v reads its own
     table (the alignment handed in is fleet_est_oracle.align_rt's);
  4. the hand-off; an adopting vehicle publishes: loc_rows[v] = its row;
  5. fleet_est_control_oracle.control_step on the tables;
  6. the record: the round's status, and with diag the error maxima, err2_nbr
     over the running controllers only;
  7. TrialSwarm.traj and the Supervisor on the true q.

loc_rows_follow="auction" is the WRONG model, kept for the distinguishing test:
the gossip subscribes under the auctioneers' rows of the moment (the identity
after a commit).

TEST INFRASTRUCTURE ONLY: imported by tests/, never by the product package.
"""
import numpy as np

import fleet_auction_oracle as FO
import fleet_est_control_oracle as EC
import fleet_est_oracle as EO
import fleet_localize_oracle as GO
import fleet_loss_trial_oracle as LT
import fleet_trial_oracle as FT


def err2_record(est, stamps, q, Pt, adj, on):
    """fleet_est_episode_oracle.err2_record with the trial's sentence: nbr runs
    over the vehicles v with on[v] only."""
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
        if on[v]:
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


class EstFleetTrial(LT.LossyFleetTrial):
    """One swarm. track_every >= 1; diag: whether the error record runs;
    loc_rows_follow: "published" (the model) or "auction"; the other arguments
    are LossyFleetTrial's."""

    def __init__(self, fseq, forms, q, vel, tp, lat, loss=0, seed=0, queue_cap=None, max_iter=0,
                 ticks_per_step=10, g=None, s=None, track_every=2, diag=False,
                 loc_rows_follow="published"):
        assert track_every >= 1 and loc_rows_follow in ("published", "auction")
        super().__init__(fseq, forms, q, vel, tp, lat, loss=loss, seed=seed, queue_cap=queue_cap,
                         max_iter=max_iter, ticks_per_step=ticks_per_step, g=g, s=s)
        p, adj, _ = forms[self.t.fidx]
        fl = self.fleet = EO.EstFleet(p, adj, lat, loss=loss, seed=seed, queue_cap=queue_cap,
                                      max_iter=max_iter)
        # acl_fleet_est_trial_init: freshly constructed auctioneers, every output 0
        fl.just_received[:] = 0
        fl.final_who[:] = 0
        fl.done_tick[:] = 0
        self.P = self.points()
        n = self.n
        self.track_every, self.diag, self.follow = int(track_every), bool(diag), loc_rows_follow
        self.loc_rows = np.tile(np.arange(n), (n, 1))  # identity rows
        self.trackers = GO.Trackers(adj, Pt=self.loc_rows, loss=fl.loss, seed=fl.seed)
        self.xst = dict(rounds_run=0, n_unknown=0, max_age=0, flags=0, err2_own=0.0,
                        err2_nbr=0.0, err2_all=0.0)

    def gossip_rows(self):
        """The rows the round of this moment subscribes under."""
        return np.array(self.loc_rows if self.follow == "published" else self.fleet.Pt, np.int64)

    def gossip(self):
        """Stage 2: one round under the current formation's adjacency, the
        localization rows and the fleet's loss and seed of the moment."""
        tr, fl = self.trackers, self.fleet
        tr.adj = np.asarray(self.forms[self.t.fidx][1])
        tr.Pt = self.gossip_rows()
        tr.loss, tr.seed = fl.loss, fl.seed
        st = tr.run(1, self.q)
        self.xst["rounds_run"] += st["rounds_run"]
        self.xst["n_unknown"], self.xst["max_age"] = st["n_unknown"], st["max_age"]
        return st

    def step(self, Rt=None, sup=None, own=True):
        """One control step; Rt and sup as FleetTrial.step takes them. own=False:
        the step of acl_fleet_lossy_trial_batch (the shared snapshot; the
        trackers and loc_rows stand still). The record also holds the tables the
        step flew (est, stamps), the rows its round subscribed under
        (gossip_rows, None without one), the localize status of the round (loc),
        the control status (cst), err2 (None without diag or for a finished
        trial) and loc_rows after the step."""
        if not own:
            return super().step(Rt=Rt, sup=sup)
        t, fl, n, s = self.t, self.fleet, self.n, self.step_no
        snap = dict(open=fl.open.copy(), queued=fl.queue_len(), inflight=self.in_flight())
        lost0 = int(fl.n_lost.sum())
        committed = bool(t.sup.commit) and not t.done and not self.fbad
        cmd, live = self.pre()
        raised = np.zeros(n, np.int32)
        loc = grows = cst = err2 = None
        if not live:
            st = dict(ticks_run=0, n_open=0, n_queued=0, flags=FT.BAD_INPUT)
            u = np.zeros((n, 3))
            us = np.zeros((n, 3))
            ca = np.zeros(n, np.uint8)
            est, stamps = self.trackers.est(), self.trackers.stamps()
        else:
            p, adj, G = self.forms[t.fidx]
            if s % self.track_every == 0:
                grows = self.gossip_rows()
                loc = self.gossip()
            est, stamps = self.trackers.est(), self.trackers.stamps()
            if cmd is not None and Rt is None:
                Rt = EO.align_rt(p, adj, est, fl.Pt)
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
            t.ctl_on[adopted] = True  # first_assignment_
            if adopted[0]:
                t.sup.assignment_msg()
            # newAssignmentCb publishes the row: the localization node's P_
            self.loc_rows[adopted] = fl.Pt[adopted]
            self.per_vehicle = int(not (fl.Pt == fl.Pt[0]).all())
            self.P = self.points()
            u, us, ca, cst = EC.control_step(est, self.vel, fl.Pt, p, adj, G, self.g, self.s)
            if self.diag:
                err2 = err2_record(est, stamps, self.q, fl.Pt, adj, t.ctl_on)
                for k, x in zip(("err2_own", "err2_nbr", "err2_all"), err2):
                    if x > self.xst[k]:
                        self.xst[k] = x
        on = t.ctl_on & (not t.done)
        self.q, self.vel = t.traj(self.q, self.vel, us)
        if s % self.tp["ep"]["sample_every"] == 0:
            su, sc, sq = sup if sup is not None else (u, ca, self.q)
            sp, cs = t.samples(su, sc)
            t.sup.tick(s, sp, cs, sq)
        self.step_no += 1
        return dict(step=s, cmd=cmd, status=st, raised=raised, u=u, us=us, ca=ca, on=on,
                    P=self.P.copy(), per_vehicle=self.per_vehicle, committed=committed,
                    before=snap, state=t.sup.state, ctl_on=t.ctl_on.copy(),
                    n_thrown=fl.n_thrown.copy(), invalid=fl.invalid.copy(), open=fl.open.copy(),
                    lost=int(fl.n_lost.sum()) - lost0, est=est, stamps=stamps, loc=loc, cst=cst,
                    err2=err2, gossip_rows=grows, loc_rows=self.loc_rows.copy(),
                    Pt=np.array(fl.Pt, np.int64), live=live, fidx=int(t.fidx))
