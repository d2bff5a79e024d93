"""Plain-Python restatement of acl_fleet_episode_batch (include/aclswarm_amd.h):
one swarm flown with every vehicle its own Auctioneer.

TEST INFRASTRUCTURE ONLY: imported by tests/, never by the product package.

Composes, per control step s, in the model's order:
  1. every vehicle's own autoauctionCb (coordination_ros.cpp:322-359) when
     s % auction_every == 0: FLUSH for a vehicle whose last auction converged
     on an invalid table, START from the current q for every other (a restart
     when its auctioneer is open);
  2. ticks_per_step ticks of fleet_auction_oracle.Fleet;
  3. the hand-off (newAssignmentCb, :284-303): every vehicle flies its own
     row; the swarm flies one table when all rows are equal;
  4. episode_oracle.control_step(..., tables=rows);
  5. episode_oracle.make_safe_traj and episode_oracle.Supervisor.
"""
import numpy as np

import episode_oracle as E
import fleet_auction_cases as C
import fleet_auction_oracle as FO


class FleetEpisode:
    """One swarm. p [n][3], adj [n][n], gains [3n][3n]; q, vel [n][3]; Pt
    [n][n] the vehicles' own rows (None: identity); ep: a dict as
    episode_oracle.default_params() (auction_latency and assignment 0)."""

    def __init__(self, p, adj, gains, q, vel, ep, Pt=None, queue_cap=None, max_iter=0,
                 ticks_per_step=10, g=None, s=None):
        assert ticks_per_step >= 1
        assert ep.get("auction_latency", 0) == 0 and ep.get("assignment", 0) == 0
        self.p, self.adj, self.gains = np.asarray(p, np.float64), np.asarray(adj), gains
        self.n = n = len(self.p)
        self.ep, self.T, self.g, self.s = ep, int(ticks_per_step), g, s
        self.fleet = FO.Fleet(self.p, self.adj, Pt=Pt, queue_cap=queue_cap, max_iter=max_iter)
        self.q = np.array(q, np.float64)
        self.vel = np.array(vel, np.float64)
        self.sup = E.Supervisor(n, ep)
        self.step_no = 0
        self.vflags = np.zeros(n, np.int32)  # sticky
        self.adopt_step = np.full(n, -1, np.int32)
        self.per_vehicle = 0
        self.P = self.points()
        self.converged_step = self.gridlock_step = -1
        self.n_ca_steps = 0
        self.fst = dict(flags=0, ticks_run=0, n_started=0, n_restarted=0, n_flushed=0,
                        n_consensus=0, n_adopted=0, n_invalid=0)

    def points(self):
        """Each vehicle's point in its own row."""
        Pt = self.fleet.Pt
        return np.array([int(np.nonzero(Pt[v] == v)[0][0]) for v in range(self.n)], np.uint16)

    def auto_cmd(self):
        """Step (1) for the fleet's present flags."""
        return np.where(self.fleet.invalid != 0, FO.FLUSH, FO.START).astype(np.uint8)

    def step(self, Rt=None, sup=None):
        """One control step. Rt [n][6]: the alignments handed to an
        auto-auction's START commands (default: the CPU oracle's under the
        vehicles' rows). sup: (u [n][3], ca [n]) the supervisor samples instead
        of the step's own (the GPU tests hand over the recorded commands).
        Returns the step's record."""
        fl, n, s = self.fleet, self.n, self.step_no
        cmd = None
        if s % self.ep["auction_every"] == 0:
            cmd = self.auto_cmd()
            start = cmd == FO.START
            self.fst["n_started"] += int(start.sum())
            self.fst["n_restarted"] += int((start & (fl.open != 0)).sum())
            self.fst["n_flushed"] += int((cmd == FO.FLUSH).sum())
            if Rt is None:
                Rt = C.align_rt(self.p, self.adj, self.q, fl.Pt)
        fl.vflags[:] = 0
        st = fl.run(self.T, q=self.q, cmd=cmd, Rt=Rt)
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
        # (the rows change by adoption only, so this is the device's hand-off,
        # rebuilt at an adoption and at the first step of a call)
        self.per_vehicle = int(not (fl.Pt == fl.Pt[0]).all())
        self.P = self.points()
        u, us, ca = E.control_step(self.q, self.vel, self.p, self.adj, self.gains, self.P,
                                   self.g, self.s, tables=fl.Pt.astype(np.uint16))
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
                    P=self.P.copy(), per_vehicle=self.per_vehicle)
