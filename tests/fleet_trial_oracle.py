"""Plain-Python restatement of acl_fleet_trial_batch (include/aclswarm_amd.h):
one swarm's trial flown with every vehicle its own Auctioneer.

TEST INFRASTRUCTURE ONLY: imported by tests/, never by the product package.

Composes, per control step s, in the model's order:
  1. the commit of a formation the last supervisor tick requested, as
     trial_oracle.TrialSwarm.pre does (controllers stop, one zero command,
     the countdown restarts at settle_steps), and every vehicle's
     Auctioneer::setFormation (auctioneer.cpp:42-62) on
     fleet_auction_oracle.Fleet: _reset(v), the identity row, just_received =
     1; the START bucket, the queue, invalid and whatever is in flight stay;
     the fleet's p and adj become the new formation's;
  2. the swarm's auto-auction countdown; when it fires, every vehicle's own
     autoauctionCb (coordination_ros.cpp:322-359): FLUSH for a vehicle whose
     last auction converged on an invalid table, START from the current q for
     every other (a restart when its auctioneer is open);
  3. ticks_per_step ticks of the Fleet;
  4. the hand-off (newAssignmentCb, :284-303): an adopting vehicle starts its
     controller; vehicle 0's adoption is the supervisor's assignment message
     (supervisor.py:110-113,147-150); every vehicle flies its own row;
  5. episode_oracle.control_step(..., tables=rows), TrialSwarm.traj, and
     every sample_every steps TrialSwarm.samples and Supervisor.tick.
"""
import numpy as np

import episode_oracle as E
import fleet_auction_cases as C
import fleet_auction_oracle as FO
import trial_oracle as T

BAD_INPUT = 0x4


class FleetTrial:
    """One swarm. forms: list of (p [n][3], adj [n][n], gains [3n][3n]) indexed
    by fseq [K]; q, vel [n][3]; tp: a dict as trial_oracle.default_params()
    (ep.auction_latency and ep.assignment 0)."""

    def __init__(self, fseq, forms, q, vel, tp, queue_cap=None, max_iter=0, ticks_per_step=10,
                 g=None, s=None):
        assert ticks_per_step >= 1
        assert tp["ep"].get("auction_latency", 0) == 0 and tp["ep"].get("assignment", 0) == 0
        self.q = np.array(q, np.float64)
        self.vel = np.array(vel, np.float64)
        self.n = n = len(self.q)
        self.forms, self.tp, self.T, self.g, self.s = forms, tp, int(ticks_per_step), g, s
        self.fbad = any(f < 0 or f >= len(forms) for f in fseq)
        self.t = T.TrialSwarm(n, fseq, forms, tp)  # the supervisor, ctl_on, the countdown, traj
        if self.fbad:
            self.t.fidx = 0
        p, adj, _ = forms[self.t.fidx]
        fl = self.fleet = FO.Fleet(p, adj, queue_cap=queue_cap, max_iter=max_iter)
        # acl_fleet_trial_init: freshly constructed auctioneers, every output 0
        fl.just_received[:] = 0
        fl.final_who[:] = 0
        fl.done_tick[:] = 0
        self.step_no = 0
        self.vflags = np.zeros(n, np.int32)  # sticky
        self.adopt_step = np.full(n, -1, np.int32)
        self.per_vehicle = 0
        self.P = self.points()
        self.n_auctions = 0
        self.fst = dict(flags=0, ticks_run=0, n_started=0, n_restarted=0, n_flushed=0,
                        n_consensus=0, n_adopted=0, n_invalid=0)

    @property
    def sup(self):
        return self.t.sup

    def points(self):
        """Each vehicle's point in its own row."""
        Pt = self.fleet.Pt
        return np.array([int(np.nonzero(Pt[v] == v)[0][0]) for v in range(self.n)], np.uint16)

    def auto_cmd(self):
        return np.where(self.fleet.invalid != 0, FO.FLUSH, FO.START).astype(np.uint8)

    def commit(self):
        """Step (1)."""
        t, fl, n = self.t, self.fleet, self.n
        t.fidx = t.fseq[t.sup.formation]
        t.ctl_on[:] = False
        t.zs = True
        t.sup.commit = False
        for v in range(n):
            fl._reset(v)
            fl.Pt[v] = np.arange(n)
            fl.just_received[v] = 1
        p, adj, _ = self.forms[t.fidx]
        fl.p, fl.adj = np.asarray(p, np.float64), np.asarray(adj)

    def pre(self):
        """Steps (1) and (2); returns the commands (None: the countdown did not
        fire) and whether the fleet kernel sees the swarm."""
        t = self.t
        t.zs = False
        if self.fbad and not t.done:
            t.sup.last_state, t.sup.state = t.sup.state, T.TERMINATE
            t.sup.done_step = self.step_no
        if t.done:
            return None, False
        now = False
        if t.sup.commit:
            self.commit()
            t.next_auction = self.tp["settle_steps"]
            now = t.next_auction <= 0
            if now:
                t.next_auction = self.tp["ep"]["auction_every"]
        elif t.next_auction > 0:
            t.next_auction -= 1
            if t.next_auction == 0:
                now = True
                t.next_auction = self.tp["ep"]["auction_every"]
        if not now:
            return None, True
        cmd = self.auto_cmd()
        start = cmd == FO.START
        self.fst["n_started"] += int(start.sum())
        self.fst["n_restarted"] += int((start & (self.fleet.open != 0)).sum())
        self.fst["n_flushed"] += int((cmd == FO.FLUSH).sum())
        self.n_auctions += 1
        return cmd, True

    def step(self, Rt=None, sup=None):
        """One control step. Rt [n][6]: the alignments handed to an
        auto-auction's START commands (default: the CPU oracle's under the
        vehicles' rows). sup: (u [n][3], ca [n], q [n][3]) the supervisor's
        samples and positions instead of the step's own (the GPU tests hand
        over the recorded ones). Returns the step's record."""
        t, fl, n, s = self.t, self.fleet, self.n, self.step_no
        snap = dict(open=fl.open.copy(), queued=fl.queue_len(),
                    inflight=[len(x) for x in fl.inflight])  # as the step begins
        committed = bool(t.sup.commit) and not t.done and not self.fbad
        cmd, live = self.pre()
        raised = np.zeros(n, np.int32)
        if not live:
            st = dict(ticks_run=0, n_open=0, n_queued=0, flags=BAD_INPUT)
            u = np.zeros((n, 3))
            us = np.zeros((n, 3))
            ca = np.zeros(n, np.uint8)
        else:
            if cmd is not None and Rt is None:
                p, adj, _ = self.forms[t.fidx]
                Rt = C.align_rt(p, adj, self.q, fl.Pt)
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
            t.ctl_on[adopted] = True  # first_assignment_
            if adopted[0]:
                t.sup.assignment_msg()
            # (the rows change by commit and adoption only, so this is the
            # device's hand-off, rebuilt at those and at the first step of a call)
            self.per_vehicle = int(not (fl.Pt == fl.Pt[0]).all())
            self.P = self.points()
            p, adj, G = self.forms[t.fidx]
            u, us, ca = E.control_step(self.q, self.vel, p, adj, G, self.P, self.g, self.s,
                                       tables=fl.Pt.astype(np.uint16))
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
                    n_thrown=fl.n_thrown.copy(), invalid=fl.invalid.copy(), open=fl.open.copy())


def run_trial(ft, steps):
    """Flies the restatement until the trial ends or `steps` steps; returns the
    per-step records."""
    recs = []
    for _ in range(steps):
        recs.append(ft.step())
        if ft.t.done:
            break
    return recs
