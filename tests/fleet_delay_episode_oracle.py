"""Plain-Python restatement of acl_fleet_delay_episode_batch
(include/aclswarm_amd.h): fleet_episode_oracle.FleetEpisode with the swarm's
auctioneers a fleet_delay_oracle.DelayFleet. Nothing else differs: the step's
ticks are the DelayFleet's, whose tick counter, publication logs and latency
matrix live across steps.

TEST INFRASTRUCTURE ONLY: imported by tests/, never by the product package.
"""
import fleet_delay_oracle as DO
import fleet_episode_oracle as FE


class DelayFleetEpisode(FE.FleetEpisode):
    """One swarm. lat: an int (uniform) or [n][n] (receiver-major); the other
    arguments are FleetEpisode's."""

    def __init__(self, p, adj, gains, q, vel, ep, lat, Pt=None, queue_cap=None, max_iter=0,
                 ticks_per_step=10, g=None, s=None):
        super().__init__(p, adj, gains, q, vel, ep, Pt=Pt, queue_cap=queue_cap, max_iter=max_iter,
                         ticks_per_step=ticks_per_step, g=g, s=s)
        self.fleet = DO.DelayFleet(self.p, self.adj, lat, Pt=Pt, queue_cap=queue_cap,
                                   max_iter=max_iter)
        self.P = self.points()

    def in_flight(self):
        """Per sender: its publications that are still due somewhere."""
        return [len(x) for x in self.fleet.log]

    def step(self, Rt=None, sup=None):
        """FleetEpisode.step; the record also says what the step found:
        before = (open [n], queued [n], in flight [n])."""
        fl = self.fleet
        snap = dict(open=fl.open.copy(), queued=fl.queue_len(), inflight=self.in_flight())
        r = super().step(Rt=Rt, sup=sup)
        r["before"] = snap
        return r
