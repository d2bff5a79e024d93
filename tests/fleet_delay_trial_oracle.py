"""Plain-Python restatement of acl_fleet_delay_trial_batch
(include/aclswarm_amd.h): fleet_trial_oracle.FleetTrial with the swarm's
auctioneers a fleet_delay_oracle.DelayFleet. The commit is FleetTrial's, which
on a DelayFleet is the model's: _reset(v), the identity row, just_received =
1; the publication log (whatever is in flight), the START bucket, the queue
and invalid stay, and a bid in flight is delivered when due to whoever
subscribes to its sender under the identity row.

TEST INFRASTRUCTURE ONLY: imported by tests/, never by the product package.
"""
import fleet_delay_oracle as DO
import fleet_trial_oracle as FT


class DelayFleetTrial(FT.FleetTrial):
    """One swarm. lat: an int (uniform) or [n][n] (receiver-major); the other
    arguments are FleetTrial's."""

    def __init__(self, fseq, forms, q, vel, tp, lat, queue_cap=None, max_iter=0,
                 ticks_per_step=10, g=None, s=None):
        super().__init__(fseq, forms, q, vel, tp, queue_cap=queue_cap, max_iter=max_iter,
                         ticks_per_step=ticks_per_step, g=g, s=s)
        p, adj, _ = forms[self.t.fidx]
        fl = self.fleet = DO.DelayFleet(p, adj, lat, queue_cap=queue_cap, max_iter=max_iter)
        # acl_fleet_delay_trial_init: freshly constructed auctioneers, every output 0
        fl.just_received[:] = 0
        fl.final_who[:] = 0
        fl.done_tick[:] = 0
        self.P = self.points()

    def in_flight(self):
        """Per sender: its publications that are still due somewhere."""
        return [len(x) for x in self.fleet.log]

    def step(self, Rt=None, sup=None):
        """FleetTrial.step; before["inflight"] counts the publication logs."""
        fly = self.in_flight()
        r = super().step(Rt=Rt, sup=sup)
        r["before"]["inflight"] = fly
        return r
