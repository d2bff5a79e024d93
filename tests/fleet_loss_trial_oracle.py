"""Plain-Python restatement of acl_fleet_lossy_trial_batch
(include/aclswarm_amd.h): fleet_delay_trial_oracle.DelayFleetTrial with the
swarm's auctioneers a fleet_loss_oracle.LossyFleet. Only the vehicles' bids are
lossy: the formation changes and the supervisor's subscription to vehicle 0
are DelayFleetTrial's.

TEST INFRASTRUCTURE ONLY: imported by tests/, never by the product package.
"""
import fleet_delay_trial_oracle as DT
import fleet_loss_oracle as LO


class LossyFleetTrial(DT.DelayFleetTrial):
    """One swarm. loss: an int (every link) or [n][n] (receiver-major); seed:
    the swarm's u32; the other arguments are DelayFleetTrial's."""

    def __init__(self, fseq, forms, q, vel, tp, lat, loss=0, seed=0, queue_cap=None, max_iter=0,
                 ticks_per_step=10, g=None, s=None):
        super().__init__(fseq, forms, q, vel, tp, lat, queue_cap=queue_cap, max_iter=max_iter,
                         ticks_per_step=ticks_per_step, g=g, s=s)
        p, adj, _ = forms[self.t.fidx]
        fl = self.fleet = LO.LossyFleet(p, adj, lat, loss=loss, seed=seed, queue_cap=queue_cap,
                                        max_iter=max_iter)
        # acl_fleet_delay_trial_init: freshly constructed auctioneers, every output 0
        fl.just_received[:] = 0
        fl.final_who[:] = 0
        fl.done_tick[:] = 0
        self.P = self.points()

    def step(self, Rt=None, sup=None):
        """DelayFleetTrial.step; the record also counts the step's lost bids."""
        before = int(self.fleet.n_lost.sum())
        r = super().step(Rt=Rt, sup=sup)
        r["lost"] = int(self.fleet.n_lost.sum()) - before
        return r
