"""Plain-Python restatement of acl_fleet_lossy_episode_batch
(include/aclswarm_amd.h): fleet_delay_episode_oracle.DelayFleetEpisode with the
swarm's auctioneers a fleet_loss_oracle.LossyFleet. Nothing else differs: the
fleet's loss matrix, seed and n_lost live across steps (fleet.loss and
fleet.seed may be replaced between steps).

TEST INFRASTRUCTURE ONLY: imported by tests/, never by the product package.
"""
import fleet_delay_episode_oracle as DE
import fleet_loss_oracle as LO


class LossyFleetEpisode(DE.DelayFleetEpisode):
    """One swarm. loss: an int (every link) or [n][n] (receiver-major); seed:
    the swarm's u32; the other arguments are DelayFleetEpisode's."""

    def __init__(self, p, adj, gains, q, vel, ep, lat, loss=0, seed=0, Pt=None, queue_cap=None,
                 max_iter=0, ticks_per_step=10, g=None, s=None):
        super().__init__(p, adj, gains, q, vel, ep, lat, Pt=Pt, queue_cap=queue_cap,
                         max_iter=max_iter, ticks_per_step=ticks_per_step, g=g, s=s)
        self.fleet = LO.LossyFleet(self.p, self.adj, lat, loss=loss, seed=seed, Pt=Pt,
                                   queue_cap=queue_cap, max_iter=max_iter)
        self.P = self.points()

    def step(self, Rt=None, sup=None):
        """DelayFleetEpisode.step; the record also counts the step's lost bids."""
        before = int(self.fleet.n_lost.sum())
        r = super().step(Rt=Rt, sup=sup)
        r["lost"] = int(self.fleet.n_lost.sum()) - before
        return r
