"""Plain-Python restatement of acl_fleet_delay_est_episode_batch
(include/aclswarm_amd.h): fleet_est_episode_oracle.EstFleetEpisode whose
VehicleTrackers are fleet_delay_localize_oracle.DelayedTrackers -- the gossip
round of stage 0 takes tables whole rounds late, and a vehicle's own feed may
be out. gossip() hands them the fleet's rows, loss and seed of the moment, as
before. Nothing else differs.

TEST INFRASTRUCTURE ONLY: imported by tests/, never by the product package.
"""
import fleet_delay_localize_oracle as DG
import fleet_est_episode_oracle as XO


class DelayEstFleetEpisode(XO.EstFleetEpisode):
    """One swarm. tlat: an int or [n][n]; max_tlat; feed_loss: an int or [n];
    the other arguments are EstFleetEpisode's."""

    def __init__(self, *args, tlat=0, max_tlat=None, feed_loss=0, **kw):
        super().__init__(*args, **kw)
        self.trackers = DG.DelayedTrackers(self.adj, Pt=self.fleet.Pt, loss=self.fleet.loss,
                                           seed=self.fleet.seed, tlat=tlat, max_tlat=max_tlat,
                                           feed_loss=feed_loss)
