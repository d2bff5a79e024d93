"""Cases of fleet localization on real links (acl_fleet_delay_localize_batch),
shared by the CPU tests (tests/test_fleet_delay_localize.py) and the GPU parity
tests (tests/test_gpu_fleet_delay_localize.py,
tests/test_gpu_fleet_delay_est_episode.py).

Every figure quoted below is what the restatement
(tests/fleet_delay_localize_oracle.py) ran; the CPU tests assert each.

  chord_ring(13) (diameter 6), identity rows, lossless, every link at d rounds:
      d = 0, 1, 2, 3: everybody known after 6, 12, 18, 24 rounds and max_age
      5, 11, 17, 23 from then on (a vehicle k hops away is known after
      k (d + 1) rounds and is k (d + 1) - 1 rounds old): KNOWN_AFTER_AT
  the mixed batch (mixed13): B = 8 on chord_ring(13), a latency matrix drawn
      per swarm in 0..3 (swarm 7: every link at 7, max_tlat 7 for the batch),
      fleet_localize_cases.loss_matrices13(), feed thresholds drawn from
      {0, 8192, 0xFFFF}, 24 rounds
"""
import numpy as np

import fleet_auction_cases as C
import fleet_delay_localize_oracle as DG
import fleet_localize_cases as GC

# d: (rounds until everybody is known, max_age from then on), chord_ring(13)
KNOWN_AFTER_AT = {0: (6, 5), 1: (12, 11), 2: (18, 17), 3: (24, 23)}

FEED_THRS = (0, 8192, 0xFFFF)


def tlat_draw(n, seed, hi):
    """[n][n] latencies drawn uniformly in 0..hi; the diagonal is drawn too
    (and ignored by the model)."""
    return np.random.RandomState(seed).randint(0, hi + 1, (n, n))


def feed_draw(n, seed, thrs=FEED_THRS):
    return np.array(thrs)[np.random.RandomState(seed).randint(0, len(thrs), n)]


MIXED_B, MIXED_ROUNDS, MIXED_MAX_TLAT = 8, 24, 7


def mixed13():
    """(adj, tlat [B], loss [B], seeds [B], feed [B]) of the mixed batch."""
    ms, seeds = GC.loss_matrices13()
    tl = [tlat_draw(13, 300 + b, 3) for b in range(MIXED_B)]
    tl[7][:] = 7
    fd = [feed_draw(13, 400 + b) for b in range(MIXED_B)]
    fd[0][:] = 0
    return C.chord_ring(13), tl, ms, seeds, fd


def mixed_trackers():
    adj, tl, ms, seeds, fd = mixed13()
    return [DG.DelayedTrackers(adj, loss=ms[b], seed=seeds[b], tlat=tl[b],
                               max_tlat=MIXED_MAX_TLAT, feed_loss=fd[b]) for b in range(MIXED_B)]
