"""Cases of the fleet auction, episodes and trials with seeded per-link message
loss (acl_fleet_lossy_auction_batch / _episode_batch / _trial_batch), shared by
the CPU tests (tests/test_fleet_loss*.py) and the GPU parity tests
(tests/test_gpu_fleet_loss*.py): a latency case of tests/fleet_delay_cases.py
(or of the delay episode / trial cases), a loss matrix and a seed.

Every figure quoted below is what the restatements (tests/fleet_loss_oracle.py
and its episode / trial subclasses) ran; the CPU tests assert each. A parity
batch must hold a swarm that finishes with nothing lost, one that lost a bid
and one that ends with open vehicles (batch_condition), so that no GPU parity
case can pass by never losing a bid.

  swarm6 / ring13 under their DRAW_SEED latencies, loss 64, seeds 0..7
      lost [0,0,0,1,0,1,1,1], n_open [0,0,0,6,0,6,6,6]          (swarm6)
      lost [0,1,1,1,0,0,1,0], n_open [0,13,1,13,0,0,13,0]       (ring13;
      seed 2 loses a bid of the last iterations: one vehicle stays open)
  ring13, loss 64, seed 1   one bid lost (receiver 8, sender 9, publication
      tick 29, iter 7, due at tick 30): all 13 open and quiescent after 54 ticks
  ring13, loss 1024, seed 3  3 bids lost, stalled after 18 ticks
  ring_case(n, 0), loss 16, seeds 0..3: RING_FIGURES (ticks_run, n_open, lost)
  episode ring13/draw2, loss 64, seed 1   a bid lost in step 3; nobody adopts
      at step 11; the auto-auction of step 12 restarts 13 open auctioneers;
      all adopt at step 23
  trial chord13_t10, loss 64, seed 1   a bid lost in step 34; nobody adopts at
      step 42; the auto-auction of step 54 restarts 13 open auctioneers; all
      adopt at step 75
  trial chord13_timeout (the same ring, 300 steps at most), loss 1024, seed 0
      every one of the 6 auctions loses a bid; TERMINATE through the
      assignment timeout at step 224, 65 restarts, no adoption
"""
import functools

import numpy as np

import fleet_auction_cases as C
import fleet_delay_cases as DC
import fleet_delay_episode_cases as DEC
import fleet_delay_trial_cases as DTC
import fleet_loss_episode_oracle as LE
import fleet_loss_oracle as LO
import fleet_loss_trial_oracle as LT

DEAD = LO.DEAD


class LossCase:
    """A fleet_delay_cases.DelayCase with a loss matrix ([n][n] or an int) and
    the swarm's seed; it has the DelayCase interface, so
    fleet_delay_cases.run_oracle runs it."""

    def __init__(self, case, loss, seed):
        self.case, self.sc, self.n = case, case.sc, case.n
        self.name = f"{case.name}/loss/seed{seed}"
        self.lat, self.max_lat, self.budget = case.lat, case.max_lat, case.budget
        self.wticks, self.queue_cap, self.max_iter = case.wticks, case.queue_cap, case.max_iter
        self.loss = LO.loss_matrix(self.n, loss)
        self.seed = int(seed)

    def ticks(self, k):
        return self.case.ticks(k)

    def fleet(self, queue_cap=None):
        return LO.LossyFleet(self.sc.p, self.sc.adj, self.lat, loss=self.loss, seed=self.seed,
                             Pt=self.sc.Pt,
                             queue_cap=self.queue_cap if queue_cap is None else queue_cap,
                             max_iter=self.max_iter)


def batch(cases, loss, seeds=0):
    """Swarm b: cases[b] (or the one case B = 8 times) under loss (an int, one
    matrix, or one per swarm) and seed seeds[b]; an int seeds: seeds + b, as
    the engine seeds a batch."""
    if not isinstance(cases, (list, tuple)):
        cases = [cases] * 8
    per = isinstance(loss, (list, tuple))
    if not isinstance(seeds, (list, tuple)):
        seeds = [seeds + b for b in range(len(cases))]
    return [LossCase(c, loss[b] if per else loss, seeds[b]) for b, c in enumerate(cases)]


def figures(fl, recs):
    """(ticks_run of the last window that ran, n_open, bids lost)."""
    ran = [r["status"]["ticks_run"] for r in recs if r["status"]["ticks_run"]]
    return (ran[-1] if ran else 0, int(fl.open.sum()), int(fl.n_lost.sum()))


def batch_condition(runs):
    """runs: [(fleet, records)] of a parity batch."""
    figs = [figures(fl, recs) for fl, recs in runs]
    clean = any(lost == 0 and n_open == 0 for _, n_open, lost in figs)
    return clean and any(lost > 0 for _, _, lost in figs) and any(o > 0 for _, o, _ in figs)


# ---- the committed batches ----
ITEM5_LOSS = 64
ITEM5_LOST = {"swarm6": [0, 0, 0, 1, 0, 1, 1, 1], "ring13": [0, 1, 1, 1, 0, 0, 1, 0]}
ITEM5_OPEN = {"swarm6": [0, 0, 0, 6, 0, 6, 6, 6], "ring13": [0, 13, 1, 13, 0, 0, 13, 0]}
ITEM5_TICKS = {"swarm6": [57, 57, 57, 57, 57, 28, 29, 28],
               "ring13": [119, 54, 119, 79, 119, 119, 30, 119]}


def item5(name):
    return batch(DC.draw(name), ITEM5_LOSS)


RING_LOSS = 16
RING_FIGURES = {64: [(145, 0, 0), (130, 56, 1), (136, 46, 1), (145, 3, 1)],
                65: [(129, 0, 0), (129, 51, 1), (129, 0, 0), (129, 0, 0)],
                128: [(66, 0, 0), (66, 0, 0), (66, 0, 0), (66, 11, 1)]}


def rings(n):
    return batch([DC.ring_case(n, 0)] * 4, RING_LOSS)


def loss_draw(n, seed, density=0.06):
    """[n][n] (receiver-major): 0 on most links, and on a drawn `density` of
    them one of 256, 4096 and 0xFFFF."""
    rng = np.random.RandomState(seed)
    m = rng.choice([256, 4096, DEAD], size=(n, n))
    return np.where(rng.random_sample((n, n)) < density, m, 0)


MATRIX_SEED = 700


def matrices13():
    """B = 8 at n = 13, a drawn matrix per swarm: four latency draws of the
    clean ring, both asymmetric-row fleets and the four-window stale sequence
    (restarts onto stalled auctions) twice."""
    cases = [DC.draw("ring13", s) for s in (2,) + DC.CLEAN_SEEDS] + [
        DC.draw("rows13"), DC.rows13_stall_finishes(), DC.draw("stale13"), DC.draw("stale13", 33)]
    return batch(cases, [loss_draw(13, MATRIX_SEED + b) for b in range(8)])


# (ticks_run of the last window that ran, n_open, lost) per swarm
MATRIX_FIGURES = [(30, 13, 2), (131, 0, 0), (25, 13, 1), (25, 13, 2), (23, 13, 3), (20, 13, 4),
                  (121, 0, 1), (131, 0, 1)]

WRAP_LOSS = 256
WRAP_SEEDS = [10, 34, 28, 75, 0, 2]
WRAP_FIGURES = [(78, 0, 0), (78, 4, 1), (70, 13, 2), (78, 5, 1), (16, 13, 1), (34, 13, 4)]


def wrap13():
    """The log-ring wrap cases (max_lat = 2: a ring of 4 entries, reused every
    other tick) under loss 256: the clean ring under four seeds (nothing
    lost; bids lost late, at tick 70 and after), rows13 and the stale sequence."""
    return batch([DC.wrap()] * 4 + [DC.wrap("rows13", 22), DC.wrap("stale13", 23)], WRAP_LOSS,
                 WRAP_SEEDS)


DEAD_W = 2  # the dead link of swarm6: into receiver 2 from its first subscribed sender (0)


def dead_link():
    """swarm6 under its draw with one subscribed link dead."""
    case = DC.draw("swarm6")
    u = min(case.fleet().subscribed(DEAD_W))
    loss = np.zeros((6, 6), np.int64)
    loss[DEAD_W][u] = DEAD
    return LossCase(case, loss, 5), int(u)


def dead_into_3():
    """fleet_delay_cases.overflow6 (queue_cap 2) with every link into vehicle 3
    dead: what would have been appended or dropped there is lost instead."""
    loss = np.zeros((6, 6), np.int64)
    loss[3, :] = DEAD
    return LossCase(DC.overflow6(), loss, 9)


def publications(fl, u):
    """How many bids sender u has published: its START bid and one per tally
    that went on (the tally that ends in consensus publishes nothing)."""
    done = int((fl.vflags[u] & C.FO.V_CONSENSUS) != 0)
    return 1 + int(fl.n_tally[u]) - done


@functools.lru_cache(maxsize=None)
def cpu_batch(key, *args):
    """A batch run once on the restatement with the CPU oracle's alignments:
    [(fleet, records)], shared by the tests (which leave it alone)."""
    return [DC.run_oracle(lc) for lc in globals()[key](*args)]


# ---- episodes ----
EP_LOSS, EP_SEED = 64, 1


class LossyEpisodeCase:
    """A fleet_delay_episode_cases.DelayCase with loss (an int or [n][n]) and seed."""

    def __init__(self, cs, loss, seed):
        self.cs, self.loss, self.seed = cs, LO.loss_matrix(cs.n, loss), int(seed)
        self.name = f"{cs.name}/loss/seed{seed}"

    def __getattr__(self, k):
        return getattr(self.cs, k)

    def oracle(self, queue_cap=None):
        cs = self.cs
        ep = LE.LossyFleetEpisode(cs.p, cs.adj, cs.gains, cs.q0, cs.vel0, cs.ep, cs.lat,
                                  loss=self.loss, seed=self.seed, Pt=cs.Pt, queue_cap=queue_cap,
                                  max_iter=cs.max_iter, ticks_per_step=cs.T)
        for v in cs.invalid0:
            ep.fleet.invalid[v] = 1
        return ep


def episode(name, loss=EP_LOSS, seed=EP_SEED):
    return LossyEpisodeCase(DEC.case(name), loss, seed)


RING65_EP_LOSS, RING65_EP_SEED = 64, 1  # bids lost in steps 4, 7, 9, 13: 10 consensus, 55 open


def episode_ring65():
    return episode("ring65_draw", RING65_EP_LOSS, RING65_EP_SEED)


@functools.lru_cache(maxsize=None)
def cpu_episode(name, loss=EP_LOSS, seed=EP_SEED):
    cs = episode(name, loss, seed)
    ep, recs = DEC.fly(cs, cs.oracle())
    return cs, ep, recs


# ---- trials ----
TR_LOSS, TR_SEED = 64, 1
TIMEOUT_LOSS, TIMEOUT_SEED, TIMEOUT_STEPS = 1024, 0, 300


class LossyTrialCase:
    """A fleet_delay_trial_cases.DelayCase with loss (an int or [n][n]) and seed."""

    def __init__(self, cs, loss, seed):
        self.cs, self.loss, self.seed = cs, LO.loss_matrix(cs.n, loss), int(seed)
        self.name = f"{cs.name}/loss/seed{seed}"

    def __getattr__(self, k):
        return getattr(self.cs, k)

    def oracle(self):
        cs = self.cs
        return LT.LossyFleetTrial(cs.fseq, cs.forms, cs.q, cs.vel, cs.tp, cs.lat, loss=self.loss,
                                  seed=self.seed, max_iter=cs.max_iter, ticks_per_step=cs.T)


def chord13_timeout():
    """chord13_t10 with room for the assignment timeout to run out."""
    return DTC.DelayCase("chord13_timeout", DTC._chord13("chord13_timeout", TIMEOUT_STEPS, 10, 33),
                         DC.lat_draw(13, DTC.SEED_RING13, 1, 5))


def trial(name, loss=TR_LOSS, seed=TR_SEED):
    cs = chord13_timeout() if name == "chord13_timeout" else DTC.case(name)
    return LossyTrialCase(cs, loss, seed)


@functools.lru_cache(maxsize=None)
def cpu_trial(name, loss=TR_LOSS, seed=TR_SEED):
    cs = trial(name, loss, seed)
    ft, recs = DTC.fly(cs, cs.oracle())
    return cs, ft, recs
