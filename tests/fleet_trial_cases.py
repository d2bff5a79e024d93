"""Cases of the trials on the message-level auction (acl_fleet_trial_batch),
shared by the CPU tests of the restatement (tests/test_fleet_trial.py) and the
GPU parity tests (tests/test_gpu_fleet_trial.py). Built on tests/trial_cases.py
(complete graphs, closed-form gains) and tests/fleet_auction_cases.py (chord
rings and the two disjoint rings, helpers.synth_gains: parity of the
arithmetic needs no designed gains). A case is one swarm; timings are
trial_cases.FAST / FAST_EP unless the case says otherwise.

What each case is for:
  sync6_two, sync6_reassign  ticks_per_step = 60, one clean auction of six
                   vehicles on the complete graph: the trial must equal
                   trial_oracle.run_trial's bit for bit
  interrupt6, interrupt13   the second formation commits while auctioneers are
                   open and bids are queued; the old auction's bids are thrown
                   away in the new formation's first auction
  restart13        an auction (312 ticks) longer than the auto-auction period
                   (200 ticks): every auto-auction restarts it, nobody adopts,
                   the supervisor's assignment timeout ends the trial
  stagger13_t2     two ticks per step: the controllers start over several
                   steps and the supervisor waits for vehicle 0's
  rings12_invalid  two disjoint rings: every auction ends INVALID, the next
                   auto-auction flushes, no controller ever starts
  ring65           the second wave of every kernel with one live lane
  near128          both task slots of every lane; max_iter = 40 is below the
                   graph's diameter, so only the vehicles near the chords end
                   on a whole table and adopt; the others flag INVALID
  interrupt128     near128 and a commit forced after three steps, onto open
                   auctioneers with queued bids and bids in flight
"""
import functools

import numpy as np

import fleet_auction_cases as FA
import fleet_auction_oracle as FO
import fleet_trial_oracle as FT
import helpers as H
import trial_cases as TC
import trial_oracle as T


class Case:
    """forms: [(p, adj, gains)]; fseq [K]; tp / ep: overrides of the default
    trial and episode parameters (over FAST / FAST_EP)."""

    def __init__(self, name, forms, fseq, q, steps, ticks_per_step, max_iter=0, tp=None, ep=None):
        self.name, self.forms, self.fseq = name, forms, np.asarray(fseq, np.int32)
        self.q = np.array(q, np.float64)
        self.vel = np.zeros_like(self.q)
        self.n = len(self.q)
        self.steps, self.T, self.max_iter = steps, ticks_per_step, max_iter
        self.tp_over = dict(TC.FAST, **(tp or {}))
        self.ep_over = dict(TC.FAST_EP, **(ep or {}))

    @property
    def tp(self):
        """The parameters as the restatements take them."""
        tp = T.default_params()
        tp.update(self.tp_over)
        tp["ep"] = dict(tp["ep"], **self.ep_over)
        return tp

    def oracle(self, q=None, vel=None):
        return FT.FleetTrial(self.fseq, self.forms, self.q if q is None else q,
                             self.vel if vel is None else vel, self.tp, max_iter=self.max_iter,
                             ticks_per_step=self.T)


def _from_trial(name, c, steps, ticks_per_step, **ep):
    """A tests/trial_cases.py case (complete graph, closed-form gains)."""
    return Case(name, list(zip(c["pts"], c["adj"], c["gains"])), c["fseq"], c["q"], steps,
                ticks_per_step, tp=c["tp"], ep=ep)


def sync6_two():
    return _from_trial("sync6_two", TC.two_formations(6), 230, 60)


def sync6_reassign():
    return _from_trial("sync6_reassign", TC.reassign(6), 230, 60)


def interrupt6():
    return _from_trial("interrupt6", TC.two_formations(6), 320, 2, auction_every=31)


def interrupt13():
    return _from_trial("interrupt13", TC.reassign(13), 380, 10, auction_every=33)


def restart13():
    return _from_trial("restart13", TC.reassign(13), 240, 10, auction_every=20)


def _ring_form(sc, seed=7):
    return (sc.p, sc.adj, H.synth_gains(np.random.RandomState(seed), sc.adj))


def stagger13_t2():
    sc = FA.clean_ring(13)
    return Case("stagger13_t2", [_ring_form(sc)], [0], sc.windows[0][1], 80, 2,
                ep=dict(auction_every=45))


def rings12_invalid():
    sc = FA.rings12()
    return Case("rings12_invalid", [_ring_form(sc)], [0], sc.windows[0][1], 240, 10,
                ep=dict(auction_every=12))


QUICK = dict(hover_wait=0.02, settle_steps=1)  # the first formation commits at step 3
DEFAULT_EVERY = dict(auction_every=120)  # acl_default_episode_params: an auction fits the period


def ring65():
    sc = FA.clean_ring(65)
    return Case("ring65", [_ring_form(sc)], [0], sc.windows[0][1], 60, 10, tp=QUICK,
                ep=DEFAULT_EVERY)


def _near128_forms():
    p, rng = TC.formation_points(128)
    adj = FA.chord_ring(128)
    G = H.synth_gains(np.random.RandomState(7), adj)
    q = p + TC.START_OFFSET
    q[:, :2] += rng.normal(0, 0.05, (128, 2))
    # vehicles 2 and 4 start at each other's points: the tables the auction
    # ends on are not the identity, so adopters and the others fly different rows
    q[[2, 4]] = q[[4, 2]]
    return p, adj, G, q


def near128():
    p, adj, G, q = _near128_forms()
    return Case("near128", [(p, adj, G)], [0], q, 22, 10, max_iter=40, tp=QUICK,
                ep=DEFAULT_EVERY)


# the commit is forced after three steps of near128's first auction (steps 4 to 6)
INTERRUPT128_AT = 4 + 3


def interrupt128():
    p, adj, G, q = _near128_forms()
    p2 = TC._scaled(p, 1.04)
    return Case("interrupt128", [(p, adj, G), (p2, adj, G)], [0, 1], q, INTERRUPT128_AT + 3, 10,
                max_iter=40, tp=QUICK, ep=DEFAULT_EVERY)


def force_commit(ft):
    """interrupt128's teacher forcing: the operator's second formation arrives
    now, whatever the supervisor's state."""
    ft.sup.commit = True
    ft.sup.formation = 1


CASES = {f.__name__: f for f in (sync6_two, sync6_reassign, interrupt6, interrupt13, restart13,
                                 stagger13_t2, rings12_invalid, ring65, near128, interrupt128)}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def cpu_run(name):
    """A case flown once on the restatement alone (the CPU oracle's
    alignments) until the trial ends or the case's steps are up, shared by the
    tests, which leave it unchanged. Returns (case, restatement, [per-step
    record])."""
    cs = case(name)
    ft = cs.oracle()
    recs = []
    for s in range(cs.steps):
        if name == "interrupt128" and s == INTERRUPT128_AT:
            force_commit(ft)
        recs.append(ft.step())
        if ft.t.done:
            break
    return cs, ft, recs


def adoption_steps(recs):
    """Steps at which some vehicle adopted -> the vehicles that did."""
    return {r["step"]: np.nonzero(r["raised"] & FO.V_ADOPTED)[0].tolist() for r in recs
            if (r["raised"] & FO.V_ADOPTED).any()}
