"""Trials above one wave (acl_trial_batch at n = 65, 129, 257), shared by the
CPU tests of the restatement (tests/test_trial.py) and the GPU parity tests
(tests/test_gpu_trial.py). Plain numpy: complete graphs and closed-form gains,
so a case is built without an ADMM run and without a GPU.

A case is one swarm: its own formations (pts / adj / gains lists), a start
(q, vel [n][3]), a formation sequence fseq [K] into its own lists, and the
trial parameters it needs beyond FAST (tp). `batch` puts cases side by side
in one formation table, as one Trial flies them.

What each case is for (csrc/trial.hip runs vehicles over 128-thread blocks,
the commit over 64 threads, the adoption over 256):
  calm            nothing happens that the last lane decides: the yardstick
  late_last       vehicle n - 1 alone keeps has_converged false for at least
                  one window: the last live lane of the last wave or pass
                  vetoes the all()
  pair_last       formation points n - 2 and n - 1 are 0.3 m apart: those two
                  vehicles alone hold collision avoidance, so the last two
                  lanes decide has_gridlocked's any()
  reassign        a second formation rotated under the swarm: auctions change
                  vehicle 0's table, its assignment message is counted
                  (changed0, n_assign)
  two_formations  a second formation that keeps the assignment: a whole
                  two-formation record
"""
import numpy as np

import helpers as H

# short supervisor timings so that the CPU restatement stays fast: the state
# machine is the reference's, the clocks are scaled down
FAST = dict(settle_steps=10, hover_wait=0.2, formation_received_wait=0.1, converged_wait=0.2,
            gridlock_timeout=2.0, trial_timeout=60.0, assignment_timeout=2.0)
FAST_EP = dict(auction_every=20, bufflen=10)

START_OFFSET = np.array([3.0, -2.0, 0.0])


def closed_form_gains(p):
    """A gain matrix [3n][3n] for the complete graph whose kernel holds the
    formation p [n][3]: with z = p_x + i p_y, Q an orthonormal basis of
    span{1, z} and Qz one of span{1, p_z},
        A = -(I - Q Q^H)  (complex, n x n),  C = -(I - Qz Qz^T),
    block (i, j) = [[Re A_ij, -Im A_ij, 0], [Im A_ij, Re A_ij, 0], [0, 0, C_ij]]
    for all i, j. The reference's block structure [a b 0; -b a 0; 0 0 c], zero
    row sums (1 is in both kernels), negative semidefinite: the swarm flies
    into a translated, rotated and scaled copy of p."""
    p = np.asarray(p, np.float64)
    n = p.shape[0]
    z = p[:, 0] + 1j * p[:, 1]
    Q, _ = np.linalg.qr(np.c_[np.ones(n), z])
    A = -(np.eye(n) - Q @ Q.conj().T)
    Qz, _ = np.linalg.qr(np.c_[np.ones(n), p[:, 2]])
    C = -(np.eye(n) - Qz @ Qz.T)
    G = np.zeros((n, 3, n, 3))
    G[:, 0, :, 0] = A.real
    G[:, 0, :, 1] = -A.imag
    G[:, 1, :, 0] = A.imag
    G[:, 1, :, 1] = A.real
    G[:, 2, :, 2] = C
    return G.reshape(3 * n, 3 * n)


def complete(n):
    return (np.ones((n, n)) - np.eye(n)).astype(np.uint8)


def formation_points(n, seed=0):
    """n points at least 2.5 m apart in a square of side 28 sqrt(n / 20),
    altitudes U(0.5, 3)."""
    rng = np.random.RandomState(1000 * n + seed)
    p = H.random_positions(rng, n, 28.0 * np.sqrt(n / 20.0), r=1.25)
    p[:, 2] = rng.uniform(0.5, 3.0, n)
    return p, rng


def start(p, rng):
    """Uncrossed: every vehicle next to its own point of the shifted
    formation, so CBAA keeps the identity."""
    q = p + START_OFFSET
    q[:, :2] += rng.normal(0, 0.1, (len(p), 2))
    q[:, 2] = 1.0
    return q


def _case(name, pts, q, fseq, **tp):
    n = q.shape[0]
    return dict(name=name, pts=list(pts), adj=[complete(n) for _ in pts],
                gains=[closed_form_gains(p) for p in pts], q=q, vel=np.zeros_like(q),
                fseq=np.asarray(fseq, np.int32), tp=tp)


def calm(n, seed=0):
    p, rng = formation_points(n, seed)
    return _case("calm", [p], start(p, rng), [0])


# the smallest multiple of 0.25 m that keeps IN_FORMATION back by a whole
# window (2 * bufflen steps) at n = 65 and at n = 129 on the CPU restatement
# (0.25 m: 10 steps at n = 65, none at n = 129; 0.5 m: 38 and 44 steps)
LATE_LAST_M = 0.5


def late_last(n, d=LATE_LAST_M):
    """calm with vehicle n - 1 started d metres further out, along its own
    formation point's direction from the formation's centroid."""
    p, rng = formation_points(n)
    q = start(p, rng)
    r = p[n - 1, :2] - p[:, :2].mean(axis=0)
    q[n - 1, :2] += d * r / np.hypot(*r)
    return _case("late_last", [p], q, [0])


PAIR_GRIDLOCK_TIMEOUT = 0.4


def pair_last(n):
    """calm with formation point n - 1 put 0.3 m in x from point n - 2 at the
    same altitude, and vehicle n - 1 started a further 1.1 m out in x: the
    two close on each other, nobody else is near."""
    p, rng = formation_points(n)
    p[n - 1] = p[n - 2] + np.array([0.3, 0.0, 0.0])
    q = start(p, rng)
    q[n - 1, 0] += 1.1
    return _case("pair_last", [p], q, [0], gridlock_timeout=PAIR_GRIDLOCK_TIMEOUT)


def _scaled(p, s, deg=0.0):
    c, sn = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    out = p.copy()
    out[:, :2] = s * p[:, :2] @ np.array([[c, sn], [-sn, c]])
    return out


def reassign(n):
    """Two formations, the second the first scaled by 1.1 and turned by 10
    degrees in xy: the gains fly a similar copy wherever it forms, so after
    the first formation the swarm is turned against the second and auctions
    change the assignment."""
    p, rng = formation_points(n)
    return _case("reassign", [p, _scaled(p, 1.1, 10.0)], start(p, rng), [0, 1])


def two_formations(n):
    """Two formations, the second the first scaled by 1.04: the assignment
    stays, both formations converge."""
    p, rng = formation_points(n)
    return _case("two_formations", [p, _scaled(p, 1.04)], start(p, rng), [0, 1])


def batch(cases, **ep):
    """The cases as the swarms of one Trial: one formation table, fseq [B][K]
    with K the longest sequence (a shorter one flies its last formation
    again: the commit, the auction and the convergence once more from inside
    the formation), the cases' own trial parameters merged over FAST (they
    must not contradict each other)."""
    K = max(len(c["fseq"]) for c in cases)
    pts, adj, gains, fseq, tp = [], [], [], [], dict(FAST)
    own = {}
    for c in cases:
        f = list(len(pts) + c["fseq"]) + [len(pts) + c["fseq"][-1]] * (K - len(c["fseq"]))
        fseq.append(f)
        pts += c["pts"]; adj += c["adj"]; gains += c["gains"]
        for k, v in c["tp"].items():
            assert own.setdefault(k, v) == v, k
    tp.update(own)
    return dict(names=[c["name"] for c in cases], pts=pts, adj=adj, gains=gains,
                q=np.stack([c["q"] for c in cases]), vel=np.stack([c["vel"] for c in cases]),
                fseq=np.asarray(fseq, np.int32), tp=tp, ep=dict(FAST_EP, **ep))


def oracle_params(case):
    """The batch's parameters as oracle/trial_oracle.py takes them."""
    import trial_oracle as T
    tp = T.default_params()
    tp.update(case["tp"])
    tp["ep"] = dict(tp["ep"], **case["ep"])
    return tp


def first_step(states, s):
    """The first step whose state is s (-1: none); states [steps]."""
    w = np.nonzero(np.asarray(states) == s)[0]
    return int(w[0]) if len(w) else -1
