"""Plain-Python restatement of acl_fleet_est_control_batch
(include/aclswarm_amd.h): one control step of one swarm in which every vehicle
steers on its own table of position estimates under its own row.

TEST INFRASTRUCTURE ONLY: imported by tests/, never by the product package.

Per vehicle v, with T = est[v] and row = Pt[v]:
  a row that is not a permutation: u = u_safe = 0, ca = 0, counted;
  otherwise pyoracle.control(v, T, vel[v], row, ...) -- DistCntrl::compute with
  q_veh := T -- then pyoracle.saturate and pyoracle.collision_avoidance(v, T,
  ...): an entry never heard of is whatever T holds, not special-cased.
"""
import math

import numpy as np

import episode_oracle as E
import pyoracle as O

BAD_INPUT, BAD_ROW = 0x4, 0x8


def control_step(est, vel, Pt, p, adj, gains, g=None, s=None):
    """est [n][n][3], vel [n][3], Pt [n][n] (row v: vehicle v's formation point
    -> vehicle). Returns u, u_safe [n][3], ca [n] u8 and the status record."""
    est = np.asarray(est, np.float64)
    n = est.shape[0]
    u = np.zeros((n, 3))
    us = np.zeros((n, 3))
    ca = np.zeros(n, np.uint8)
    n_bad = 0
    for v in range(n):
        row = np.asarray(Pt[v], np.int64)
        if not E.is_perm(row):
            n_bad += 1
            continue
        u[v] = O.control(v, est[v], vel[v], row.astype(np.uint16), adj, gains, p, g)
        c = O.saturate(u[v], s)
        us[v], mod = O.collision_avoidance(v, est[v], c, s)
        ca[v] = mod
    return u, us, ca, dict(n_ca=int(ca.sum()), n_bad_rows=n_bad, reserved=0,
                           flags=BAD_ROW if n_bad else 0)


def _wrap(a):  # utils.h:275-280
    if a > math.pi:
        return a - 2 * math.pi
    if a < -math.pi:
        return a + 2 * math.pi
    return a


def sectors(v, T, s=None):
    """collisionAvoidance's view of table T from vehicle v (safety.cpp:412-460):
    dict(dist: every |T[j] - T[v]|_xy, j != v; close: how many are within
    d_avoid_thresh (a NaN distance is: !(d > thresh)); nan: how many of those
    are NaN; wrapped: some sector crossed +-pi; zones: the united no-fly zones'
    edges as utils::closest sees them, the +-pi ones dropped when wrapped).
    A NaN sector is left out of the zones."""
    s = s or O.default_safety()
    T = np.asarray(T, np.float64)
    dist, edges = [], []
    close = nan = 0
    wrapped = False
    for j in range(T.shape[0]):
        if j == v:
            continue
        qx, qy = T[j, 0] - T[v, 0], T[j, 1] - T[v, 1]
        d = math.sqrt(qx * qx + qy * qy)
        if math.isnan(d):
            close += 1
            nan += 1
            continue
        dist.append(d)
        if d > s.d_avoid_thresh:
            continue
        close += 1
        theta = math.atan2(qy, qx)
        alpha = abs(math.asin(min(1.0, s.r_keep_out / d)))
        beg, end = _wrap(theta - alpha), _wrap(theta + alpha)
        edges += [(beg, +1), (end, -1)]
        if beg > end:
            wrapped = True
            edges += [(-math.pi, +1), (math.pi, -1)]
    edges.sort()
    zones, count, start = [], 0, 0.0
    for a, sg in edges:
        if count == 0:
            start = a
        count += sg
        if count == 0:
            zones += [start, a]
    if wrapped:
        zones = [a for a in zones if abs(a) != math.pi]
    return dict(dist=dist, close=close, nan=nan, wrapped=wrapped, zones=zones)


def decision_margins(v, T, cmd, s=None):
    """What a 1e-5 difference in the command, or a last-bit difference in a
    distance, could flip in collisionAvoidance for vehicle v on table T with the
    saturated command cmd. None when no vehicle is within d_avoid_thresh, else
      d_margin        min | dist_j - d_avoid_thresh | over all j != v
      edge_margin     min | psi - edge | over the no-fly zones' edges
      quarter_margin  min | |wrapToPi(edge - psi)| - pi/2 | over those edges
    (inf where there is no such edge). A NaN distance is close whatever its
    last bit, and its sector's edges are NaN: neither enters a minimum."""
    s = s or O.default_safety()
    sc = sectors(v, T, s)
    if sc["close"] == 0:
        return None
    psi = math.atan2(cmd[1], cmd[0])
    d_margin = min([abs(d - s.d_avoid_thresh) for d in sc["dist"]], default=math.inf)
    edge_margin = min([abs(psi - e) for e in sc["zones"]], default=math.inf)
    quarter = min([abs(abs(_wrap(e - psi)) - math.pi / 2) for e in sc["zones"]], default=math.inf)
    return d_margin, edge_margin, quarter
