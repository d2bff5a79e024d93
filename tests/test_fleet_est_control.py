"""CPU tests of the own-estimate control step (acl_fleet_est_control_batch):
the restatement tests/fleet_est_control_oracle.py against the shared-snapshot
control of oracle/episode_oracle.py, what stale and unknown estimates do to a
command, the input condition and the coverage of the GPU tests' cases
(tests/fleet_est_control_cases.py), and the ABI without a GPU."""
import ctypes as ct

import numpy as np

import episode_oracle as E
import fleet_auction_cases as C
import fleet_episode_cases as EC
import fleet_est_control_cases as K
import fleet_est_control_oracle as CO
import fleet_localize_oracle as GO
import pyoracle as O

TOL = 1e-5


def _rel(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1.0)


def test_shared_table_is_the_shared_snapshot_control():
    """est[v] = q for every v and one shared table: episode_oracle.control_step
    exactly."""
    for key in ((13, "dense", 5), (20, "packed", 9), (65, "spread", 5)):
        cs = K.case(*key)
        n = cs.n
        rng = np.random.RandomState(n)
        P = rng.permutation(n).astype(np.uint16)
        u0, us0, ca0 = E.control_step(cs.q, cs.vel, cs.p, cs.adj, cs.gains, P)
        est = np.broadcast_to(cs.q, (n, n, 3))
        Pt = np.tile(E.inverse(P), (n, 1))
        u, us, ca, st = CO.control_step(est, cs.vel, Pt, cs.p, cs.adj, cs.gains)
        assert np.array_equal(u, u0) and np.array_equal(us, us0) and np.array_equal(ca, ca0)
        assert st == dict(n_ca=int(ca0.sum()), n_bad_rows=0, reserved=0, flags=0)


def test_bad_row_rule():
    cs = K.case(13, "dense", 5)
    u, us, ca, st = cs.reference()
    (v,) = cs.bad
    assert not u[v].any() and not us[v].any() and ca[v] == 0
    assert st["n_bad_rows"] == 1 and st["flags"] == CO.BAD_ROW
    # the other vehicles are unaffected: the same commands with that row mended
    Pt = cs.Pt.copy()
    Pt[v] = np.arange(cs.n)
    u2, us2, ca2, st2 = CO.control_step(cs.est, cs.vel, Pt, cs.p, cs.adj, cs.gains)
    keep = np.arange(cs.n) != v
    assert np.array_equal(u[keep], u2[keep]) and np.array_equal(us[keep], us2[keep])
    assert np.array_equal(ca[keep], ca2[keep]) and st2["n_bad_rows"] == 0 and st2["flags"] == 0


def test_stale_estimates_change_the_command_on_ring13():
    """ring13 flown on own estimates with a gossip round every 2 control steps
    (tracking_dt 20 ms / control_dt 10 ms): a neighbour's entry is a step old
    on every odd step, so the own-estimate u differs from the shared-snapshot u
    of the same moment by more than the parity tolerance."""
    cs = EC.case("ring13")
    n = cs.n
    tr = GO.Trackers(cs.adj)
    q, vel = np.array(cs.q0), np.array(cs.vel0)
    P = np.arange(n, dtype=np.uint16)
    worst = 0.0
    for s in range(12):
        if s % 2 == 0:
            tr.one_round(q)
        u, us, _, _ = CO.control_step(tr.est(), vel, tr.Pt, cs.p, cs.adj, cs.gains)
        u0, _, _ = E.control_step(q, vel, cs.p, cs.adj, cs.gains, P)
        if s % 2 == 0:  # a round has just run: every neighbour's entry is current
            assert np.array_equal(u, u0)
        else:
            worst = max(worst, _rel(u, u0).max())
        q, vel = E.make_safe_traj(q, vel, us, cs.ep)
    assert worst > TOL


def test_phantom_at_the_origin():
    """rings12 (two components): a vehicle never hears of the other ring, whose
    entries stay at the origin however long the gossip runs. Moved to within
    d_avoid_thresh of (0, 0) and heading there, it is turned away by vehicles
    that are nowhere near; the shared-snapshot control raises no flag."""
    sc = C.rings12()
    n = sc.n
    s = O.default_safety()
    gains = EC.case("rings12").gains
    q = np.array(sc.windows[0][1])
    v = 0
    q[v, :2] = [0.9, 0.3]  # |q_v| < d_avoid_thresh = 1.5
    far = np.hypot(q[:, 0] - q[v, 0], q[:, 1] - q[v, 1])
    assert (np.delete(far, v) > s.d_avoid_thresh + 0.5).all()
    tr = GO.Trackers(sc.adj)
    tr.run(2 * n, q)
    est = tr.est()
    unknown = tr.stamps()[v] == 0
    assert unknown.sum() == 6 and not est[v][unknown].any()
    vel = np.zeros((n, 3))
    P = np.arange(n, dtype=np.uint16)
    u, us, ca, st = CO.control_step(est, vel, tr.Pt, sc.p, sc.adj, gains)
    u0, us0, ca0 = E.control_step(q, vel, sc.p, sc.adj, gains, P)
    # the ring's own entries are current, so DistCntrl's command is the same
    assert np.array_equal(u[v], u0[v])
    # heading for the origin (the saturated command points into the phantoms'
    # sector): steer the case there, so that the test does not rest on chance
    cmd = O.saturate(np.array([-q[v, 0], -q[v, 1], 0.0]))
    c_own, mod_own = O.collision_avoidance(v, est[v], cmd, s)
    c_sh, mod_sh = O.collision_avoidance(v, q, cmd, s)
    assert mod_own and not mod_sh
    assert np.array_equal(c_sh, cmd) and not np.array_equal(c_own, cmd)
    assert ca0[v] == 0 and np.array_equal(us0[v], O.saturate(u0[v]))
    # and through the control step itself: somewhere on the circle of radius 1
    # around the origin DistCntrl's own command heads into the phantoms
    hit = 0
    for k in range(16):
        q[v, :2] = [np.cos(k * np.pi / 8), np.sin(k * np.pi / 8)]
        tr.run(1, q)
        u, us, ca, st = CO.control_step(tr.est(), vel, tr.Pt, sc.p, sc.adj, gains)
        u0, us0, ca0 = E.control_step(q, vel, sc.p, sc.adj, gains, P)
        assert np.array_equal(u[v], u0[v]) and ca0[v] == 0
        if ca[v]:
            hit += 1
            assert st["n_ca"] >= 1 and not np.array_equal(us[v], us0[v])
    assert hit >= 1


def test_input_condition():
    """For every vehicle of every case that has a close vehicle: every
    |dist - d_avoid_thresh| >= 1e-6, psi at least 1e-4 rad from every
    no-fly-zone edge and from the |wrapToPi(edge - psi)| = pi/2 boundary."""
    for key in K.all_keys():
        cs = K.case(*key)
        d, e, q = K.condition(cs)
        assert d >= K.D_MARGIN and e >= K.ANGLE_MARGIN and q >= K.ANGLE_MARGIN, (cs.name, d, e, q)


def test_coverage():
    """The cases reach every resolve path and special sector the GPU tests
    claim: at most 2 close vehicles, 3-16, 17 and more (over 64 edge slots),
    a wrapped sector, a surrounded vehicle whose command is zeroed, a NaN
    estimate of a non-neighbour, unknown entries, a bad row, and the phantom:
    a spread case in which unknown entries at the origin are the close ones."""
    tot = dict(le2=0, mid=0, ge17=0, wrapped=0, zeroed=0, nan=0)
    for key in K.all_keys():
        cs = K.case(*key)
        cov = K.coverage(cs)
        tot["le2"] += sum(1 for c in cov["close"] if 1 <= c <= 2)
        tot["mid"] += sum(1 for c in cov["close"] if 3 <= c <= 16)
        tot["ge17"] += sum(1 for c in cov["close"] if c >= 17)
        for k in ("wrapped", "zeroed", "nan"):
            tot[k] += cov[k]
        assert cs.bad and cs.reference()[3]["n_bad_rows"] == 1
        assert cs.n <= 6 or cs.unknown.any()
        if cs.nan:
            v, j = cs.nan
            u, us, ca, _ = cs.reference()
            assert np.isnan(cs.est[v, j]).all() and np.isfinite(u[v]).all() and ca[v] == 0
            assert np.array_equal(us[v], O.saturate(u[v]))
    assert all(tot.values()), tot
    assert sum(1 for k in K.all_keys() if K.case(*k).nan) == len(K.NAN_CASES)
    # 4 slots per close vehicle: the general path from 17 close vehicles on
    assert 4 * 17 > 64 >= 4 * 16
    cs = K.case(128, "spread", 5)
    v = int(np.argmax(K.coverage(cs)["close"]))
    vs = [w for w in range(cs.n) if w not in cs.bad]
    sc = CO.sectors(vs[v], cs.est[vs[v]])
    assert sc["close"] >= 17 and np.hypot(*cs.est[vs[v], vs[v], :2]) < O.default_safety().d_avoid_thresh


# ---- the ABI without a GPU ----

def test_exports_and_struct_layout():
    from aclswarm_amd import _lib as L
    lib = L.lib()
    assert "acl_fleet_est_control_batch" in L.EXPORTS and hasattr(lib, "acl_fleet_est_control_batch")
    A = L.FleetEstControlArgs
    assert ct.sizeof(A) == 8 + 8 * 8 + 64 + 32
    assert (A.fidx.offset, A.status.offset, A.cntrl.offset, A.safety.offset) == (8, 64, 72, 136)
    assert L.FLEET_CONTROL_STATUS_DTYPE.itemsize == 16
    assert L.FLEET_CTL_BAD_ROW == CO.BAD_ROW and L.FLEET_BAD_INPUT == CO.BAD_INPUT
    assert lib.acl_abi_version() == 11


def test_est_control_argument_errors_without_gpu():
    from aclswarm_amd import _lib as L
    lib = L.lib()
    call = lib.acl_fleet_est_control_batch
    name = b"acl_fleet_est_control_batch: "
    F = L.Formations(129, 1, None, None, None, None, 5, None)
    a = L.FleetEstControlArgs()

    def fails(msg):
        assert call(ct.byref(F), ct.byref(a), None) == 1  # INVALID_ARG
        err = lib.acl_last_error()
        assert err.startswith(name) and msg in err, err

    a.B = 1
    fails(b"n out of range [1, 128]")
    F.n = 0
    fails(b"n out of range [1, 128]")
    F.n = 13
    fails(b"required pointer is NULL")
    a.B = -1
    fails(b"B < 0")
    a.B = 1
    F.gain_planes = 7
    fails(b"gain_planes must be 9 (or 0) or 5")
    F.gain_planes = 0
    need = ("fidx", "est", "vel", "Pt", "u_safe", "ca_flag", "status")
    form = ("p", "adj", "gains", "gain_off")
    for k in need:
        setattr(a, k, 8)  # never dereferenced: the calls below fail their checks
    for k in form:
        setattr(F, k, 8)
    for obj, keys in ((a, need), (F, form)):
        for k in keys:
            setattr(obj, k, None)
            fails(b"required pointer is NULL")
            setattr(obj, k, 8)
    F.n_formations = 0
    fails(b"formation table is empty")
    F.n_formations = 1
    a.B = 0
    a.fidx = None
    assert call(ct.byref(F), ct.byref(a), None) == 0  # empty batch (u may be NULL throughout)
    assert call(None, ct.byref(a), None) == 1 and call(ct.byref(F), None, None) == 1
    assert lib.acl_last_error() == name + b"null argument"
