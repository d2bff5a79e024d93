"""GPU parity of acl_fleet_est_control_batch (one control step, every vehicle
on its own table of estimates under its own row) against the plain-Python
restatement tests/fleet_est_control_oracle.py on tests/fleet_est_control_cases.py.

Bar (the project's own, as tests/test_gpu_parity.py): u and u_safe within
|d| / max(|ref|, 1) <= 1e-5, ca_flag and the status words exact, for every
vehicle of every case -- the cases' input condition (asserted on the CPU in
tests/test_fleet_est_control.py) keeps a 1e-5 difference in u from flipping a
collision decision. Sizes: n = 1, 2, 6, 13, 20 (three vehicles per wave), 64,
65 (the second lane chunk), 100 and 128, both gain layouts; every launch has at
most 8 swarms."""
import numpy as np
import pytest

import fleet_est_control_cases as K
import fleet_est_control_oracle as CO
import test_gpu_fleet_auction as G

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _run(cases, fidx=None, want=("u", "u_safe", "ca_flag", "status")):
    """The cases (one n, one gain layout) as the swarms of one launch."""
    import torch
    from aclswarm_amd import _lib as L
    from aclswarm_amd import engine
    c0 = cases[0]
    assert all((c.n, c.planes) == (c0.n, c0.planes) for c in cases)
    T = engine.FormationTable.from_host([c.p for c in cases], [c.adj for c in cases],
                                        [c.gains for c in cases], device=G._dev())
    assert T.gain_planes == c0.planes or c0.n == 1  # (no edges: either layout)
    fidx = np.arange(len(cases)) if fidx is None else np.asarray(fidx)
    out = engine.fleet_est_control(T, G._t(fidx, np.int32),
                                   G._t(np.stack([c.est for c in cases]), np.float64),
                                   G._t(np.stack([c.vel for c in cases]), np.float64),
                                   G._u16(np.stack([c.Pt for c in cases])))
    torch.cuda.synchronize()
    got = {k: out[k].cpu().numpy() for k in want}
    got["status"] = np.ascontiguousarray(got["status"]).view(L.FLEET_CONTROL_STATUS_DTYPE).reshape(-1)
    return got


def _close(got, ref, what):
    err = np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)
    # (a NaN on either side fails: no case's reference holds one)
    assert np.isfinite(got).all() and err.max() <= TOL, f"{what}: {err.max():.3e}"


def _compare(got, b, cs):
    u, us, ca, st = cs.reference()
    w = f"{cs.name} (swarm {b})"
    _close(got["u"][b], u, f"{w}: u")
    _close(got["u_safe"][b], us, f"{w}: u_safe")
    np.testing.assert_array_equal(got["ca_flag"][b], ca, err_msg=f"{w}: ca_flag")
    assert {k: int(got["status"][k][b]) for k in st} == st, w
    for v in cs.bad:  # the bad row: exact zeros
        assert not got["u"][b, v].any() and not got["u_safe"][b, v].any()


def _groups():
    """The cases by (n, planes): one launch each."""
    out = {}
    for n, kind, planes in K.all_keys():
        out.setdefault((n, planes), []).append((n, kind, planes))
    return out


@pytest.mark.parametrize("n,planes", sorted(_groups()))
def test_parity(cuda, n, planes):
    """Every case of one size and gain layout: perturbed tables, unknown
    entries at the origin, a row per vehicle, a bad row; the crowded cases
    cover every resolve path (tests/test_fleet_est_control.py::test_coverage)."""
    cases = [K.case(*k) for k in _groups()[(n, planes)]]
    assert len(cases) <= 8
    got = _run(cases)
    for b, cs in enumerate(cases):
        _compare(got, b, cs)


def test_bad_fidx_zeroes_the_swarm(cuda):
    cs = K.case(13, "dense", 5)
    got = _run([cs, cs, cs, cs], fidx=[0, -1, 4, 0])
    for b in (0, 3):
        _compare(got, b, cs)
    for b in (1, 2):
        assert not got["u"][b].any() and not got["u_safe"][b].any() and not got["ca_flag"][b].any()
        assert {k: int(got["status"][k][b]) for k in ("n_ca", "n_bad_rows", "reserved", "flags")} \
            == dict(n_ca=0, n_bad_rows=0, reserved=0, flags=CO.BAD_INPUT)


@pytest.mark.parametrize("n,kind,planes", [(20, "dense", 5), (13, "dense", 9), (100, "spread", 5),
                                           (128, "dense", 5)])
def test_broadcast_equals_control(cuda, n, kind, planes):
    """est broadcast from q and equal rows: acl_control_batch's commands within
    the tolerance, equal flags."""
    import torch
    from aclswarm_amd import engine
    cs = K.case(n, kind, planes)
    rng = np.random.RandomState(n)
    B = 4
    T = engine.FormationTable.from_host([cs.p], [cs.adj], [cs.gains], device=G._dev())
    q = np.stack([cs.q + rng.normal(0, 0.05, (n, 3)) for _ in range(B)])
    vel = rng.normal(0, 0.1, (B, n, 3))
    P = np.stack([rng.permutation(n) for _ in range(B)]).astype(np.uint16)  # vehicle -> point
    Pt = np.zeros((B, n), np.uint16)
    for b in range(B):
        Pt[b, P[b]] = np.arange(n)
    fidx = G._t(np.zeros(B, np.int32), np.int32)
    ref = engine.control(T, fidx, G._t(q, np.float64), G._t(vel, np.float64), G._u16(P))
    out = engine.fleet_est_control(
        T, fidx, G._t(np.broadcast_to(q[:, None], (B, n, n, 3)), np.float64),
        G._t(vel, np.float64), G._u16(np.broadcast_to(Pt[:, None], (B, n, n))))
    torch.cuda.synchronize()
    for k in ("u", "u_safe"):
        _close(out[k].cpu().numpy(), ref[k].cpu().numpy(), f"{cs.name}: {k}")
    ca = ref["ca_flag"].cpu().numpy()
    np.testing.assert_array_equal(out["ca_flag"].cpu().numpy(), ca)
    np.testing.assert_array_equal(out["status"].cpu().numpy()[:, 0], ca.sum(axis=1))
    assert ca.any()


def test_malformed_arguments_raise_before_anything_runs(cuda):
    from aclswarm_amd import engine
    cs = K.case(6, "dense", 5)
    T = engine.FormationTable.from_host([cs.p], [cs.adj], [cs.gains], device=G._dev())
    fidx = G._t(np.zeros(2, np.int32), np.int32)
    est = G._t(np.stack([cs.est] * 2), np.float64)
    vel = G._t(np.stack([cs.vel] * 2), np.float64)
    Pt = G._u16(np.stack([cs.Pt] * 2))
    with pytest.raises(ValueError):
        engine.fleet_est_control(T, fidx, est[:1], vel, Pt)
    with pytest.raises(ValueError):
        engine.fleet_est_control(T, fidx, est.float(), vel, Pt)
    with pytest.raises(ValueError):
        engine.fleet_est_control(T, fidx, est, vel, Pt[:, :, :5])
    with pytest.raises(ValueError):
        engine.fleet_est_control(T, fidx.cpu(), est, vel, Pt)
