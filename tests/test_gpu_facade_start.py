"""The facade's exchange-mode start (include/aclswarm_amd.hpp,
Auctioneer::start with setBidExchange): one acl_vehicle_start_batch call per
vehicle -- its alignment under its OWN assignment and its START bid -- instead
of a whole-swarm acl_solve_batch. Driven through tests/facade_start_driver.cpp
(aclswarm_amd/lib/libfacade_start_driver.so, loaded by ctypes).

Checked bit for bit against the oracle's composition for each vehicle's row,
  pyoracle.align(n, v, q, p, adj, P_v)  then
  cbaa_step_oracle.step(v, True, 0s, -1s, [], price_row(p, q[v], Rt)),
and a vehicle whose assignment is not a permutation must report
ACL_ERR_INVALID_ARG, send no bid and stay idle."""
import ctypes as ct
import os

import numpy as np
import pytest

import cbaa_step_oracle as S
import helpers as H
import pyoracle as O

pytestmark = pytest.mark.gpu

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "aclswarm_amd", "lib", "libfacade_start_driver.so")
ACL_OK, ACL_ERR_INVALID_ARG = 0, 1
ERR_LEN = 160


def _fleet(p, adj, q, P_rows):
    n = p.shape[0]
    if not os.path.exists(LIB):
        raise RuntimeError(f"{LIB} missing: run python -m aclswarm_amd.build")
    lib = ct.CDLL(LIB)
    VP = ct.c_void_p
    lib.facade_start_fleet.argtypes = [ct.c_int] + [VP] * 11 + [ct.c_int]
    p_cm = np.asfortranarray(p, np.float64)
    q_cm = np.asfortranarray(q, np.float64)
    adj_cm = np.asfortranarray(adj, np.uint8)
    rows = np.ascontiguousarray(P_rows, np.uint8)
    sends = np.full(n, -9, np.int32)
    iters = np.full(n, -9, np.int32)
    who = np.full((n, n), -9, np.int32)
    price = np.full((n, n), -9.0, np.float32)
    status = np.full(n, -9, np.int32)
    idle = np.full(n, 9, np.uint8)
    err = ct.create_string_buffer(n * ERR_LEN)
    rc = lib.facade_start_fleet(n, p_cm.ctypes.data, adj_cm.ctypes.data, q_cm.ctypes.data,
                                rows.ctypes.data, sends.ctypes.data, iters.ctypes.data,
                                who.ctypes.data, price.ctypes.data, status.ctypes.data,
                                idle.ctypes.data, ct.addressof(err), ERR_LEN)
    assert rc == 0
    errs = [err.raw[v * ERR_LEN:(v + 1) * ERR_LEN].split(b"\0")[0].decode() for v in range(n)]
    return dict(sends=sends, iters=iters, who=who, price=price, status=status, idle=idle,
                err=errs)


def _cases():
    pts, adj, _, q0 = H.swarm6()
    rng = np.random.RandomState(61)
    yield "swarm6", pts[0], adj[0], q0 + np.c_[rng.normal(0, 0.3, (6, 2)), np.zeros(6)], rng
    Pf, Af = H.simform("simform20_nc")
    rng = np.random.RandomState(62)
    yield "simform20_nc", Pf[0, 0], Af[0].astype(np.uint8), H.random_positions(rng, 20, 20.0), rng


@pytest.mark.parametrize("case", [0, 1], ids=["swarm6", "simform20_nc"])
def test_fleet_starts_from_own_assignments(case):
    """Every vehicle holds its own (different) assignment: one send-bid call
    with iter 0 whose table is the oracle's START bid for that row."""
    _, p, adj, q, rng = list(_cases())[case]
    n = p.shape[0]
    P_rows = np.stack([rng.permutation(n) for _ in range(n)]).astype(np.uint8)
    assert len({tuple(r) for r in P_rows}) == n
    got = _fleet(p, adj, q, P_rows)
    np.testing.assert_array_equal(got["sends"], np.ones(n))
    np.testing.assert_array_equal(got["iters"], np.zeros(n))
    np.testing.assert_array_equal(got["status"], np.full(n, ACL_OK))
    np.testing.assert_array_equal(got["idle"], np.zeros(n))  # the auction is open
    assert got["err"] == [""] * n
    for v in range(n):
        R, t = O.align(n, v, q, p, adj, P_rows[v].astype(np.uint16))
        Rt = np.concatenate([R.reshape(4), t])
        pr, wh, task, _ = S.step(v, True, np.zeros(n, np.float32), np.full(n, -1, np.int32), [],
                                 S.price_row(p, q[v], Rt))
        assert task >= 0
        np.testing.assert_array_equal(got["who"][v], wh, err_msg=f"vehicle {v}")
        np.testing.assert_array_equal(got["price"][v].view(np.uint32), pr.view(np.uint32),
                                      err_msg=f"vehicle {v}")


@pytest.mark.parametrize("case", [0, 1], ids=["swarm6", "simform20_nc"])
def test_non_permutation_assignment_starts_nothing(case):
    """Vehicle 2 is given P with a duplicated index (P[0] = P[1] = 0: its Pt_
    then holds vehicle 1 twice). It must not price a bid from a stale
    alignment: INVALID_ARG, no bid, idle. The others are unaffected."""
    _, p, adj, q, rng = list(_cases())[case]
    n = p.shape[0]
    P_rows = np.tile(np.arange(n, dtype=np.uint8), (n, 1))
    bad = 2
    P_rows[bad, 1] = 0
    got = _fleet(p, adj, q, P_rows)
    assert got["status"][bad] == ACL_ERR_INVALID_ARG
    assert "not a permutation" in got["err"][bad]
    assert got["sends"][bad] == 0 and got["iters"][bad] == -1
    assert got["idle"][bad] == 1
    assert (got["who"][bad] == -9).all() and (got["price"][bad] == -9.0).all()
    ok = np.arange(n) != bad
    assert (got["status"][ok] == ACL_OK).all() and (got["sends"][ok] == 1).all()
    assert (got["idle"][ok] == 0).all()
