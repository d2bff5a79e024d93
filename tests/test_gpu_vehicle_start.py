"""GPU parity of acl_vehicle_start_batch (one vehicle's auction start: the
alignment under its own assignment, auctioneer.cpp:347-415, and the START
bid, :448-465,517-549) against the CPU oracle's composition
  pyoracle.align(n, v, q, p, adj, argsort(row))
  cbaa_step_oracle.step(v, True, 0s, -1s, [], price_row(p, q[v], Rt)),
against acl_solve_batch's align_Rt and against acl_cbaa_step_batch's START.

Bar: everything bit for bit. The alignment is the oracle's f64 operations in
its order (one rounding each, no contraction), the prices the same getPrice
expression rounded to float, the rest integer work."""
import ctypes as ct
import functools

import numpy as np
import pytest

import cbaa_step_oracle as S
import helpers as H
import pyoracle as O

pytestmark = pytest.mark.gpu

BAD, SELECTED = 0x10, 0x02


def _dev():
    import torch
    return torch.device("cuda:0")


def _t(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dt)).to(_dev())


def _u16(a):
    return _t(np.ascontiguousarray(a, np.uint16).view(np.int16), np.int16)


def _table(ps, adjs):
    from aclswarm_amd import engine
    return engine.FormationTable.from_host(ps, adjs, None, device=_dev())


def _start(ps, adjs, fidx, vehid, q, rows, qidx=None, want_bid=True):
    import torch
    from aclswarm_amd import engine
    out = engine.vehicle_start(_table(ps, adjs), _t(fidx, np.int32), _t(vehid, np.int32),
                               _t(q, np.float64), _u16(rows),
                               qidx=None if qidx is None else _t(qidx, np.int32),
                               want_bid=want_bid)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _oracle(ps, adjs, f, v, qs, row):
    """(Rt[6], price, who, task) of one vehicle: the issue's composition."""
    n = len(row)
    R, t = O.align(n, v, qs, ps[f], adjs[f], np.argsort(row).astype(np.uint16))
    Rt = np.concatenate([R.reshape(4), t])
    pr, wh, task, _ = S.step(v, True, np.zeros(n, np.float32), np.full(n, -1, np.int32), [],
                             S.price_row(ps[f], qs[v], Rt))
    return Rt, pr, wh, task


def _graphs(rng, n):
    """The full graph; a ring with a few chords (closed neighbourhoods of
    3-5); a random graph of density about 0.3 with point `iso` isolated."""
    full = np.ones((n, n), np.uint8) - np.eye(n, dtype=np.uint8)
    ring = np.zeros((n, n), np.uint8)
    for i in range(n):
        ring[i, (i + 1) % n] = ring[(i + 1) % n, i] = 1
    for a in (0, 1):
        b = a + n // 2
        ring[a, b] = ring[b, a] = 1
    u = np.triu((rng.uniform(size=(n, n)) < 0.3).astype(np.uint8), 1)
    rnd = u + u.T
    iso = n // 3
    rnd[iso, :] = 0
    rnd[:, iso] = 0
    return [full, ring, rnd], iso


@functools.lru_cache(maxsize=None)
def _parity_case(n):
    """V = 96 vehicles, S = 4 snapshots, F = 3 formations; every vehicle its
    own random permutation row. Returns the inputs, the GPU result and the
    oracle's, computed once per n (tests share them and leave them alone)."""
    rng = np.random.RandomState(7300 + n)
    V, Sn, F = 96, 4, 3
    adjs, iso = _graphs(rng, n)
    ps = [np.c_[rng.uniform(-n, n, (n, 2)), rng.uniform(0, 2, n)] for _ in range(F)]
    q = np.stack([np.c_[rng.uniform(-n, n, (n, 2)), rng.uniform(0.5, 1.5, n)]
                  for _ in range(Sn)])
    fidx = (np.arange(V) % F).astype(np.int32)
    vehid = rng.randint(0, n, V).astype(np.int32)
    qidx = rng.randint(0, Sn, V).astype(np.int32)
    rows = np.stack([rng.permutation(n) for _ in range(V)]).astype(np.uint16)
    # vehicle 5 (formation 2, the random graph) sits at the isolated point
    k0 = 5
    assert fidx[k0] == 2
    j = int(np.where(rows[k0] == vehid[k0])[0][0])
    rows[k0, j], rows[k0, iso] = rows[k0, iso], rows[k0, j]
    got = _start(ps, adjs, fidx, vehid, q, rows, qidx)
    exp = [_oracle(ps, adjs, int(fidx[k]), int(vehid[k]), q[qidx[k]], rows[k]) for k in range(V)]
    point = np.array([int(np.where(rows[k] == vehid[k])[0][0]) for k in range(V)])
    ksize = np.array([1 + int(np.delete(adjs[fidx[k]][point[k]], point[k]).sum())
                      for k in range(V)])
    for a in (q, rows, fidx, vehid, qidx, point, ksize):
        a.setflags(write=False)
    return dict(ps=ps, adjs=adjs, iso=iso, q=q, fidx=fidx, vehid=vehid, qidx=qidx, rows=rows,
                got=got, exp=exp, point=point, ksize=ksize)


@pytest.mark.parametrize("n", [7, 64, 65, 128, 129, 300, 512])
def test_start_matches_oracle(n):
    c = _parity_case(n)
    got, exp = c["got"], c["exp"]
    V = len(c["vehid"])
    # the cases hold what they are meant to (asserted so nobody thins them)
    if n >= 16:
        assert (c["ksize"] < 16).any() and (c["ksize"] >= 16).any()  # lazy and GEMM forms
        assert ((c["fidx"] == 2) & (c["point"] == c["iso"])).any()   # the isolated point
        assert (c["ksize"] == 1).any()
    for k in range(V):
        eRt, epr, ewh, etask = exp[k]
        assert np.isfinite(eRt).all(), k
        np.testing.assert_array_equal(got["Rt"][k].view(np.uint64), eRt.view(np.uint64),
                                      err_msg=f"Rt of vehicle {k} (k = {c['ksize'][k]})")
        np.testing.assert_array_equal(got["price"][k].view(np.uint32), epr.view(np.uint32),
                                      err_msg=str(k))
        np.testing.assert_array_equal(got["who"][k], ewh, err_msg=str(k))
        assert got["task"][k] == etask, k
        assert got["flags"][k] == (SELECTED if etask >= 0 else 0), k
    assert (got["task"] >= 0).all()


def test_isolated_point_is_identity_and_translation():
    """k = 1: R = I and t = q - p (the composition's own check of the issue)."""
    c = _parity_case(65)
    k = 5
    f, v, i = int(c["fidx"][k]), int(c["vehid"][k]), int(c["point"][k])
    assert c["ksize"][k] == 1 and i == c["iso"]
    Rt = c["got"]["Rt"][k]
    np.testing.assert_array_equal(Rt[:4], [1.0, 0.0, 0.0, 1.0])
    np.testing.assert_array_equal(Rt[4:], c["q"][c["qidx"][k], v, :2] - c["ps"][f][i, :2])


def _solve_case(rng, n):
    """One swarm whose graph has sparse rows (lazy form) and, for n >= 16,
    hub points adjacent to everyone (GEMM form)."""
    u = np.triu((rng.uniform(size=(n, n)) < min(0.15, 3.0 / n)).astype(np.uint8), 1)
    adj = u + u.T
    for i in range(n):
        adj[i, (i + 1) % n] = adj[(i + 1) % n, i] = 1
    for h in (2, n // 2):
        adj[h, :] = 1
        adj[:, h] = 1
    np.fill_diagonal(adj, 0)
    p = np.c_[rng.uniform(-n, n, (n, 2)), rng.uniform(0, 2, n)]
    q = np.c_[rng.uniform(-n, n, (n, 2)), np.ones(n)]
    return p, adj, q, H.random_perm(rng, n)


def _solve_align(p, adj, q, P_in, rows=None):
    import torch
    from aclswarm_amd import engine
    n = p.shape[0]
    dev = _dev()
    kw = {}
    if rows is not None:
        kw = dict(P_rows=_u16(rows[None]), P_rows_on=_t([1], np.uint8))
    out = engine.solve(_table([p], [adj]), torch.zeros(1, dtype=torch.int32, device=dev),
                       _t(q[None], np.float64),
                       torch.zeros((1, n, 3), dtype=torch.float64, device=dev),
                       _u16(P_in[None]), do_control=False, want_who=True, want_align=True, **kw)
    torch.cuda.synchronize()
    assert not (_status(out)["flags"][0] & 0x10)
    who = out["who"].cpu().numpy().view(np.uint16)[0].astype(np.int32)
    return out["align_Rt"].cpu().numpy()[0], np.where(who == 0xFFFF, -1, who)


def _status(out):
    from aclswarm_amd import engine
    return engine.status_to_numpy(out["status"])


@pytest.mark.parametrize("n,own", [(20, False), (100, False), (160, False), (100, True)])
def test_same_bits_as_the_batched_solve(n, own):
    """V = n vehicles of one swarm, every row the inverse of P_in (or, own:
    differing rows with P_rows on): Rt is acl_solve_batch's align_Rt bit for
    bit -- the inline-alignment kernel (n <= 64), align_kernel and the wide
    path."""
    rng = np.random.RandomState(7400 + n + own)
    p, adj, q, P_in = _solve_case(rng, n)
    Pt = np.zeros(n, np.uint16)
    Pt[P_in] = np.arange(n, dtype=np.uint16)
    if own:
        from test_gpu_own_rows import _own_rows
        rows = _own_rows(rng, P_in, 0.5)
        assert (rows != Pt).any()
    else:
        rows = np.tile(Pt, (n, 1))
    Rt_solve, _ = _solve_align(p, adj, q, P_in, rows if own else None)
    got = _start([p], [adj], np.zeros(n, np.int32), np.arange(n, dtype=np.int32), q[None], rows,
                 qidx=np.zeros(n, np.int32), want_bid=False)
    assert set(got) == {"Rt", "flags"} and (got["flags"] == 0).all()
    ks = 1 + adj.sum(1)
    assert (ks < 16).any() and (ks >= 16).any()
    assert np.isfinite(Rt_solve).all()
    np.testing.assert_array_equal(got["Rt"].view(np.uint64), Rt_solve.view(np.uint64))


def test_start_equals_the_tally_kernels_start():
    """The returned Rt fed to acl_cbaa_step_batch with start = 1 gives the
    same table and task (one header makes both)."""
    from test_gpu_cbaa_step import _run as step_run
    c = _parity_case(129)
    got = c["got"]
    V, n = c["rows"].shape
    q_own = c["q"][c["qidx"], c["vehid"]]
    rng = np.random.RandomState(1)
    pr, wh, task, flags = step_run(
        c["ps"], c["fidx"].copy(), c["vehid"].copy(), q_own, got["Rt"], np.ones(V, np.uint8),
        rng.uniform(0, 1, (V, n)).astype(np.float32), rng.randint(-1, n, (V, n)),
        [[] for _ in range(V)])
    np.testing.assert_array_equal(pr.view(np.uint32), got["price"].view(np.uint32))
    np.testing.assert_array_equal(wh, got["who"])
    np.testing.assert_array_equal(task, got["task"])
    np.testing.assert_array_equal(flags, got["flags"])


def test_protocol_from_vehicle_start_equals_one_call_consensus():
    """simform20_nc: vehicle_start for all n vehicles (alignment and START
    bids; no acl_solve_batch supplies the alignment), then 2n tallies from the
    neighbours' bids of the same iteration: the final tables are
    acl_solve_batch's `who`."""
    from test_gpu_cbaa_step import _run as step_run
    Pf, Af = H.simform("simform20_nc")
    p, adj = Pf[0, 0], Af[0].astype(np.uint8)
    n = p.shape[0]
    rng = np.random.RandomState(5)
    q = H.random_positions(rng, n, 20.0)
    P = H.random_perm(rng, n)
    Pt = np.empty(n, np.int64)
    Pt[P] = np.arange(n)
    ids = np.arange(n, dtype=np.int32)
    got = _start([p], [adj], np.zeros(n, np.int32), ids, q[None], np.tile(Pt, (n, 1)),
                 qidx=np.zeros(n, np.int32))
    assert (got["flags"] == SELECTED).all()
    Rt, pr, wh = got["Rt"], got["price"], got["who"]
    nbrs = [sorted(int(Pt[j]) for j in range(n) if adj[P[v]][j]) for v in range(n)]
    for _ in range(2 * n):
        cands = [[(u, pr[u], wh[u]) for u in sorted(set(nbrs[v]) | {v})] for v in range(n)]
        pr, wh, _, fl = step_run([p], np.zeros(n, np.int32), ids, q, Rt, np.zeros(n, np.uint8),
                                 pr, wh, cands)
        assert not (fl & BAD).any()
    _, who_1 = _solve_align(p, adj, q, P)
    np.testing.assert_array_equal(wh, who_1)


def _raw_start(T, fidx, vehid, qidx, q, rows, Rt, price, who, task, flags, S_rows):
    """The C entry itself, on caller-owned (pre-filled) device outputs."""
    import torch
    from aclswarm_amd import _lib as L
    a = L.VehicleStartArgs()
    a.V, a.S = len(vehid), S_rows
    a.fidx = fidx.data_ptr(); a.vehid = vehid.data_ptr(); a.qidx = qidx.data_ptr()
    a.q = q.data_ptr(); a.Pt = rows.data_ptr(); a.Rt = Rt.data_ptr()
    a.price = price.data_ptr(); a.who = who.data_ptr(); a.task = task.data_ptr()
    a.flags = flags.data_ptr()
    F = T.struct()
    stream = torch.cuda.current_stream(_dev()).cuda_stream
    assert L.lib().acl_vehicle_start_batch(ct.byref(F), ct.byref(a), ct.c_void_p(stream)) == 0
    torch.cuda.synchronize()


def test_bad_input_is_flagged_and_leaves_the_tables():
    n, V, F, Sn = 10, 8, 3, 2
    rng = np.random.RandomState(11)
    adjs, _ = _graphs(rng, n)
    ps = [np.c_[rng.uniform(-n, n, (n, 2)), rng.uniform(0, 2, n)] for _ in range(F)]
    q = np.stack([np.c_[rng.uniform(-n, n, (n, 2)), np.ones(n)] for _ in range(Sn)])
    fidx = (np.arange(V) % F).astype(np.int32)
    vehid = rng.randint(0, n, V).astype(np.int32)
    qidx = (np.arange(V) % Sn).astype(np.int32)
    rows = np.stack([rng.permutation(n) for _ in range(V)]).astype(np.uint16)
    good = (0, 4)
    rows[1, 3] = rows[1, 7]   # a duplicate in the row
    rows[2, 6] = n            # an entry = n
    vehid[3] = n
    fidx[5] = F
    qidx[6] = Sn
    qidx[7] = -1
    SENT_P, SENT_W = np.float32(-7.5), -77
    Rt = _t(np.full((V, 6), 123.0), np.float64)
    price = _t(np.full((V, n), SENT_P), np.float32)
    who = _t(np.full((V, n), SENT_W), np.int32)
    task = _t(np.full(V, -55), np.int32)
    flags = _t(np.full(V, -55), np.int32)
    _raw_start(_table(ps, adjs), _t(fidx, np.int32), _t(vehid, np.int32), _t(qidx, np.int32),
               _t(q, np.float64), _u16(rows), Rt, price, who, task, flags, Sn)
    Rt, price, who = Rt.cpu().numpy(), price.cpu().numpy(), who.cpu().numpy()
    task, flags = task.cpu().numpy(), flags.cpu().numpy()
    for k in range(V):
        if k in good:
            eRt, epr, ewh, etask = _oracle(ps, adjs, int(fidx[k]), int(vehid[k]), q[qidx[k]],
                                           rows[k])
            np.testing.assert_array_equal(Rt[k].view(np.uint64), eRt.view(np.uint64))
            np.testing.assert_array_equal(price[k].view(np.uint32), epr.view(np.uint32))
            np.testing.assert_array_equal(who[k], ewh)
            assert task[k] == etask >= 0 and flags[k] == SELECTED
        else:
            assert flags[k] == BAD and task[k] == -1, k
            assert np.isnan(Rt[k]).all(), k
            assert (price[k] == SENT_P).all() and (who[k] == SENT_W).all(), k


def test_non_finite_snapshot_is_the_references_arithmetic():
    """A neighbour's x is NaN: no error; Rt all NaN, the table reset, no task
    (NaN prices are never eligible). Alignment only gives the same Rt."""
    n = 10
    rng = np.random.RandomState(12)
    adjs, _ = _graphs(rng, n)
    ps = [np.c_[rng.uniform(-n, n, (n, 2)), rng.uniform(0, 2, n)]]
    q = np.c_[rng.uniform(-n, n, (n, 2)), np.ones(n)][None].copy()
    rows = np.stack([rng.permutation(n) for _ in range(2)]).astype(np.uint16)
    vehid = np.array([3, 4], np.int32)
    # vehicle 3's ring neighbour (formation point i + 1) is the vehicle there
    i = int(np.where(rows[0] == 3)[0][0])
    nb = int(rows[0, (i + 1) % n])
    q[0, nb, 0] = np.nan
    i1 = int(np.where(rows[1] == 4)[0][0])
    clean = nb not in [int(rows[1, j]) for j in range(n) if j == i1 or adjs[1][i1, j]]
    got = _start(ps, [adjs[1]], np.zeros(2, np.int32), vehid, q, rows, qidx=np.zeros(2, np.int32))
    assert np.isnan(got["Rt"][0]).all()
    assert got["flags"][0] == 0 and got["task"][0] == -1
    assert (got["price"][0] == 0).all() and (got["who"][0] == -1).all()
    eRt, epr, ewh, etask = _oracle(ps, [adjs[1]], 0, 3, q[0], rows[0])
    assert np.isnan(eRt).all() and etask == -1 and (epr == 0).all() and (ewh == -1).all()
    if clean:  # the other vehicle's neighbourhood does not hold the NaN
        assert np.isfinite(got["Rt"][1]).all() and got["flags"][1] == SELECTED
    only = _start(ps, [adjs[1]], np.zeros(2, np.int32), vehid, q, rows,
                  qidx=np.zeros(2, np.int32), want_bid=False)
    assert set(only) == {"Rt", "flags"}
    np.testing.assert_array_equal(np.isnan(only["Rt"]), np.isnan(got["Rt"]))
    np.testing.assert_array_equal(only["Rt"][1].view(np.uint64), got["Rt"][1].view(np.uint64))
