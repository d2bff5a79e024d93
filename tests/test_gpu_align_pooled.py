"""GPU: the alignment launch of 64 < n <= 128 (align_kernel), which pools the
alignment work items of consecutive swarms into shared 64-lane chunks.

An item is a formation row whose closed neighbourhood is incomplete, plus one
item for all complete rows (align_worklist's rule, restated in _items below
and asserted on the hand-built graphs before the GPU runs). Every comparison
is exact: align_Rt against the Rt of the oracle's prices(), P_out, the status
fields and `who` against the oracle's solve.

Shapes: n = 65 (the smallest n of this launch), 100, 128; B = 1, 7, 9, 17, 33
(a partial last group and a group boundary for any group size in 2 ... 32);
every swarm has its own formation. Item counts 1, 3, 63, 64, 65 and n (no
complete row), orders in which a chunk straddles two and three swarms
(40 + 40 + 1 + 65), groups whose items sum to exactly 64 and 65 for each group
size, a sparse formation (the lazy product form) next to near-complete ones,
a bad swarm in the middle of good ones, one own-row swarm between two others.

Two things asked of this file cannot be built. A count of exactly 2 items
does not exist for n >= 3: the adjacency is symmetric, so incomplete rows come
at least in pairs, and a pair plus the complete rows' item is 3 (the count
used here). And the engine does not split a call, so no launch has b0 != 0.
"""
import numpy as np
import pytest

import pyoracle as O
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

BAD_INPUT, CA_ACTIVE = 0x10, 0x20  # ACL_SWARM_BAD_INPUT, ACL_SWARM_CA_ACTIVE
RING = "ring"


def _items(adj):
    """align_worklist's rule: the rows with an incomplete closed
    neighbourhood, plus one item when any row is complete."""
    n = adj.shape[0]
    closed = adj.astype(bool) | np.eye(n, dtype=bool)
    ninc = int((closed.sum(1) < n).sum())
    return ninc + (1 if ninc < n else 0)


def _graph(rng, n, count):
    """A connected formation graph with `count` alignment items: the complete
    graph minus a path through m randomly chosen rows (those m rows become
    incomplete); RING: the cycle (3 members per row: every item takes the
    lazy product form)."""
    if count == RING:
        a = np.zeros((n, n), np.uint8)
        i = np.arange(n)
        a[i, (i + 1) % n] = a[(i + 1) % n, i] = 1
        assert _items(a) == n
        return a
    assert count == 1 or 3 <= count <= n
    m = 0 if count == 1 else (n if count == n else count - 1)
    a = np.ones((n, n), np.uint8) - np.eye(n, dtype=np.uint8)
    rows = rng.permutation(n)[:m]
    for i, j in zip(rows[:-1], rows[1:]):
        a[i, j] = a[j, i] = 0
    assert _items(a) == count, (count, _items(a))
    return a


def _inputs(rng, n, counts):
    B = len(counts)
    adjs = [_graph(rng, n, c) for c in counts]
    pts = [np.c_[rng.uniform(-n, n, (n, 2)), rng.uniform(0, 2, n)] for _ in range(B)]
    q = np.stack([np.c_[rng.uniform(-n, n, (n, 2)), np.ones(n)] for _ in range(B)])
    P_in = np.stack([rng.permutation(n).astype(np.uint16) for _ in range(B)])
    return pts, adjs, q, P_in


def _gpu(pts, adjs, fidx, q, P_in, rows=None, on=None):
    import torch
    from aclswarm_amd import engine
    dev = torch.device("cuda:0")
    B, n = q.shape[0], q.shape[1]
    T = engine.FormationTable.from_host(pts, adjs, None, device=dev)
    kw = {}
    if rows is not None:
        kw = dict(P_rows=torch.from_numpy(np.ascontiguousarray(rows, np.uint16).view(np.int16)).to(dev),
                  P_rows_on=torch.from_numpy(np.asarray(on, np.uint8)).to(dev))
    out = engine.solve(T, torch.from_numpy(np.asarray(fidx, np.int32)).to(dev),
                       torch.from_numpy(np.ascontiguousarray(q)).to(dev),
                       torch.zeros((B, n, 3), dtype=torch.float64, device=dev),
                       torch.from_numpy(np.ascontiguousarray(P_in, np.uint16).view(np.int16)).to(dev),
                       do_control=False, want_who=True, want_align=True, **kw)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["P_out"] = res["P_out"].view(np.uint16)
    res["who"] = res["who"].view(np.uint16)
    res["status"] = np.ascontiguousarray(res["status"]).view(O.STATUS_DTYPE).reshape(-1)
    return res


def _oracle_one(pts, adj, q, P_in, rows=None):
    n = q.shape[0]
    r = O.solve(q, np.zeros((n, 3)), pts, adj, np.zeros((3 * n, 3 * n)), P_in, P_rows=rows)
    # the GPU calls here run the auction only (do_control=False): the control
    # stage's flag is not theirs
    r["status"]["flags"] = int(r["status"]["flags"]) & ~CA_ACTIVE
    return r


def _check(gpu, pts, adjs, q, P_in, swarms=None):
    """Swarms b (formation b each): align_Rt, who, P_out, status, all exact."""
    B = q.shape[0]
    swarms = list(range(B)) if swarms is None else swarms
    for b in swarms:
        _, Rt_ref = O.prices(q[b], pts[b], adjs[b], P_in[b])
        np.testing.assert_array_equal(gpu["align_Rt"][b], Rt_ref, err_msg=f"align_Rt swarm {b}")
    sel = {k: v[swarms] for k, v in gpu.items()}
    _compare(sel, [_oracle_one(pts[b], adjs[b], q[b], P_in[b]) for b in swarms],
             check_control=False)


def _counts(rng, n, B):
    if B == 1:
        return [65]                      # one swarm, two chunks
    if B == 7:
        return [1, 3, 63, 64, 65, n, RING]
    # 40 + 40 + 1 + 65: chunk 0 straddles two swarms, chunk 1 three; the
    # sparse formation sits between near-complete ones
    head = [40, 40, 1, 65, RING, 3, n, 1, 64]
    more = [RING if k % 5 == 4 else int(rng.choice([1] + list(range(3, n + 1))))
            for k in range(B - len(head))]
    return head + more


@pytest.mark.parametrize("B", [1, 7, 9, 17, 33])
@pytest.mark.parametrize("n", [65, 100, 128])
def test_pooled_alignment_matches_oracle(cuda, n, B):
    rng = np.random.RandomState(9000 + 64 * n + B)
    counts = _counts(rng, n, B)
    assert len(counts) == B
    pts, adjs, q, P_in = _inputs(rng, n, counts)
    gpu = _gpu(pts, adjs, np.arange(B), q, P_in)
    _check(gpu, pts, adjs, q, P_in)


@pytest.mark.parametrize("total", [64, 65])
@pytest.mark.parametrize("S", [2, 4, 8, 16, 32])
def test_group_items_sum_to_a_chunk(cuda, S, total):
    """S swarms whose items sum to exactly `total` (a group of that size
    fills one chunk exactly, or spills one item into a second), then one more
    group's worth of small swarms after the boundary."""
    n = 100
    rng = np.random.RandomState(9500 + 4 * S + total)
    counts = [total - (S - 1)] + [1] * (S - 1) + [3] * min(S, 4)
    assert sum(counts[:S]) == total
    pts, adjs, q, P_in = _inputs(rng, n, counts)
    gpu = _gpu(pts, adjs, np.arange(len(counts)), q, P_in)
    _check(gpu, pts, adjs, q, P_in)


@pytest.mark.parametrize("kind", ["not_a_permutation", "fidx_minus_1", "fidx_F"])
def test_bad_swarm_inside_a_group(cuda, kind):
    """One bad swarm among good ones: it is BAD_INPUT, and its neighbours'
    outputs are those of the same call without it (and the oracle's)."""
    n, B, bad = 100, 9, 3
    rng = np.random.RandomState(9700)
    counts = [40, 40, 1, 65, RING, 3, n, 1, 64]
    pts, adjs, q, P_in = _inputs(rng, n, counts)
    fidx = np.arange(B)
    if kind == "not_a_permutation":
        P_in[bad, 7] = P_in[bad, 90]
    else:
        fidx[bad] = -1 if kind == "fidx_minus_1" else B
    good = [b for b in range(B) if b != bad]
    gpu = _gpu(pts, adjs, fidx, q, P_in)
    assert gpu["status"]["flags"][bad] == BAD_INPUT
    np.testing.assert_array_equal(gpu["P_out"][bad], P_in[bad])
    assert (gpu["who"][bad] == 0xFFFF).all()
    _check(gpu, pts, adjs, q, P_in, swarms=good)
    without = _gpu(pts, adjs, fidx[good], q[good], P_in[good])
    for key in ("align_Rt", "P_out", "who", "status"):
        np.testing.assert_array_equal(gpu[key][good], without[key], err_msg=key)


def test_own_row_swarm_between_two_others(cuda):
    """A swarm that runs from its vehicles' own rows (P_rows_on) takes its
    alignments from them in the auction kernel; its neighbours in the group
    take the pooled launch's."""
    n, B = 100, 3
    rng = np.random.RandomState(9800)
    pts, adjs, q, P_in = _inputs(rng, n, [65, 40, 64])
    rows = np.zeros((B, n, n), np.uint16)
    for b in range(B):
        rows[b, :, P_in[b]] = np.arange(n, dtype=np.uint16)  # every row: the inverse of P_in
    v = 11  # vehicle v holds another table: two other points swapped
    a, c = [j for j in range(n) if j != P_in[1, v]][:2]
    rows[1, v, a], rows[1, v, c] = rows[1, v, c], rows[1, v, a]
    on = np.array([0, 1, 0], np.uint8)
    gpu = _gpu(pts, adjs, np.arange(B), q, P_in, rows=rows, on=on)
    _check(gpu, pts, adjs, q, P_in, swarms=[0, 2])
    _compare({k: x[1:2] for k, x in gpu.items()},
             [_oracle_one(pts[1], adjs[1], q[1], P_in[1], rows=rows[1])], check_control=False)
