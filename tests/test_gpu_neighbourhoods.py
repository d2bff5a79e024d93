"""The auction kernel's vehicle-space neighbourhood masks (csrc/
neighbourhood_dev.h): vehicle u is in vehicle v's mask iff u == v or
adj[P[v]][P[u]].

The masks of the bit walk, of the ballot loop and of the automatic choice
between them (acl_internal_neighbourhoods) are compared bit for bit with a
numpy model, on graphs that reach every branch of the walk (both polarities,
both words, walks at and just above the threshold), and acl_solve_batch is
compared with the CPU restatement on graphs of bridges, where one wrong bit
changes the tables or the round count."""
import ctypes as ct

import numpy as np
import pytest

import helpers as H

NS = [2, 3, 20, 63, 64, 65, 100, 127, 128]
MODES = {"auto": 0, "walk": 1, "ballot": 2}
B_PER_GRAPH = 8


def walk_max(n):
    """nb_walk_max (neighbourhood_dev.h): the longest row walk the bit walk
    is taken for."""
    waves = (n + 63) // 64
    return max(0, int((23 * n // (2 * waves) - 69) / 34))


def model(adj, P):
    """M[v][u] = (u == v) or adj[P[v]][P[u]]."""
    P = np.asarray(P, np.int64)
    return (adj[np.ix_(P, P)] != 0) | np.eye(len(P), dtype=bool)


def pack_rows(M):
    """[..., n, n] bool -> [..., n, 2] u64 (bit u & 63 of word u >> 6)."""
    n = M.shape[-1]
    out = np.zeros(M.shape[:-1] + (2,), np.uint64)
    for u in range(n):
        out[..., u >> 6] |= M[..., u].astype(np.uint64) << np.uint64(u & 63)
    return out


def _sym(a):
    a = ((a + a.T) > 0).astype(np.uint8)
    np.fill_diagonal(a, 0)
    return a


def _complete(n):
    return np.ones((n, n), np.uint8) - np.eye(n, dtype=np.uint8)


def _missing_star(n, m):
    """Complete minus the edges (0, 1..m): vertex 0 misses m neighbours."""
    a = _complete(n)
    a[0, 1:m + 1] = a[1:m + 1, 0] = 0
    return a


def _sparse_star(n, d):
    """Only the edges (0, 1..d): vertex 0 has degree d."""
    a = np.zeros((n, n), np.uint8)
    a[0, 1:d + 1] = a[1:d + 1, 0] = 1
    return a


def graphs(n, rng):
    """(name, adjacency) for size n; the longest row walk of each is noted."""
    L = walk_max(n)
    g = [("complete", _complete(n))]
    a = _complete(n)
    for i in range(0, n - 1, 2):
        a[i, i + 1] = a[i + 1, i] = 0
    g.append(("matching", a))                      # one missing neighbour per row
    g.append(("star", _sparse_star(n, n - 1)))     # centre dense, leaves sparse
    a = np.zeros((n, n), np.uint8)
    for i in range(n - 1):
        a[i, i + 1] = a[i + 1, i] = 1
    g.append(("path", a))                          # deg <= 2
    a = np.zeros((n, n), np.uint8)
    h = n // 2
    a[:h, :h] = 1
    a[h:, h:] = 1
    g.append(("two_cliques", _sym(a)))
    a = _complete(n)
    a[n // 2, :] = a[:, n // 2] = 0
    g.append(("isolated", a))
    g.append(("random_half", _sym(np.triu(rng.uniform(size=(n, n)) < 0.5, 1))))
    for name, m in (("walk_L", L), ("walk_L_plus_1", L + 1)):
        if m <= (n - 1) // 2:
            g.append((name, _missing_star(n, m)))   # vertex 0's walk is m
            assert min(m, n - 1 - m) == m
    for name, d in (("half_floor", (n - 1) // 2), ("half_ceil", n // 2)):
        g.append((name, _sparse_star(n, d)))       # deg (n - 1) / 2, either side
    a = _complete(n) + np.eye(n, dtype=np.uint8)   # a set diagonal is ignored
    g.append(("complete_with_diagonal", a))
    if n > 64:
        a = _complete(n)
        a[0, 64:] = a[64:, 0] = 0                  # row 0 misses only >= 64
        a[1, 2:40] = a[2:40, 1] = 0                # row 1 misses only < 64
        g.append(("word_split", a))
    return g


def perms(n, rng):
    """Identity and reversal (the word-split rows keep their words in vehicle
    space), then random permutations."""
    p = [np.arange(n), np.arange(n)[::-1]]
    p += [rng.permutation(n) for _ in range(B_PER_GRAPH - 2)]
    return np.stack(p).astype(np.int32)


def test_model_by_hand():
    """4 vehicles on the path 0-1-2-3 of formation points, P = [2, 0, 3, 1]:
    vehicle 0 sits at point 2 (neighbours: points 1, 3 = vehicles 3, 2),
    vehicle 1 at point 0 (point 1 = vehicle 3), vehicle 2 at point 3 (point
    2 = vehicle 0), vehicle 3 at point 1 (points 0, 2 = vehicles 1, 0)."""
    adj = np.array([[0, 1, 0, 0], [1, 0, 1, 0], [0, 1, 0, 1], [0, 0, 1, 0]], np.uint8)
    M = model(adj, [2, 0, 3, 1])
    want = np.array([[1, 0, 1, 1], [0, 1, 0, 1], [1, 0, 1, 0], [1, 1, 0, 1]], bool)
    np.testing.assert_array_equal(M, want)
    np.testing.assert_array_equal(pack_rows(M)[:, 0], np.array([13, 10, 5, 11], np.uint64))
    np.testing.assert_array_equal(pack_rows(M)[:, 1], np.zeros(4, np.uint64))
    # the threshold's values (neighbourhood_dev.h)
    assert [walk_max(n) for n in (2, 8, 9, 20, 32, 64, 65, 100, 128)] == [0, 0, 1, 4, 8, 19, 8, 14, 19]


def _pack_adj(adj):
    """acl_pack_adjacency's layout: bit j & 63 of word j >> 6 of row i."""
    n = adj.shape[0]
    W = (n + 63) // 64
    out = np.zeros((n, W), np.uint64)
    for j in range(n):
        out[:, j >> 6] |= (adj[:, j] != 0).astype(np.uint64) << np.uint64(j & 63)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_masks_bit_for_bit(cuda, n):
    import torch
    from aclswarm_amd import _lib as L
    rng = np.random.RandomState(9000 + n)
    gs = graphs(n, rng)
    P = perms(n, rng)
    bits = np.stack([_pack_adj(a) for _, a in gs for _ in range(B_PER_GRAPH)])
    P_all = np.concatenate([P] * len(gs))
    want = np.stack([pack_rows(model(a, p)) for _, a in gs for p in P])
    B = len(P_all)
    dev = torch.device("cuda:0")
    d_bits = torch.from_numpy(bits.view(np.int64)).to(dev)
    d_P = torch.from_numpy(P_all).to(dev)
    for mname, mode in MODES.items():
        out = torch.full((B, n, 2), -1, dtype=torch.int64, device=dev)
        rc = L.lib().acl_internal_neighbourhoods(n, B, ct.c_void_p(d_bits.data_ptr()),
                                                 ct.c_void_p(d_P.data_ptr()),
                                                 ct.c_void_p(out.data_ptr()), mode)
        assert rc == 0, (mname, rc)
        got = out.cpu().numpy().view(np.uint64)
        bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
        assert bad.size == 0, (mname, n, [(gs[b // B_PER_GRAPH][0], b % B_PER_GRAPH) for b in bad[:6]])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [20, 65, 100])
def test_solve_on_bridge_graphs(cuda, n):
    """acl_solve_batch on the path, two-clique and star formations against
    the CPU restatement: tables, assignments, flags and eff_rounds exact."""
    from test_gpu_parity import _compare, _gpu_solve, _oracle
    rng = np.random.RandomState(9100 + n)
    byname = dict(graphs(n, rng))
    adjs = [byname["path"], byname["two_cliques"], byname["star"]]
    F, B = len(adjs), 12
    pts = [np.c_[rng.uniform(-n, n, (n, 2)), rng.uniform(0, 2, n)] for _ in range(F)]
    gains = [H.synth_gains(rng, a, scale=1.0) for a in adjs]
    fidx = np.arange(B) % F
    q = np.stack([H.dense_positions(rng, n, 2.0 * n) for _ in range(B)])
    vel = rng.normal(0, 0.3, (B, n, 3))
    P_in = np.stack([H.random_perm(rng, n) for _ in range(B)])
    gpu = _gpu_solve(pts, adjs, gains, fidx, q, vel, P_in)
    ref = _oracle(pts, adjs, gains, fidx, q, vel, P_in)
    _compare(gpu, ref)
