"""The CBAA column update of the fused solve (auction_kernel) against the CPU
restatement, on inputs built to reach each branch of the column body: the
peeled first level, the loop over the further levels, the tie and non-finite
exits to the exact ordered scan, vehicles left over after the last level, and
swarms that never agree.

Every (family, n) case runs acl_solve_batch with the decision margin on and
off (skip_margin) and with early_exit on and off; tables, assignments, flags,
round counts and margins are compared bit for bit, commands to the suite's
tolerance (test_gpu_parity._compare). n covers the 128-thread kernel with one
mask word (20), 256 threads (40), the last lane of word 0 (64), the first lane
of word 1 (65), the bench shape (100) and the last / full lanes of word 1
(127, 128).

The tests without the gpu mark assert, on the oracle alone, that each
construction still reaches its edge, so the GPU comparison cannot weaken
unnoticed."""
import copy

import numpy as np
import pytest

import helpers as H
import pyoracle as O

NS = [20, 40, 64, 65, 100, 127, 128]
FAMILIES = ["one_missing", "ring", "path", "star", "two_components", "ties", "nan_prices"]
B = 4  # swarms per case

FLAG_AGREE, FLAG_NONFINITE, FLAG_CA_ACTIVE, FLAG_FRAGILE = 0x02, 0x08, 0x20, 0x40


def _sym(a):
    a = np.maximum(a, a.T)
    np.fill_diagonal(a, 0)
    return a.astype(np.uint8)


def _graph(family, rng, n):
    a = np.zeros((n, n), np.uint8)
    if family in ("one_missing", "nan_prices"):
        # complete minus one random neighbour per row (the bench config's shape)
        a[:] = 1
        for i in range(n):
            j = (i + 1 + rng.randint(0, n - 1)) % n
            a[i, j] = a[j, i] = 0
    elif family in ("ring", "path"):
        i = np.arange(n - 1)
        a[i, i + 1] = 1
        if family == "ring":
            a[n - 1, 0] = 1
    elif family == "star":
        a[0, :] = 1
    elif family == "two_components":
        h = n // 2
        a[:h, :h] = 1
        a[h:, h:] = 1
    elif family == "ties":
        # twin pairs (2k, 2k + 1): adjacent, with one closed neighbourhood, so
        # both run one alignment; pairs joined at random, connected by a ring
        m = n // 2
        g = rng.rand(m, m) < 0.6
        k = np.arange(m)
        g[k, (k + 1) % m] = True
        g = g | g.T | np.eye(m, dtype=bool)
        a[:2 * m, :2 * m] = np.kron(g, np.ones((2, 2), np.uint8))
        if n % 2:
            a[n - 1, :] = 1
    return _sym(a)


def _lattice(rng, n, side):
    """n distinct points on the quarter-unit lattice (dyadic coordinates)."""
    cells = int(side * 4)
    idx = rng.choice(cells * cells, n, replace=False)
    return np.c_[(idx // cells) / 4.0, (idx % cells) / 4.0, np.full(n, 1.0)]


def _force_tie(q, p, adj, P_in):
    """Move one vehicle w (in place) so that its START bid goes to the task of
    a non-adjacent, lower vehicle v at v's price, bit for bit in f32: w is
    put at v's distance from its own aligned image of the task, then the
    distance is bisected until the oracle's f32 price of w equals v's (a
    float price spans ~2^28 doubles of the distance). v is not in w's closed
    neighbourhood, so v's alignment and prices do not move. A vehicle that
    sees w and not v (w itself) then takes w in the ordered scan, where the
    first holder's `who` would be v."""
    n = q.shape[0]
    C, Rt = O.prices(q, p, adj, P_in)
    for v in range(n):
        j = int(C[v].argmax())
        target = C[v, j]
        if not target > 0:
            continue
        for w in range(n - 1, v, -1):
            if adj[v, w] or (q == q[w]).all(1).sum() > 1 or (q == q[v]).all(1).sum() > 1:
                continue
            d = 1.0 / float(target) - 1e-8
            q0 = q[w].copy()
            # w's alignment row (P_in as vehicle -> point or its inverse)
            r = [x for x in {w, int(P_in[w]), int(np.flatnonzero(P_in == w)[0])}
                 if np.array_equal(_price_rows(q[[w]], p, Rt[[x]])[0], C[w])][0]
            for _ in range(3):  # the image of task j moves with w: fixed-point steps
                Rw = O.prices(q, p, adj, P_in)[1][r]
                a = np.array([(Rw[0] * p[j, 0] + Rw[1] * p[j, 1]) + Rw[4],
                              (Rw[2] * p[j, 0] + Rw[3] * p[j, 1]) + Rw[5], p[j, 2]])
                q[w] = a + np.array([d, 0.0, 0.0])
            lo, hi = 0.5 * d, 2.0 * d
            for _ in range(100):
                mid = 0.5 * (lo + hi)
                q[w] = a + np.array([mid, 0.0, 0.0])
                Cw = O.prices(q, p, adj, P_in)[0]
                if Cw[w, j] == target:
                    break
                if Cw[w, j] > target:
                    lo = mid
                else:
                    hi = mid
            if (Cw[w, j] == target and int(Cw[w].argmax()) == j
                    and np.array_equal(Cw[v], C[v])):
                return v, w
            q[w] = q0
    raise AssertionError("no tie constructed")


_cases = {}


def _inputs(family, n):
    """(points, adjs, gains, fidx, q, vel, P_in) of a case, built once."""
    key = (family, n)
    if key in _cases:
        return _cases[key]
    rng = np.random.RandomState(8000 + 131 * FAMILIES.index(family) + n)
    side = 4.5 * np.sqrt(n)
    adj = _graph(family, rng, n)
    vel = rng.normal(0, 0.2, (B, n, 3))
    if family == "ties":
        p = _lattice(rng, n, side)
        q = np.stack([_lattice(rng, n, side) for _ in range(B)])
        # identity, or twins swapped: twin vehicles hold twin points either way
        P_in = np.tile(np.arange(n, dtype=np.uint16), (B, 1))
        for b in range(1, B):
            for k in range(n // 2):
                if rng.rand() < 0.5:
                    P_in[b, [2 * k, 2 * k + 1]] = P_in[b, [2 * k + 1, 2 * k]]
        # some twin vehicles share one position: one alignment, one position,
        # so their whole price rows are equal bit for bit
        for b in range(B):
            for k in rng.choice(n // 2, max(2, n // 8), replace=False):
                q[b, 2 * k + 1] = q[b, 2 * k]
            _force_tie(q[b], p, adj, P_in[b])
    else:
        p = H.random_positions(rng, n, side)
        q = np.stack([H.random_positions(rng, n, side) for _ in range(B)])
        P_in = np.stack([H.random_perm(rng, n) if b % 2 else np.arange(n, dtype=np.uint16)
                         for b in range(B)])
    if family == "nan_prices":
        p[n // 3, 0] = np.inf  # one non-finite formation coordinate
    gains = H.synth_gains(rng, adj)
    _cases[key] = ([p], [adj], [gains], np.zeros(B, np.int32), q, vel, P_in)
    return _cases[key]


def _price_rows(q, p, Rt):
    """Price rows restated in numpy from alignments (R00, R01, R10, R11, t0,
    t1): the aligned point [R 0; 0 1] p + [t; 0] in f64, the squared distance
    summed as (dx^2 + dy^2) + dz^2, the price 1 / (sqrt(d2) + 1e-8) rounded to
    f32 (getPrice). Row k: the vehicle at q[k] under alignment Rt[k]."""
    ax = (Rt[:, None, 0] * p[None, :, 0] + Rt[:, None, 1] * p[None, :, 1]) + Rt[:, None, 4]
    ay = (Rt[:, None, 2] * p[None, :, 0] + Rt[:, None, 3] * p[None, :, 1]) + Rt[:, None, 5]
    dx, dy, dz = q[:, None, 0] - ax, q[:, None, 1] - ay, q[:, None, 2] - p[None, :, 2]
    return (1.0 / (np.sqrt((dx * dx + dy * dy) + dz * dz) + 1e-8)).astype(np.float32)


_refs = {}


def _reference(family, n, early_exit):
    """The oracle's outputs of a case, computed once and shared, never modified."""
    key = (family, n, early_exit)
    if key not in _refs:
        pts, adjs, gains, fidx, q, vel, P_in = _inputs(family, n)
        _refs[key] = [O.solve(q[b], vel[b], pts[0], adjs[0], gains[0], P_in[b],
                              early_exit=early_exit) for b in range(B)]
    return _refs[key]


def _expected(ref, margin, control):
    """The reference as a call without the margin / without the control stage
    reports it: margin -1 and FRAGILE clear under skip_margin (test_gpu_fused.
    test_skip_margin_same_outcome); CA_ACTIVE clear when no control ran."""
    out = copy.deepcopy(ref)
    for r in out:
        fl = int(r["status"]["flags"])
        if not margin:
            fl &= ~FLAG_FRAGILE
            r["status"]["margin"] = -1.0
        if not control:
            fl &= ~FLAG_CA_ACTIVE
        r["status"]["flags"] = fl
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("family", FAMILIES)
def test_columns_vs_oracle(cuda, family, n):
    from test_gpu_parity import _compare, _gpu_solve
    args = _inputs(family, n)
    # a non-finite formation point makes the commands NaN on both sides: the
    # auction alone is compared there (as test_gpu_parity does)
    control = family != "nan_prices"
    for early in (True, False):
        ref = _reference(family, n, early)
        for margin in (True, False):
            gpu = _gpu_solve(*args, early_exit=early, do_control=control, margin=margin)
            _compare(gpu, _expected(ref, margin, control), check_control=control)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("family", ["ring", "path"])
def test_sparse_graphs_leave_vehicles_to_the_scan(family, n):
    """Closed neighbourhoods of at most 3 vehicles: the levels of a contested
    column resolve a few vehicles only; consensus takes many rounds."""
    adj = _inputs(family, n)[1][0]
    assert (adj.sum(1) + 1).max() == 3
    ref = _reference(family, n, True)
    assert max(int(r["status"]["eff_rounds"]) for r in ref) > n / 4


@pytest.mark.parametrize("n", NS)
def test_star_has_one_hub(n):
    adj = _inputs("star", n)[1][0]
    deg = adj.sum(1)
    assert deg[0] == n - 1 and (deg[1:] == 1).all()


@pytest.mark.parametrize("n", NS)
def test_one_missing_rows_miss_a_neighbour(n):
    for family in ("one_missing", "nan_prices"):
        adj = _inputs(family, n)[1][0]
        assert (adj.sum(1) <= n - 2).all() and adj.sum(1).min() >= n - 1 - 8


@pytest.mark.parametrize("n", NS)
def test_two_components_do_not_agree(n):
    ref = _reference("two_components", n, True)
    assert all(not (int(r["status"]["flags"]) & FLAG_AGREE) for r in ref)


@pytest.mark.parametrize("n", NS)
def test_nan_prices_set_nonfinite(n):
    ref = _reference("nan_prices", n, True)
    assert all(int(r["status"]["flags"]) & FLAG_NONFINITE for r in ref)




@pytest.mark.parametrize("n", NS)
def test_ties_hold_equal_prices_under_two_holders(n):
    """Every swarm of the ties family has two vehicles that are not adjacent
    and whose START bids (each row's first largest price) go to one task at
    bit-equal f32 prices: that column's top level is held under two `who`s
    in round 1, and the higher of the two sees itself and not the other. The
    two price rows are recomputed in numpy from the oracle's alignments with
    getPrice's expression and an f32 rounding, and must be the oracle's."""
    pts, adjs, gains, fidx, q, vel, P_in = _inputs("ties", n)
    for b in range(B):
        C, Rt = O.prices(q[b], pts[0], adjs[0], P_in[b])
        assert C.dtype == np.float32 and np.isfinite(C).all()
        best = C.argmax(1)  # the first of the largest
        top = C[np.arange(n), best]
        tied = [(v, w) for v in range(n) for w in range(v + 1, n)
                if best[v] == best[w] and top[v] > 0 and not adjs[0][v, w]
                and top[v].view(np.uint32) == top[w].view(np.uint32)]
        assert tied, (n, b)
        for v, w in tied:
            rows = []
            for x in (v, w):  # the alignment that gives the oracle's row of x
                mine = [r for r in range(n) if np.array_equal(
                    _price_rows(q[b][[x]], pts[0], Rt[[r]])[0].view(np.uint32),
                    C[x].view(np.uint32))]
                assert mine, (n, b, x)
                rows.append(_price_rows(q[b][[x]], pts[0], Rt[[mine[0]]])[0])
            j = best[v]
            assert rows[0][j].view(np.uint32) == rows[1][j].view(np.uint32)
            assert rows[0].argmax() == j and rows[1].argmax() == j
