"""GPU: the tile loops of the fused control phase (csrc/pair_fused.h) on the
paths a lean common path could lose: the body for swarms whose q is finite
and the general one side by side in a batch, the wave votes that send a tile
to the guarded square roots (an argument of exactly 0 or +inf) and to the
atan's infinite-argument result, in regular and in packed tiles, and the
tile shapes n = 9 (two row blocks, no packed tile), 20 (one packed tile of
two row blocks), 28 (the odd packed tile with its upper half masked), 65 (the
second mask word, four packed tiles) and 100.

Against the CPU restatement with the comparisons of
tests/test_gpu_fused.py::test_fused_solve_vs_oracle_and_control: tables,
assignments, status, gates and collision flags exact, u / u_safe 1e-5
relative, and the pattern of non-finite entries of u / u_safe exact. Every
swarm has a formation of its own."""
import numpy as np
import pytest

import helpers as H
import pyoracle as O
from test_gpu_parity import U_RTOL, _compare, _gpu_solve

NS = [9, 20, 28, 65, 100]
B = 6
NAN_SWARM, INF_SWARM = 2, 4  # in the middle of an otherwise finite batch
OUT_KEYS = ("who", "P_out", "u", "u_safe", "ca_flag", "gate_margin")


def _graph(rng, n):
    """Complete minus one random neighbour per row (the bench's shape)."""
    a = np.ones((n, n), np.uint8)
    for i in range(n):
        j = (i + 1 + rng.randint(0, n - 1)) % n
        a[i, j] = a[j, i] = 0
    np.fill_diagonal(a, 0)
    return a


def _complete(n):
    return np.ones((n, n), np.uint8) - np.eye(n, dtype=np.uint8)


def _batch(seed, n, complete):
    """B swarms, each with its own formation points, graph and gains."""
    rng = np.random.RandomState(seed)
    side = 4.5 * np.sqrt(n)
    pts = [np.c_[H.random_positions(rng, n, side)[:, :2], rng.uniform(0.5, 2.5, n)]
           for _ in range(B)]
    adjs = [_complete(n) if complete else _graph(rng, n) for _ in range(B)]
    gains = [H.synth_gains(rng, a) for a in adjs]
    q = np.stack([np.c_[H.random_positions(rng, n, side)[:, :2], rng.uniform(0.5, 2.5, n)]
                  for _ in range(B)])
    vel = rng.normal(0, 0.2, (B, n, 3))
    P_in = np.stack([H.random_perm(rng, n) if b % 2 else np.arange(n, dtype=np.uint16)
                     for b in range(B)])
    return pts, adjs, gains, np.arange(B, dtype=np.int32), q, vel, P_in


def _solve_ref(args, b):
    pts, adjs, gains, fidx, q, vel, P_in = args
    return O.solve(q[b], vel[b], pts[b], adjs[b], gains[b], P_in[b])


_cache = {}


def _once(key, make):
    """Inputs and references are built once, shared and never modified."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _finite(n):
    return _once(("finite", n), lambda: _batch(7100 + n, n, complete=False))


def _finite_ref(n):
    return _once(("finite_ref", n), lambda: [_solve_ref(_finite(n), b) for b in range(B)])


def _nonfinite(n):
    def make():
        pts, adjs, gains, fidx, q, vel, P_in = _finite(n)
        q = q.copy()
        q[NAN_SWARM, n // 2, 1] = np.nan
        q[INF_SWARM, n // 3, 0] = np.inf
        return pts, adjs, gains, fidx, q, vel, P_in
    return _once(("nonfinite", n), make)


def _nonfinite_ref(n):
    return _once(("nonfinite_ref", n),
                 lambda: {b: _solve_ref(_nonfinite(n), b) for b in (NAN_SWARM, INF_SWARM)})


def _rows_of(ref, v1, v2):
    """Formation rows of two vehicles after the solve, smaller first."""
    r = sorted((int(ref["P_out"][v1]), int(ref["P_out"][v2])))
    return r[0], r[1]


# the guard batch's swarms (complete graphs: every pair is an edge)
G_PLAIN, G_Z_REG, G_Z_PACK, G_XY_REG, G_XY_PACK, G_HUGE = range(6)


def _guards(n):
    """Swarms whose special pair is one lane of its tile: two formation points
    with equal z (the Gram expression of the z distance is exactly 0), two
    vehicles with equal xy (s2 = 0; they are then within the avoidance
    threshold too), each once in a regular tile and once in a packed one (a
    column of the last column block, rows of an earlier row block), and one
    vehicle at x = 1e200 (finite, s2 = +inf for its whole row and column)."""
    def make():
        pts, adjs, gains, fidx, q, vel, P_in = _batch(7300 + n, n, complete=True)
        pts = [p.copy() for p in pts]
        q = q.copy()
        last = 8 * ((n + 7) // 8 - 1)  # first column of the last column block
        pts[G_Z_REG][11, 2] = pts[G_Z_REG][2, 2]
        pts[G_Z_PACK][last + 1, 2] = pts[G_Z_PACK][3, 2]
        where = {}
        for b, packed in ((G_XY_REG, False), (G_XY_PACK, True)):
            # the pair's rows follow from the assignment: take the first pair
            # of vehicles whose rows land where the case wants them
            for v1, v2 in ((v1, v2) for v1 in range(n) for v2 in range(v1 + 1, n)):
                keep = q[b, v2].copy()
                q[b, v2, :2] = q[b, v1, :2]
                i, j = _rows_of(_solve_ref((pts, adjs, gains, fidx, q, vel, P_in), b), v1, v2)
                if (j >= last and i < last - 8) if packed else (j < last and j - i >= 8):
                    where[b] = (i, j)
                    break
                q[b, v2] = keep
            assert b in where
        q[G_HUGE, n // 2, 0] = 1e200
        return (pts, adjs, gains, fidx, q, vel, P_in), where
    return _once(("guards", n), make)


def _guards_ref(n):
    return _once(("guards_ref", n), lambda: [_solve_ref(_guards(n)[0], b) for b in range(B)])


def _compare_control(gpu, refs, swarms):
    """_compare's control checks, for outputs that may hold non-finite
    entries: the same entries NaN, the same entries infinite with the same
    sign, every other entry within U_RTOL."""
    for b in swarms:
        r = refs[b]
        gm, rg = float(gpu["gate_margin"][b]), r["gate_margin"]
        if np.isfinite(rg):
            assert abs(gm - rg) <= 1e-10, (b, gm, rg)
        else:
            assert gm == rg or (np.isnan(gm) and np.isnan(rg)), (b, gm, rg)
        assert int(gpu["status"][b]["n_ca"]) == int(r["status"]["n_ca"]), b
        np.testing.assert_array_equal(gpu["ca_flag"][b], r["ca"], err_msg=f"ca swarm {b}")
        for key in ("u", "u_safe"):
            g, x = gpu[key][b], r[key]
            np.testing.assert_array_equal(np.isnan(g), np.isnan(x), err_msg=f"{key} NaN swarm {b}")
            inf = np.isinf(x)
            np.testing.assert_array_equal(np.isinf(g), inf, err_msg=f"{key} inf swarm {b}")
            np.testing.assert_array_equal(g[inf], x[inf], err_msg=f"{key} inf sign swarm {b}")
            fin = np.isfinite(x)
            err = np.abs(g[fin] - x[fin]) / np.maximum(np.abs(x[fin]), 1.0)
            assert err.size == 0 or err.max() <= U_RTOL, (b, key, err.max())


def _bits_equal(a, b, swarms, what):
    for k in OUT_KEYS:
        np.testing.assert_array_equal(a[k][swarms].view(np.uint8), b[k][swarms].view(np.uint8),
                                      err_msg=f"{what}: {k}")
    np.testing.assert_array_equal(a["status"][swarms].view(np.uint8),
                                  b["status"][swarms].view(np.uint8), err_msg=f"{what}: status")


@pytest.mark.parametrize("n", NS)
def test_oracle_is_defined_where_the_tests_expect_it(n):
    """CPU: the reference is finite for the finite batch, for the equal-z and
    the equal-xy swarms and for every vehicle of the 1e200 swarm's u (its
    commands are of the order of 1e200, not infinite); the non-finite swarms'
    references do hold NaN; the special pairs sit where the cases want them."""
    for r in _finite_ref(n):
        assert np.isfinite(r["u"]).all() and np.isfinite(r["u_safe"]).all()
    for b, r in _nonfinite_ref(n).items():
        assert np.isnan(r["u"]).any(), b
    if n not in (20, 100):  # the guard cases' sizes
        return
    (pts, adjs, gains, fidx, q, vel, P_in), where = _guards(n)
    refs = _guards_ref(n)
    last = 8 * ((n + 7) // 8 - 1)
    assert pts[G_Z_REG][2, 2] == pts[G_Z_REG][11, 2]
    assert pts[G_Z_PACK][3, 2] == pts[G_Z_PACK][last + 1, 2]
    assert where[G_XY_REG][1] < last <= where[G_XY_PACK][1]
    for b in (G_PLAIN, G_Z_REG, G_Z_PACK, G_XY_REG, G_XY_PACK):
        assert np.isfinite(refs[b]["u"]).all() and np.isfinite(refs[b]["u_safe"]).all(), b
    for b in (G_XY_REG, G_XY_PACK):  # the coincident pair is a collision pair
        assert int(refs[b]["status"]["flags"]) & 0x20 and int(refs[b]["status"]["n_ca"]) >= 1, b
    assert np.isfinite(refs[G_HUGE]["u"]).all()
    assert np.abs(refs[G_HUGE]["u"]).max() > 1e150


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_finite_body_vs_oracle_and_twice(cuda, n):
    """Finite q: the specialised body; the same inputs twice, bit-equal."""
    args = _finite(n)
    a = _gpu_solve(*args)
    _compare(a, _finite_ref(n))
    b = _gpu_solve(*args)
    _bits_equal(a, b, np.arange(B), "second run")


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_nonfinite_swarms_in_a_finite_batch(cuda, n):
    """A NaN in one swarm's q and +inf in another's: those two match the
    reference, the NaN entries of u included; every other swarm of the batch
    is bit-equal to the same batch run without them."""
    base = _gpu_solve(*_finite(n))
    gpu = _gpu_solve(*_nonfinite(n))
    refs = _nonfinite_ref(n)
    special = sorted(refs)
    _compare({k: v[special] for k, v in gpu.items()}, [refs[b] for b in special],
             check_control=False)
    _compare_control(gpu, refs, special)
    others = np.array([b for b in range(B) if b not in refs])
    _bits_equal(gpu, base, others, "finite swarms beside the non-finite ones")
    for b in special:
        assert np.isnan(gpu["u"][b]).any(), b


@pytest.mark.gpu
@pytest.mark.parametrize("n", [20, 100])
def test_guard_fallback_in_regular_and_packed_tiles(cuda, n):
    """One special lane carries its wave through the guarded form."""
    args, _ = _guards(n)
    gpu = _gpu_solve(*args)
    refs = _guards_ref(n)
    _compare(gpu, refs, check_control=False)
    _compare_control(gpu, refs, range(B))
    again = _gpu_solve(*args)
    _bits_equal(gpu, again, np.arange(B), "second run")
