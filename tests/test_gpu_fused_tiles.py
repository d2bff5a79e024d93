"""GPU: the fused control phase's packed edge tiles (csrc/pair_fused.h). Where
n mod 8 is 1 to 4 and there are at least three row blocks, the half-empty
8x8 tiles of the last column block run two to a tile; the sizes below have
last-block widths 1 and 4, odd and even numbers of edge tiles, two row blocks
(nothing packs) and, as controls, sizes where no packing applies.

Checked against the CPU restatement (commands 1e-5 relative), against
acl_control_batch on the same assignments (the same terms in another
summation order: 1e-12) and for bit-identical repeats in either batch order."""
import numpy as np
import pytest

import helpers as H
from test_gpu_parity import _compare, _gpu_solve, _oracle

pytestmark = pytest.mark.gpu

PACKED = [9, 12, 17, 20, 25, 97, 100, 124]
CONTROLS = [13, 16, 24]


def _formations(rng, n):
    near = np.ones((n, n), np.uint8) - np.eye(n, dtype=np.uint8)
    for _ in range(max(1, n // 3)):
        i, j = rng.randint(0, n, 2)
        if i != j:
            near[i, j] = near[j, i] = 0
    sparse = np.triu(rng.uniform(size=(n, n)) < 0.3, 1)
    sparse = (sparse | sparse.T).astype(np.uint8)
    full = np.ones((n, n), np.uint8) - np.eye(n, dtype=np.uint8)
    adjs = [near, sparse, full]
    pts = [np.c_[rng.uniform(-n, n, (n, 2)), rng.uniform(0, 2, n)] for _ in adjs]
    gains = [H.synth_gains(rng, a, scale=1.0) for a in adjs]
    return pts, adjs, gains


@pytest.mark.parametrize("n", PACKED + CONTROLS)
def test_packed_tiles(cuda, n):
    import torch
    from aclswarm_amd import engine
    rng = np.random.RandomState(7000 + n)
    F, B = 3, 12
    pts, adjs, gains = _formations(rng, n)
    fidx = np.arange(B) % F
    q = np.stack([H.dense_positions(rng, n, 2.0 * n) for _ in range(B)])
    q[::3, :, :2] *= 0.3  # crowded: collision candidates in every tile, the packed ones too
    vel = rng.normal(0, 0.3, (B, n, 3))
    P_in = np.stack([H.random_perm(rng, n) for _ in range(B)])
    gpu = _gpu_solve(pts, adjs, gains, fidx, q, vel, P_in)
    _compare(gpu, _oracle(pts, adjs, gains, fidx, q, vel, P_in))

    # uniform swarms: the fused phase against the stand-alone pair kernel
    dev = torch.device("cuda:0")
    T = engine.FormationTable.from_host(pts, adjs, gains, device=dev, planes=5)
    uni = [b for b in range(B) if gpu["status"]["flags"][b] & 0x3 == 0x3]
    assert uni
    P = torch.from_numpy(gpu["P_out"][uni].view(np.int16)).to(dev)
    out = engine.control(T, torch.from_numpy(fidx[uni].astype(np.int32)).to(dev),
                         torch.from_numpy(q[uni]).to(dev), torch.from_numpy(vel[uni]).to(dev), P,
                         want_gate_margin=True)
    torch.cuda.synchronize()
    c = {k: v.cpu().numpy() for k, v in out.items()}
    np.testing.assert_array_equal(c["ca_flag"], gpu["ca_flag"][uni])
    for k in ("u", "u_safe"):
        np.testing.assert_allclose(c[k], gpu[k][uni], rtol=1e-12, atol=1e-12, err_msg=k)
    np.testing.assert_array_equal(c["gate_margin"], gpu["gate_margin"][uni])

    # two runs and a reversed batch: bit-identical
    again = _gpu_solve(pts, adjs, gains, fidx, q, vel, P_in)
    rev = _gpu_solve(pts, adjs, gains, fidx[::-1].copy(), q[::-1].copy(), vel[::-1].copy(),
                     P_in[::-1].copy())
    for k in ("P_out", "u", "u_safe", "ca_flag", "who", "gate_margin"):
        np.testing.assert_array_equal(gpu[k], again[k], err_msg=k)
        np.testing.assert_array_equal(gpu[k], rev[k][::-1], err_msg=k)
