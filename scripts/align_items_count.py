#!/usr/bin/env python3
"""Alignment work items per swarm at config C3, and what pooling them buys.

An item is a formation row whose closed neighbourhood is incomplete, plus one
item for all complete rows (align_worklist, csrc/auction.hip). The alignment
launch walks all n members twice per chunk of 64 items whatever the number of
active lanes, so its vector work goes with the chunk passes. This script
counts, for the benchmark's formations (seeds 0 .. B-1, each swarm its own):

  * the items histogram,
  * chunk passes per swarm and lane use with one wave per swarm,
  * the same with the items of S consecutive swarms pooled into shared chunks.

Adjacency source: workload.reference_formations on the device (--device), or
the same draws on the CPU (default): the graph is the first thing the
reference generator draws after np.random.seed(s) -- m = randint(1, n - 3),
rows = choice(n, m), cols = choice(n, m) (generate_random_formation.py:61-72)
-- so numpy's own legacy stream gives the identical adjacency without the
points. --check N compares the two sources on the first N seeds.

Usage: python scripts/align_items_count.py [--n 100] [--B 65536] [--device]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def items_of(adj):
    """adj [n][n] bool (no diagonal): the work item count."""
    n = adj.shape[0]
    ninc = int(((adj.sum(1) + 1) < n).sum())
    return ninc + (1 if ninc < n else 0)


def adjacency_numpy(seed, n):
    np.random.seed(seed)
    adj = np.ones((n, n), bool) & ~np.eye(n, dtype=bool)
    m = np.random.randint(1, n - 4 + 1)
    rows = np.random.choice(n, size=(m,))
    cols = np.random.choice(n, size=(m,))
    adj[rows, cols] = False
    adj[cols, rows] = False
    return adj


def counts_numpy(n, B, seed0=0):
    return np.array([items_of(adjacency_numpy(seed0 + s, n)) for s in range(B)])


def counts_device(n, B, L, seed0=0, step=8192):
    import torch
    from aclswarm_amd import workload
    dev = torch.device("cuda:0")
    out = []
    for s0 in range(0, B, step):
        _, adj = workload.reference_formations(min(step, B - s0), n, L, False, seed0 + s0, dev)
        ninc = ((adj.sum(2) + 1) < n).sum(1)
        out.append((ninc + (ninc < n).to(ninc.dtype)).cpu().numpy())
    return np.concatenate(out)


def pooled(c, S):
    """Chunk passes when S consecutive swarms share their chunks."""
    pad = (-len(c)) % S
    g = np.r_[c, np.zeros(pad, c.dtype)].reshape(-1, S).sum(1)
    return int(((g + 63) // 64).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--L", type=float, default=40.0)
    ap.add_argument("--device", action="store_true", help="adjacency from the device generator")
    ap.add_argument("--check", type=int, default=0, metavar="N",
                    help="compare the CPU draws with the device generator on N seeds")
    a = ap.parse_args()
    if a.check:
        cd, cn = counts_device(a.n, a.check, a.L), counts_numpy(a.n, a.check)
        print(f"device generator vs numpy draws, {a.check} seeds: "
              f"{'identical' if (cd == cn).all() else 'DIFFERENT'}")
        if not (cd == cn).all():
            return 1
    c = counts_device(a.n, a.B, a.L) if a.device else counts_numpy(a.n, a.B)
    B = len(c)
    print(f"n = {a.n}, B = {B}, adjacency from {'the device generator' if a.device else 'numpy draws'}")
    pc = np.percentile(c, [5, 25, 50, 75, 95])
    print(f"items per swarm: mean {c.mean():.1f}, min {c.min()}, max {c.max()}; "
          f"percentiles 5/25/50/75/95 = {' / '.join(f'{x:.0f}' for x in pc)}")
    over = c > 64
    print(f"swarms with more than 64 items: {100.0 * over.mean():.1f} % "
          f"(median {np.median(c[over] - 64) if over.any() else 0:.0f} extra items)")
    print("histogram (items: swarms):")
    edges = list(range(0, a.n + 1, 8))
    h, _ = np.histogram(c, bins=edges + [a.n + 1])
    for lo, k in zip(edges, h):
        print(f"  {lo:3d}-{min(lo + 7, a.n):3d}: {k}")
    now = int(((c + 63) // 64).sum())
    total = int(c.sum())
    print(f"one wave per swarm: {now / B:.3f} chunk passes per swarm, lane use "
          f"{100.0 * total / (64 * now):.0f} %")
    print("| S | chunk passes per swarm | ratio to now | lane use |")
    print("|---|---|---|---|")
    for S in (2, 4, 8, 16, 32):
        p = pooled(c, S)
        print(f"| {S} | {p / B:.3f} | {p / now:.3f} | {100.0 * total / (64 * p):.0f} % |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
