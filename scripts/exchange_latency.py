#!/usr/bin/env python3
"""Per-tally latency of the facade's bid-exchange mode (ABI 11): fleets of
exchange-mode Auctioneers (tests/facade_driver.cpp facade_exchange) on one
bus, every completed bid iteration tallied on the GPU by
acl_cbaa_step_batch (V = 1, host-synchronous). The reference's vehicles tick
their Auctioneer every 1 ms (coordination_ros.cpp:146-153); one tally here
must fit well inside that. Prints one JSON line per fleet size, then the
latency of one start() on its own (tests/facade_start_driver.cpp
facade_start_latency: flush(); start(q) repeated, a host clock around each
start, which ends in the facade's own synchronise).

Usage (GPU box): python scripts/exchange_latency.py
       --starts-only --start-driver PATH --label NAME   another build of the
       same driver source (an A/B against an older library), starts alone
"""
import argparse
import ctypes as ct
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers as H  # noqa: E402

LIB = os.path.join(ROOT, "aclswarm_amd", "lib", "libfacade_driver.so")
START_LIB = os.path.join(ROOT, "aclswarm_amd", "lib", "libfacade_start_driver.so")


def run(name, idx, seed):
    Pf, Af = H.simform(name)
    p, adj = Pf[idx, 0], Af[idx]
    n = p.shape[0]
    rng = np.random.RandomState(seed)
    q = H.random_positions(rng, n, 20.0 if n <= 20 else 45.0)
    P_in = H.random_perm(rng, n).astype(np.uint8)
    lib = ct.CDLL(LIB)
    f = lib.facade_exchange
    f.restype = ct.c_int
    f.argtypes = [ct.c_int] + [ct.c_void_p] * 4 + [ct.c_uint32, ct.c_int] + [ct.c_void_p] * 6
    outs = [np.zeros((n, n), np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.int32),
            np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, n), np.int32)]
    ins = [np.asfortranarray(p, np.float64), np.asfortranarray(np.asarray(adj, np.uint8)),
           np.asfortranarray(q, np.float64), np.ascontiguousarray(P_in)]
    ptr = lambda a: a.ctypes.data_as(ct.c_void_p)  # noqa: E731
    t0 = time.perf_counter()
    rc = f(n, *[ptr(a) for a in ins], seed, 0, *[ptr(a) for a in outs])
    dt = time.perf_counter() - t0
    assert rc == 0
    tallies = n * (2 * n + 1)  # each vehicle: its START bid and 2n iterations
    starts = n                 # each start() is one acl_vehicle_start_batch launch (V = 1)
    return dict(fleet=name, n=n, seconds=dt, tallies=tallies, starts=starts,
                us_per_tally_incl_starts=1e6 * dt / tallies)


def start_only(name, idx, seed, lib_path=START_LIB, label="tree", warm=20, reps=200):
    """One exchange-mode vehicle's start() on its own: microseconds per call."""
    Pf, Af = H.simform(name)
    p, adj = Pf[idx, 0], Af[idx]
    n = p.shape[0]
    rng = np.random.RandomState(seed)
    q = H.random_positions(rng, n, 20.0 if n <= 20 else 45.0)
    lib = ct.CDLL(lib_path)
    f = lib.facade_start_latency
    f.restype = ct.c_int
    f.argtypes = [ct.c_int] + [ct.c_void_p] * 3 + [ct.c_int, ct.c_int, ct.c_void_p]
    ins = [np.asfortranarray(p, np.float64), np.asfortranarray(np.asarray(adj, np.uint8)),
           np.asfortranarray(q, np.float64)]
    us = np.zeros(reps)
    rc = f(n, *[a.ctypes.data_as(ct.c_void_p) for a in ins], warm, reps,
           us.ctypes.data_as(ct.c_void_p))
    assert rc == 0
    return dict(start_only=name, build=label, n=n, reps=reps, us_median=float(np.median(us)),
                us_p10=float(np.percentile(us, 10)), us_p90=float(np.percentile(us, 90)),
                us_min=float(us.min()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--starts-only", action="store_true")
    ap.add_argument("--start-driver", default=START_LIB)
    ap.add_argument("--label", default="tree")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    if not args.starts_only:
        run("simform20_nc", 0, 1)  # warm-up (module load, first launches)
        for name, idx, seed in (("simform20_nc", 1, 2), ("simform20_fc", 2, 3),
                                ("simform100_nc", 0, 4)):
            print(json.dumps(run(name, idx, seed)), flush=True)
    for name, idx, seed in (("simform20_nc", 1, 2), ("simform100_nc", 0, 4)):
        print(json.dumps(start_only(name, idx, seed, args.start_driver, args.label)), flush=True)


if __name__ == "__main__":
    main()
