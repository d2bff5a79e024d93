#!/usr/bin/env python3
"""Time of fleet localization on real links (acl_fleet_delay_localize_batch)
beside the existing entry, and of the closed loop on it
(acl_fleet_delay_est_episode_batch) beside acl_fleet_est_episode_batch.

Rounds: B swarms of n vehicles (fleet_auction_bench's formations, identity
rows) run `rounds` gossip rounds from fresh trackers, lossless, on
  existing  acl_fleet_localize_batch (the call's rounds stay in LDS);
  lat0      the new entry with every link at 0 rounds (max_table_latency 2):
            the same result, through the publication log;
  lat2      the new entry with every link at 2 rounds.
existing and lat0 must agree bit for bit.

Episodes: scripts/fleet_est_episode_bench.py's workload (noncomplete
formations, 5-plane gains, ticks_per_step 10, an auto-auction every 120 steps,
track_every 2, diag on) on acl_fleet_est_episode_batch, and on the new entry at
table latency 0 and 2; with the flights' records: err2 maxima, vehicles
adopted, collision-avoidance vehicle-steps.

All are timed wall-clock between synchronisations after a warm-up, alternated
in one session, medians reported. Writes one JSON document (--out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from aclswarm_amd import engine, workload  # noqa: E402
from fleet_auction_bench import make_case, timed  # noqa: E402

PATHS = (("existing", None), ("lat0", 0), ("lat2", 2))


def bench_rounds(n, B, F, rounds, reps, warmup, dev):
    T, adj, fidx, q = make_case(n, B, F, 1000 + n, dev)

    def one(lat):
        kw = {} if lat is None else dict(table_latency=lat, max_table_latency=2)
        loc = engine.FleetLocalization(T, fidx, **kw)  # fresh (not timed)
        if lat is not None:
            loc.run(0, q)  # (allocates the zero-filled log: not timed)
        dt, _ = timed(lambda: loc.run(rounds, q), dev)
        return dt, loc

    t = {k: [] for k, _ in PATHS}
    for r in range(warmup + reps):
        runs = {k: one(lat) for k, lat in PATHS}
        if r >= warmup:
            for k, (dt, _) in runs.items():
                t[k].append(dt)
    a, b = runs["existing"][1], runs["lat0"][1]
    assert bool((a.stamp == b.stamp).all()), "latency 0 and the existing entry disagree (stamp)"
    assert bool((a.est.view(torch.int64) == b.est.view(torch.int64)).all()), "... (est)"
    med = {k: statistics.median(v) for k, v in t.items()}
    out = dict(n=n, B=B, formations=F, rounds=rounds, d_max=int(adj.sum(axis=2).max()),
               lat0_equals_existing=True, log_bytes=int(b.loc_ws.numel()),
               log_traffic_bytes_per_round_and_swarm=2 * 28 * n * n)
    for k, _ in PATHS:
        st = runs[k][1].status()
        out[k] = dict(ms=med[k] * 1e3, us_per_round=med[k] * 1e6 / rounds,
                      ms_all=[x * 1e3 for x in t[k]], n_unknown_max=int(st["n_unknown"].max()),
                      max_age_max=int(st["max_age"].max()))
    out["lat0_over_existing"] = med["lat0"] / med["existing"]
    out["lat2_over_existing"] = med["lat2"] / med["existing"]
    return out


def bench_episode(n, B, F, steps, reps, warmup, track_every, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(500 + n)
    w = workload.simform_workload(B, n, gen, dev, F=F, complete=False, planes=5)
    T = engine.FormationTable(w["n"], w["p"], w["bits"], w["gains"], w["gain_off"], w["planes"])
    T.tile_gains()

    def one(lat):
        kw = {} if lat is None else dict(table_latency=lat, max_table_latency=2)
        fe = engine.FleetEstEpisode(T, w["fidx"], w["q"], w["vel"], track_every=track_every,
                                    diag=True, **kw)
        fe.run(0)  # (allocates the zero-filled workspace: not timed)
        return timed(lambda: fe.run(steps), dev)[0], fe

    t = {k: [] for k, _ in PATHS}
    for r in range(warmup + reps):
        runs = {k: one(lat) for k, lat in PATHS}
        if r >= warmup:
            for k, (dt, _) in runs.items():
                t[k].append(dt)
    a, b = runs["existing"][1], runs["lat0"][1]
    same = all(bool((getattr(a, k).view(torch.uint8) == getattr(b, k).view(torch.uint8)).all())
               for k in ("q", "vel", "loc_stamp", "loc_est", "xst"))
    assert same, "latency 0 and acl_fleet_est_episode_batch disagree"
    med = {k: statistics.median(v) for k, v in t.items()}
    out = dict(n=n, B=B, formations=F, steps=steps, track_every=track_every,
               lat0_equals_existing=True)
    for k, _ in PATHS:
        st = runs[k][1].status()
        x = st["estimates"]
        assert (st["fleet"]["flags"] == 0).all(), "a swarm overflowed or was refused"
        out[k] = dict(ms_per_step=med[k] / steps * 1e3, swarm_steps_per_s=B * steps / med[k],
                      s_all=t[k], vehicles_adopted=int(st["fleet"]["n_adopted"].sum()),
                      ca_vehicle_steps=int(st["episode"]["n_ca_steps"].sum()),
                      converged=int(st["episode"]["converged"].sum()),
                      n_unknown_max=int(x["n_unknown"].max()), max_age=int(x["max_age"].max()),
                      err_own_m=float(np.sqrt(x["err2_own"].max())),
                      err_nbr_m=float(np.sqrt(x["err2_nbr"].max())),
                      err_all_m=float(np.sqrt(x["err2_all"].max())))
    out["lat0_over_existing"] = med["lat0"] / med["existing"]
    out["lat2_over_existing"] = med["lat2"] / med["existing"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20x4096,100x256", help="n x B, comma-separated")
    ap.add_argument("--formations", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=64)
    ap.add_argument("--steps", type=int, default=240, help="0: no episodes")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--track-every", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_delay_localize",
                                                  "rounds.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res, eps = [], []
    for s in a.shapes.split(","):
        n, B = (int(x) for x in s.split("x"))
        r = bench_rounds(n, B, a.formations, a.rounds, a.reps, a.warmup, dev)
        print(json.dumps(r), flush=True)
        res.append(r)
        if a.steps > 0:
            r = bench_episode(n, B, a.formations, a.steps, max(a.reps // 2, 1), a.warmup,
                              a.track_every, dev)
            print(json.dumps(r), flush=True)
            eps.append(r)
    doc = dict(device=torch.cuda.get_device_name(dev), reps=a.reps, warmup=a.warmup,
               timing="wall clock between synchronisations, medians, paths alternated",
               rounds=res, episodes=eps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
