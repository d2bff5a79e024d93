#!/usr/bin/env python3
"""Step time of the episodes on each vehicle's own estimates
(acl_fleet_est_episode_batch, engine.FleetEstEpisode) beside the
shared-snapshot episodes with the same links (acl_fleet_lossy_episode_batch,
engine.FleetEpisode with latency 1 and loss 0) on the same swarms.

The shapes and the workload are scripts/fleet_episode_bench.py's: B swarms of n
vehicles on noncomplete formations of the reference generator, 5-plane gains,
ticks_per_step 10, an auto-auction every 120 steps, 240 steps from fresh
state; every link at 1 tick, loss 0, track_every 2. Three loops are alternated
in one session -- the lossy entry, the new entry with diag off, the new entry
with diag on -- timed wall-clock between synchronisations after a warm-up,
medians reported.

The stages' shares: the public entries the loop calls are timed alone on the
flight's final state (one gossip round of acl_fleet_localize_batch, which runs
every track_every steps; one acl_fleet_est_control_batch; for comparison one
acl_control_batch on the true q), medians over `inner` calls each; the error
kernel's time is the difference of the diag-on and diag-off loops.
Writes one JSON document (--out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from aclswarm_amd import engine, workload  # noqa: E402


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def bench(n, B, F, steps, reps, warmup, inner, track_every, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(500 + n)
    w = workload.simform_workload(B, n, gen, dev, F=F, complete=False, planes=5)
    T = engine.FormationTable(w["n"], w["p"], w["bits"], w["gains"], w["gain_off"], w["planes"])
    T.tile_gains()

    def lossy():
        fe = engine.FleetEpisode(T, w["fidx"], w["q"], w["vel"], latency=1, loss=0)
        fe.run(0)  # (allocates the zero-filled workspace: not timed)
        return timed(lambda: fe.run(steps), dev), fe

    def own(diag):
        fe = engine.FleetEstEpisode(T, w["fidx"], w["q"], w["vel"], track_every=track_every,
                                    diag=diag)
        fe.run(0)
        return timed(lambda: fe.run(steps), dev), fe

    t = dict(lossy=[], off=[], on=[])
    for r in range(warmup + reps):
        runs = dict(lossy=lossy(), off=own(False), on=own(True))
        if r >= warmup:
            for k, (dt, _) in runs.items():
                t[k].append(dt)
    med = {k: statistics.median(v) for k, v in t.items()}
    fl, fx = runs["lossy"][1], runs["on"][1]
    st, sl = fx.status(), fl.status()
    assert (st["fleet"]["flags"] == 0).all() and (sl["fleet"]["flags"] == 0).all(), \
        "a swarm overflowed or was refused"
    x = st["estimates"]

    # the public entries alone, on the flight's final state
    loc = engine.FleetLocalization(T, w["fidx"], Pt=fx.Pt, loss=0)
    loc.stamp.copy_(fx.loc_stamp)
    loc.est.copy_(fx.loc_est)
    loc.round.copy_(fx.loc_round)

    def many(fn):
        def go():
            for _ in range(inner):
                fn()
        fn()
        return statistics.median(timed(go, dev) for _ in range(reps)) / inner
    t_round = many(lambda: loc.run(1, fx.q))
    t_ctl = many(lambda: engine.fleet_est_control(T, w["fidx"], fx.loc_est, fx.vel, fx.Pt))
    t_shared = many(lambda: engine.control(T, w["fidx"], fx.q, fx.vel, fx.P))
    step_off, step_on = med["off"] / steps, med["on"] / steps
    err = max(step_on - step_off, 0.0)

    def row(key):
        m = med[key]
        return dict(ms_per_step=m / steps * 1e3, swarm_steps_per_s=B * steps / m, s_all=t[key])
    return dict(
        n=n, B=B, formations=F, steps=steps, ticks_per_step=fx.ticks_per_step,
        auction_every=int(fx.ep.auction_every), track_every=track_every, latency=1, loss=0,
        d_max=int(w["adj"].sum(dim=2).max().item()),
        lossy=row("lossy"), est_diag_off=row("off"), est_diag_on=row("on"),
        est_over_lossy=med["off"] / med["lossy"], diag_on_over_off=med["on"] / med["off"],
        gossip_round_ms=t_round * 1e3, est_control_ms=t_ctl * 1e3, shared_control_ms=t_shared * 1e3,
        gossip_share=t_round / track_every / step_off, control_share=t_ctl / step_off,
        err_kernel_ms=err * 1e3, err_kernel_share_of_diag_on=err / step_on,
        vehicles_adopted=int(st["fleet"]["n_adopted"].sum()),
        vehicles_adopted_lossy=int(sl["fleet"]["n_adopted"].sum()),
        ca_vehicle_steps=int(st["episode"]["n_ca_steps"].sum()),
        ca_vehicle_steps_lossy=int(sl["episode"]["n_ca_steps"].sum()),
        rounds_run=int(x["rounds_run"].max()), n_unknown_total=int(x["n_unknown"].sum()),
        n_unknown_max=int(x["n_unknown"].max()), max_age=int(x["max_age"].max()),
        err_own_m=float(np.sqrt(x["err2_own"].max())), err_nbr_m=float(np.sqrt(x["err2_nbr"].max())),
        err_all_m=float(np.sqrt(x["err2_all"].max())), workspace_bytes=fx.workspace_bytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20x4096,100x256", help="n x B, comma-separated")
    ap.add_argument("--formations", type=int, default=8)
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--track-every", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_est_episode",
                                                  "steps.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = []
    for s in a.shapes.split(","):
        n, B = (int(x) for x in s.split("x"))
        r = bench(n, B, a.formations, a.steps, a.reps, a.warmup, a.inner, a.track_every, dev)
        print(json.dumps(r), flush=True)
        res.append(r)
    doc = dict(device=torch.cuda.get_device_name(dev), reps=a.reps, warmup=a.warmup,
               timing="wall clock between synchronisations, medians, loops alternated",
               results=res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
