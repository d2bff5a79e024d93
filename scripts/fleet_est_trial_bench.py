#!/usr/bin/env python3
"""Step time of the trials on each vehicle's own estimates
(acl_fleet_est_trial_batch, engine.FleetEstTrial) beside the shared-snapshot
trials with the same links (acl_fleet_lossy_trial_batch, engine.FleetTrial with
latency 1 and loss 0) on the same swarms.

The shapes and the workload are scripts/fleet_est_episode_bench.py's: B swarms
of n vehicles on noncomplete formations of the reference generator, 5-plane
gains, ticks_per_step 10; every link at 1 tick, loss 0, track_every 2. Swarm b
flies two formations of the table (its own and the next one) for `steps` steps
from fresh state, under the default trial timings except hover_wait and
settle_steps (--hover-wait 0.02, --settle-steps 1: the first formation commits
at step 3 and its first auction starts at step 4, so the steps timed are steps
of a flying trial, not of the supervisor's hover). Three loops are alternated in
one session -- the lossy entry, the new entry with diag off, the new entry with
diag on -- timed wall-clock between synchronisations after a warm-up, medians
reported, with the spread of the lossy entry's own repetitions.

The stages' shares: the public entries the loop calls are timed alone on the
flight's final state (one gossip round of acl_fleet_localize_batch under
loc_Pt, which runs every track_every steps; one acl_fleet_est_control_batch),
medians over `inner` calls each; the error record's time is the difference of
the diag-on and diag-off loops. The flight outcomes of the own-estimate trials
stand next to the shared-snapshot ones; the CA vehicle-steps come from one
further, untimed flight of each with histories.
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

from aclswarm_amd import _lib as L  # noqa: E402
from aclswarm_amd import engine, workload  # noqa: E402


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def outcomes(tr, steps, chunk):
    """An untimed flight with histories, in chunks: CA vehicle-steps of running
    controllers; then the trial's own records."""
    ca = 0
    for s in range(0, steps, chunk):
        h = tr.run(min(chunk, steps - s), history=True)
        ca += int(h["ca"].sum().item())
    st = tr.status()
    f = tr.fleet_status()["fleet"]
    return dict(complete=int((st["state"] == L.TRIAL_COMPLETE).sum()),
                terminated=int((st["state"] == L.TRIAL_TERMINATE).sum()),
                still_flying=int((st["done_step"] < 0).sum()),
                vehicles_adopted=int(f["n_adopted"].sum()),
                vehicles_invalid=int(f["n_invalid"].sum()),
                controllers_on=int(tr.ctl_on.sum().item()), ca_vehicle_steps=ca)


def bench(n, B, F, steps, reps, warmup, inner, track_every, hover_wait, settle_steps, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(500 + n)
    w = workload.simform_workload(B, n, gen, dev, F=F, complete=False, planes=5)
    T = engine.FormationTable(w["n"], w["p"], w["bits"], w["gains"], w["gain_off"], w["planes"])
    T.tile_gains()
    f0 = w["fidx"].to(torch.int32)
    fseq = torch.stack([f0, (f0 + 1) % F], dim=1).contiguous()

    tp = L.default_trial_params()
    tp.hover_wait, tp.settle_steps = hover_wait, settle_steps

    def lossy():
        return engine.FleetTrial(T, fseq, w["q"], w["vel"], params=tp, latency=1, loss=0)

    def own(diag):
        return engine.FleetEstTrial(T, fseq, w["q"], w["vel"], params=tp,
                                    track_every=track_every, diag=diag)

    def fly(make):
        tr = make()  # (allocation and init: not timed)
        return timed(lambda: tr.run(steps), dev), tr

    t = dict(lossy=[], off=[], on=[])
    for r in range(warmup + reps):
        runs = dict(lossy=fly(lossy), off=fly(lambda: own(False)), on=fly(lambda: own(True)))
        if r >= warmup:
            for k, (dt, _) in runs.items():
                t[k].append(dt)
    med = {k: statistics.median(v) for k, v in t.items()}
    fx = runs["on"][1]
    x = fx.fleet_status()["estimates"]
    flagged = int((fx.fleet_status()["fleet"]["flags"] != 0).sum())  # overflowed or refused

    # the public entries alone, on the flight's final state
    loc = engine.FleetLocalization(T, fx.fidx, Pt=fx.loc_Pt, loss=0)
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
    t_ctl = many(lambda: engine.fleet_est_control(T, fx.fidx, fx.loc_est, fx.vel, fx.Pt))
    step_off, step_on = med["off"] / steps, med["on"] / steps
    err = max(step_on - step_off, 0.0)
    chunk = max(1, min(steps, (1 << 28) // (B * n * 80)))
    out_own, out_lossy = outcomes(own(True), steps, chunk), outcomes(lossy(), steps, chunk)

    def row(key):
        m = med[key]
        return dict(ms_per_step=m / steps * 1e3, swarm_steps_per_s=B * steps / m, s_all=t[key])
    return dict(
        n=n, B=B, formations=F, formations_per_trial=2, steps=steps,
        ticks_per_step=fx.ticks_per_step, auction_every=int(fx.tp.ep.auction_every),
        track_every=track_every, latency=1, loss=0, hover_wait=hover_wait,
        settle_steps=settle_steps,
        d_max=int(w["adj"].sum(dim=2).max().item()),
        lossy=row("lossy"), est_diag_off=row("off"), est_diag_on=row("on"),
        lossy_spread=(max(t["lossy"]) - min(t["lossy"])) / med["lossy"],
        est_over_lossy=med["off"] / med["lossy"], diag_on_over_off=med["on"] / med["off"],
        gossip_round_ms=t_round * 1e3, est_control_ms=t_ctl * 1e3,
        gossip_share=t_round / track_every / step_off, control_share=t_ctl / step_off,
        err_record_ms=err * 1e3, err_record_share_of_diag_on=err / step_on,
        own_estimates=out_own, shared_snapshot=out_lossy, flagged_swarms=flagged,
        rounds_run=int(x["rounds_run"].max()), n_unknown_total=int(x["n_unknown"].sum()),
        n_unknown_max=int(x["n_unknown"].max()), max_age=int(x["max_age"].max()),
        err_own_m=float(np.sqrt(x["err2_own"].max())),
        err_nbr_m=float(np.sqrt(x["err2_nbr"].max())),
        err_all_m=float(np.sqrt(x["err2_all"].max())), workspace_bytes=fx.workspace_bytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20x4096,100x256", help="n x B, comma-separated")
    ap.add_argument("--formations", type=int, default=8)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--track-every", type=int, default=2)
    ap.add_argument("--hover-wait", type=float, default=0.02)
    ap.add_argument("--settle-steps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_est_trial",
                                                  "steps.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = []
    for s in a.shapes.split(","):
        n, B = (int(x) for x in s.split("x"))
        r = bench(n, B, a.formations, a.steps, a.reps, a.warmup, a.inner, a.track_every,
                  a.hover_wait, a.settle_steps, dev)
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
