#!/usr/bin/env python3
"""Step time of the trials on own estimates with tables on real links and the
encounter record (acl_fleet_delay_est_trial_batch) beside
acl_fleet_est_trial_batch on the same swarms, and what happened in the flights.

The workload is scripts/fleet_est_trial_bench.py's, unchanged: B swarms of n
vehicles on noncomplete formations of the reference generator, 5-plane gains,
ticks_per_step 10, every message link at 1 tick, loss 0, track_every 2, two
formations per trial, `steps` steps from fresh state with --hover-wait 0.02 and
--settle-steps 1. Five loops are alternated in one session, each timed wall-clock
between synchronisations after a warm-up, medians reported with every sample and
the spread of the existing entry's own repetitions:
  est         acl_fleet_est_trial_batch (diag off)
  lat0        the new entry, every table link at 0 rounds, no record
  lat0_enc    ... with the encounter record
  lat2        the new entry, every table link at 2 rounds, no record
  lat2_enc    ... with the encounter record
Then one further, untimed flight with histories at latency 0 and at latency 2
(diag and the record on): adoptions, CA vehicle-steps, the err2 maxima, the
smallest true separation and the breach, blind and ghost totals.
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

LOOPS = ("est", "lat0", "lat0_enc", "lat2", "lat2_enc")


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def outcomes(tr, steps, chunk):
    """An untimed flight with histories, in chunks."""
    ca = 0
    for s in range(0, steps, chunk):
        h = tr.run(min(chunk, steps - s), history=True)
        ca += int(h["ca"].sum().item())
    st = tr.status()
    fs = tr.fleet_status()
    f, x, e = fs["fleet"], fs["estimates"], fs["encounters"]
    worst = int(np.argmin(e["sep2_min"]))
    inside = e["sep2_min"] < tr.safety.r_keep_out ** 2
    return dict(complete=int((st["state"] == L.TRIAL_COMPLETE).sum()),
                terminated=int((st["state"] == L.TRIAL_TERMINATE).sum()),
                still_flying=int((st["done_step"] < 0).sum()),
                vehicles_adopted=int(f["n_adopted"].sum()),
                vehicles_invalid=int(f["n_invalid"].sum()),
                controllers_on=int(tr.ctl_on.sum().item()), ca_vehicle_steps=ca,
                rounds_run=int(x["rounds_run"].max()), n_unknown_total=int(x["n_unknown"].sum()),
                max_age=int(x["max_age"].max()),
                err_own_m=float(np.sqrt(x["err2_own"].max())),
                err_nbr_m=float(np.sqrt(x["err2_nbr"].max())),
                err_all_m=float(np.sqrt(x["err2_all"].max())),
                sep_min_m=float(np.sqrt(e["sep2_min"].min())),
                sep_min_median_m=float(np.sqrt(np.median(e["sep2_min"]))),
                sep_min_swarm=worst, sep_min_step=int(e["step"][worst]),
                sep_min_pair=[int(e["i"][worst]), int(e["j"][worst])],
                swarms_with_a_breach=int(inside.sum()),
                breach_pair_steps=int(e["n_breach"].sum()),
                blind_pair_steps=int(e["n_blind"].sum()),
                ghost_pair_steps=int(e["n_ghost"].sum()),
                swarms_with_blind=int((e["n_blind"] > 0).sum()),
                swarms_with_ghost=int((e["n_ghost"] > 0).sum()),
                senses_missed=int(tr.n_missed.sum().item()))


def bench(n, B, F, steps, reps, warmup, track_every, hover_wait, settle_steps, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(500 + n)
    w = workload.simform_workload(B, n, gen, dev, F=F, complete=False, planes=5)
    T = engine.FormationTable(w["n"], w["p"], w["bits"], w["gains"], w["gain_off"], w["planes"])
    T.tile_gains()
    f0 = w["fidx"].to(torch.int32)
    fseq = torch.stack([f0, (f0 + 1) % F], dim=1).contiguous()
    tp = L.default_trial_params()
    tp.hover_wait, tp.settle_steps = hover_wait, settle_steps

    def make(key, diag=False):
        kw = {}
        if key != "est":
            kw = dict(table_latency=int(key[3]), max_table_latency=2,
                      encounters=key.endswith("_enc"))
        return engine.FleetEstTrial(T, fseq, w["q"], w["vel"], params=tp,
                                    track_every=track_every, diag=diag, **kw)

    t = {k: [] for k in LOOPS}
    for r in range(warmup + reps):
        for k in LOOPS:
            tr = make(k)  # (allocation and init: not timed)
            dt = timed(lambda: tr.run(steps), dev)
            if r >= warmup:
                t[k].append(dt)
            del tr
    med = {k: statistics.median(v) for k, v in t.items()}

    def row(key):
        m = med[key]
        return dict(ms_per_step=m / steps * 1e3, swarm_steps_per_s=B * steps / m, s_all=t[key],
                    over_est=m / med["est"])
    chunk = max(1, min(steps, (1 << 28) // (B * n * 80)))
    out = dict(n=n, B=B, formations=F, formations_per_trial=2, steps=steps,
               ticks_per_step=10, track_every=track_every, latency=1, loss=0,
               hover_wait=hover_wait, settle_steps=settle_steps,
               est_spread=(max(t["est"]) - min(t["est"])) / med["est"],
               record_over_lat0=med["lat0_enc"] / med["lat0"],
               record_over_lat2=med["lat2_enc"] / med["lat2"],
               record_ms_per_step=(med["lat0_enc"] - med["lat0"]) / steps * 1e3)
    for k in LOOPS:
        out[k] = row(k)
    out["flight_lat0"] = outcomes(make("lat0_enc", True), steps, chunk)
    out["flight_lat2"] = outcomes(make("lat2_enc", True), steps, chunk)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20x4096,100x256", help="n x B, comma-separated")
    ap.add_argument("--formations", type=int, default=8)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--track-every", type=int, default=2)
    ap.add_argument("--hover-wait", type=float, default=0.02)
    ap.add_argument("--settle-steps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_delay_est_trial",
                                                  "steps.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = []
    for s in a.shapes.split(","):
        n, B = (int(x) for x in s.split("x"))
        r = bench(n, B, a.formations, a.steps, a.reps, a.warmup, a.track_every, a.hover_wait,
                  a.settle_steps, dev)
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
