#!/usr/bin/env python3
"""Monte-Carlo trials on the message-level auction (acl_fleet_trial_batch,
engine.FleetTrial) against the trials on the synchronous auction
(acl_trial_batch, engine.Trial, CBAA) on the same swarms.

B trials of n vehicles: the reference generator's formation groups ('A' then
'B') with gains designed by acl_admm_solve_batch (episode_bench.admm_table),
start.sh-style starts, the default trial timings (supervisor.py:50-57,
coordination.launch), ticks_per_step = 10. Every trial is flown to its end
(or to --max-steps); wall clock between synchronisations, one status read
per --chunk steps; a warm-up of both loops, then the two alternated --reps
times, medians reported. The records are the last repetition's (the runs
are deterministic).

For both loops: trials/s, complete / terminated counts and the state
terminated from, time to converge, gridlock time and assignments per
formation. For the new loop also the vehicle events: starts, restarts,
flushes, and the vehicle auctions that ended neither in a restart nor in
consensus, i.e. were interrupted by a commit or cut by the trial's end.

With --latency L[,L...] a further loop per L is alternated with them: the same
trials on acl_fleet_delay_trial_batch with every link at L ticks
(engine.FleetTrial(latency=L)), reported as "fleet_L<L>" with the same figures.
With --loss K[,K...] (and --latency) also acl_fleet_lossy_trial_batch at every
(L, K) (engine.FleetTrial(latency=L, loss=K, loss_seed=1)), reported as
"fleet_L<L>_loss<K>" with the bids lost and the share of trials that ended
through the supervisor's assignment timeout (TERMINATE from WAITING).
Writes one JSON document (--out)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from aclswarm_amd import _lib as L  # noqa: E402
from aclswarm_amd import engine, workload  # noqa: E402
from episode_bench import admm_table, trial_stats  # noqa: E402


def fly(make, max_steps, chunk, dev):
    """A fresh trial object flown to the end of every trial; (seconds, steps,
    object). The construction (allocation, init) is not timed."""
    tr = make()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    steps = 0
    while steps < max_steps:
        c = min(chunk, max_steps - steps)
        tr.run(c)
        steps += c
        if (tr.status()["done_step"] >= 0).all():  # (one synchronisation per chunk)
            break
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, steps, tr


def bench(n, B, reps, warmup, max_steps, chunk, dev, latencies=(), losses=()):
    L_side = 15.0 if n <= 20 else 40.0 * (n / 100.0) ** 0.5
    T, t_admm, admm = admm_table(n, B, L_side, 0, dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    side = 20.0 * (n / 20.0) ** 0.5
    q = workload.nonoverlapping_points(B, n, side, side, 1.0, 1.0, 1.5, gen, dev)
    vel = torch.zeros_like(q)
    fseq = torch.arange(2 * B, dtype=torch.int32, device=dev).view(B, 2)
    loops = {"fleet": lambda: engine.FleetTrial(T, fseq, q, vel),
             "sync": lambda: engine.Trial(T, fseq, q, vel)}
    for lat in latencies:
        loops[f"fleet_L{lat}"] = lambda lat=lat: engine.FleetTrial(T, fseq, q, vel, latency=lat)
        for k in losses:
            loops[f"fleet_L{lat}_loss{k}"] = lambda lat=lat, k=k: engine.FleetTrial(
                T, fseq, q, vel, latency=lat, loss=k, loss_seed=1)
    times = {k: [] for k in loops}
    last = {}
    for r in range(warmup + reps):
        for k, make in loops.items():
            dt, steps, tr = fly(make, max_steps, chunk, dev)
            if r >= warmup:
                times[k].append(dt)
            last[k] = (steps, tr)
            if r < warmup + reps - 1:
                del tr
                last[k] = None
                torch.cuda.empty_cache()
    out = dict(n=n, B=B, formations_per_trial=2, ticks_per_step=10, max_steps=max_steps,
               chunk=chunk, admm_seconds=t_admm, **admm)
    for k in loops:
        steps, tr = last[k]
        m = statistics.median(times[k])
        r = trial_stats(tr, 2)
        r.update(trials_per_s=B / m, seconds=m, seconds_all=times[k], steps_run=steps,
                 ms_per_step=m / steps * 1e3)
        if k.startswith("fleet"):
            f = tr.fleet_status()["fleet"]
            started, restarted = int(f["n_started"].sum()), int(f["n_restarted"].sum())
            consensus = int(f["n_consensus"].sum())
            r.update(vehicle_starts=started, vehicle_restarts=restarted,
                     vehicle_flushes=int(f["n_flushed"].sum()), vehicle_consensus=consensus,
                     vehicle_adopted=int(f["n_adopted"].sum()),
                     vehicle_invalid=int(f["n_invalid"].sum()),
                     vehicle_auctions_cut_by_commit_or_end=started - restarted - consensus,
                     bids_thrown=int(tr.n_thrown.sum().item()),
                     overflowed_swarms=int((f["flags"] & L.FLEET_OVERFLOW != 0).sum()),
                     workspace_bytes=tr.workspace_bytes())
        out[k] = r
    out["fleet_over_sync_seconds"] = out["fleet"]["seconds"] / out["sync"]["seconds"]
    for lat in latencies:
        out[f"fleet_L{lat}"]["latency"] = lat
        out[f"fleet_L{lat}_over_fleet_seconds"] = (out[f"fleet_L{lat}"]["seconds"] /
                                                   out["fleet"]["seconds"])
        for k in losses:
            r = out[f"fleet_L{lat}_loss{k}"]
            tr = last[f"fleet_L{lat}_loss{k}"][1]
            st = tr.status()
            timed_out = (st["state"] == L.TRIAL_TERMINATE) & (st["last_state"] == L.TRIAL_WAITING)
            r.update(latency=lat, loss=k, bids_lost=int(tr.n_lost.sum().item()),
                     assignment_timeout_share=float(timed_out.mean()),
                     seconds_over_delay=r["seconds"] / out[f"fleet_L{lat}"]["seconds"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20x4096", help="n x B, comma-separated")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-steps", type=int, default=12000)
    ap.add_argument("--chunk", type=int, default=500)
    ap.add_argument("--latency", default="", help="uniform link latencies in ticks, "
                                                  "comma-separated (default: none)")
    ap.add_argument("--loss", default="", help="loss thresholds 0..65535, comma-separated: "
                    "acl_fleet_lossy_trial_batch at each --latency and each of these")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_trial", "trials.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = []
    for s in a.shapes.split(","):
        n, B = (int(x) for x in s.split("x"))
        r = bench(n, B, a.reps, a.warmup, a.max_steps, a.chunk, dev,
                  [int(x) for x in a.latency.split(",") if x],
                  [int(x) for x in a.loss.split(",") if x])
        print(json.dumps(r), flush=True)
        res.append(r)
    doc = dict(device=torch.cuda.get_device_name(dev), reps=a.reps, warmup=a.warmup,
               timing="wall clock between synchronisations (one status read per chunk), medians, "
                      "loops alternated", results=res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
