#!/usr/bin/env python3
"""Step time of the episodes on the message-level auction
(acl_fleet_episode_batch, engine.FleetEpisode) against the synchronous
episode with the reference's auction timing (engine.Episode, auction_latency
= -1) on the same swarms.

B swarms of n vehicles on noncomplete formations of the reference generator
(workload.simform_workload: simform20_nc's recipe at n = 20, the C3 shape at
n = 100), 5-plane gains, ticks_per_step = 10 and the default episode
parameters (an auto-auction every 120 steps). Both loops fly `steps` control
periods from fresh state; timed wall-clock between synchronisations after a
warm-up of every shape, the two loops alternated in one session, medians
reported. The ticks' share of the step is estimated from the fleet kernel's
time per tick in profiles/fleet_auction/latency.json (its own measurement, one
launch to quiescence) times the ticks the slowest swarm ran.

Also recorded: how many of the started auctions reach consensus before the
next auto-auction restarts them -- at large d_max the reference's own
auctions (2 n d_max ticks of 1 ms) outlast its 1.2 s auto-auction period.

With --latency L[,L...] a further loop per L is alternated with them: the same
episodes on acl_fleet_delay_episode_batch with every link at L ticks
(engine.FleetEpisode(latency=L)), reported under "delay".
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

from aclswarm_amd import _lib as L  # noqa: E402
from aclswarm_amd import engine, workload  # noqa: E402


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def per_tick_us(n, B):
    path = os.path.join(ROOT, "profiles", "fleet_auction", "latency.json")
    if not os.path.exists(path):
        return None
    with open(path) as fh:
        for r in json.load(fh)["results"]:
            if (r["n"], r["B"]) == (n, B):
                return r["fleet_us_per_tick"]
    return None


def bench(n, B, F, steps, reps, warmup, dev, latencies=()):
    gen = torch.Generator(device=dev)
    gen.manual_seed(500 + n)
    w = workload.simform_workload(B, n, gen, dev, F=F, complete=False, planes=5)
    T = engine.FormationTable(w["n"], w["p"], w["bits"], w["gains"], w["gain_off"], w["planes"])
    T.tile_gains()
    d_max = int(w["adj"].sum(dim=2).max().item())
    lat = L.default_episode_params()
    lat.auction_latency = -1
    ws = None

    def fleet():
        nonlocal ws
        fe = engine.FleetEpisode(T, w["fidx"], w["q"], w["vel"])  # fresh state (not timed)
        if ws is None:
            ws = torch.zeros(fe.workspace_bytes(), dtype=torch.uint8, device=dev)
        fe.ws = ws.zero_()
        return timed(lambda: fe.run(steps), dev), fe

    def delayed(ticks):
        fe = engine.FleetEpisode(T, w["fidx"], w["q"], w["vel"], latency=ticks)
        fe.run(0)  # (allocates the zero-filled workspace: not timed)
        return timed(lambda: fe.run(steps), dev), fe

    def sync_episode():
        e = engine.Episode(T, w["fidx"], w["q"], w["vel"], w["P_in"], params=lat)
        return timed(lambda: e.run(steps), dev), e

    t_fleet, t_sync = [], []
    t_delay, last_delay = {k: [] for k in latencies}, {}
    for r in range(warmup + reps):
        dt_f, fe = fleet()
        dt_s, e = sync_episode()
        if r >= warmup:
            t_fleet.append(dt_f)
            t_sync.append(dt_s)
        for k in latencies:
            dt_d, fd = delayed(k)
            if r >= warmup:
                t_delay[k].append(dt_d)
            last_delay[k] = fd.status()["fleet"], fd.workspace_bytes()
            del fd
    st = fe.status()
    fst, est = st["fleet"], e.status()
    assert (fst["flags"] == 0).all(), "a swarm overflowed or was refused"
    mf, ms = statistics.median(t_fleet), statistics.median(t_sync)
    started, consensus = int(fst["n_started"].sum()), int(fst["n_consensus"].sum())
    ticks_max = int(fst["ticks_run"].max())
    us = per_tick_us(n, B)
    delays = []
    for k in latencies:
        md = statistics.median(t_delay[k])
        f, wsb = last_delay[k]
        assert (f["flags"] == 0).all(), "a swarm overflowed or was refused"
        delays.append(dict(
            latency=k, delay_ms_per_step=md / steps * 1e3, delay_swarm_steps_per_s=B * steps / md,
            delay_s_all=t_delay[k], delay_over_fleet=md / mf,
            ticks_run_max=int(f["ticks_run"].max()), ticks_run_min=int(f["ticks_run"].min()),
            vehicle_auctions_started=int(f["n_started"].sum()),
            vehicle_auctions_restarted=int(f["n_restarted"].sum()),
            vehicle_auctions_finished=int(f["n_consensus"].sum()),
            vehicles_adopted=int(f["n_adopted"].sum()), vehicles_invalid=int(f["n_invalid"].sum()),
            workspace_bytes=wsb))
    return dict(
        delay=delays,
        n=n, B=B, formations=F, d_max=d_max, steps=steps, ticks_per_step=fe.ticks_per_step,
        auction_every=int(fe.ep.auction_every), queue_cap=fe.queue_cap,
        fleet_ms_per_step=mf / steps * 1e3, fleet_swarm_steps_per_s=B * steps / mf,
        fleet_s_all=t_fleet,
        sync_ms_per_step=ms / steps * 1e3, sync_swarm_steps_per_s=B * steps / ms,
        sync_s_all=t_sync, fleet_over_sync=mf / ms,
        sync_auctions=int(est["n_auctions"].sum()), sync_restarted=int(est["n_restarted"].sum()),
        ticks_run_max=ticks_max, ticks_run_min=int(fst["ticks_run"].min()),
        fleet_auction_us_per_tick=us,
        ticks_share_estimate=(None if us is None else ticks_max * us * 1e-6 / mf),
        vehicle_auctions_started=started, vehicle_auctions_restarted=int(fst["n_restarted"].sum()),
        vehicle_auctions_finished=consensus,
        finished_before_restart=consensus / started if started else None,
        vehicles_adopted=int(fst["n_adopted"].sum()), vehicles_invalid=int(fst["n_invalid"].sum()),
        per_vehicle_swarms_at_end=int(st["episode"]["per_vehicle"].sum()),
        workspace_bytes=fe.workspace_bytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20x4096,100x256", help="n x B, comma-separated")
    ap.add_argument("--formations", type=int, default=8)
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--latency", default="", help="uniform link latencies in ticks, "
                                                  "comma-separated (default: none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_episode", "steps.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = []
    for s in a.shapes.split(","):
        n, B = (int(x) for x in s.split("x"))
        r = bench(n, B, a.formations, a.steps, a.reps, a.warmup, dev,
                  [int(x) for x in a.latency.split(",") if x])
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
