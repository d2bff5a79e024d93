#!/usr/bin/env python3
"""Latency of a clean message-level auction for a whole fleet, two ways.

B swarms of n vehicles (noncomplete formations of the reference generator's
kind, identity rows, every vehicle starting from one snapshot) run the
per-vehicle CBAA protocol to its end:

  fleet   one acl_fleet_auction_batch call (engine.FleetAuction): queues,
          buckets and every tick on the device, to quiescence;
  paced   the host-paced loop that was the only way before it: one
          acl_vehicle_start_batch launch for the START bids, then 2n
          acl_cbaa_step_batch launches over all B n vehicles, the host
          choosing each vehicle's candidates (its neighbours' tables of the
          same iteration) between the launches. The candidate rows are
          gathered with torch.index_select on the device from index lists
          built once, which is faster than a gather through host memory.

With --latency L[,L...] a third path per L is alternated with them:

  delay   one acl_fleet_delay_auction_batch call with every link at L ticks
          (engine.FleetAuction(latency=L)): the same auction through the
          publication logs; its final tables must equal the fleet's.

With --loss K[,K...] (needs --latency) a fourth path per (L, K) is alternated
with them:

  lossy   one acl_fleet_lossy_auction_batch call with every link at L ticks and
          loss threshold K (engine.FleetAuction(latency=L, loss=K,
          loss_seed=1)). At K = 0 its final tables must equal the fleet's and
          the time is the feature's overhead over the delay path; at K > 0 the
          share of swarms that reach consensus before quiescence, ticks_run
          and the bids lost are reported.

All are timed wall-clock between synchronisations after a warm-up, the paths
alternated in one session, and the medians reported; the paced loop's final
tables must equal the fleet's. Writes one JSON document (--out) with the
times, the fleet kernel's time per tick and the workspace bytes.
"""
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


def make_case(n, B, F, seed, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    side = 2.0 * n ** 0.5 * 2.0
    p = workload.nonoverlapping_points(F, n, side, side, 0.0, 2.0, 2.0, gen, dev)
    adj = workload.random_adjacency(F, n, False, gen, dev)
    q = workload.nonoverlapping_points(B, n, side, side, 1.0, 1.0, 1.5, gen, dev)
    T = engine.FormationTable.from_host(list(p.cpu().numpy()),
                                        list(adj.cpu().numpy().astype(np.uint8)), None, device=dev)
    fidx = (torch.arange(B, device=dev) % F).to(torch.int32)
    return T, adj.cpu().numpy(), fidx, q.contiguous()


class Paced:
    """The host-paced protocol for all B n vehicles (identity rows)."""

    def __init__(self, T, adj, fidx, q):
        dev = q.device
        B, n = q.shape[0], q.shape[1]
        self.T, self.q, self.B, self.n = T, q, B, n
        f = fidx.cpu().numpy()
        self.fidx_v = fidx.repeat_interleave(n).contiguous()
        self.vehid = torch.arange(n, dtype=torch.int32, device=dev).repeat(B).contiguous()
        self.qidx = torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(n).contiguous()
        self.rows = torch.arange(n, dtype=torch.int16, device=dev).repeat(B * n, 1).contiguous()
        self.q_v = q.reshape(B * n, 3).contiguous()
        # candidates of vehicle (b, v): itself and its neighbours, ascending
        per_f = []
        for a in adj:
            c = a.astype(bool) | np.eye(n, dtype=bool)
            per_f.append([np.nonzero(c[v])[0] for v in range(n)])
        cnt = np.array([[len(x) for x in pf] for pf in per_f])[f].reshape(-1)
        off = np.zeros(B * n + 1, np.int64)
        off[1:] = np.cumsum(cnt)
        ids = np.concatenate([np.concatenate(per_f[fb]) for fb in f])
        base = np.repeat(np.arange(B) * n, cnt.reshape(B, n).sum(axis=1))
        self.K = int(off[-1])
        assert self.K < 2 ** 31
        self.cand_off = torch.from_numpy(off.astype(np.int32)).to(dev)
        self.cand_vehid = torch.from_numpy(ids.astype(np.int32)).to(dev)
        self.cand_row = torch.from_numpy(ids + base).to(dev)
        self.start0 = torch.zeros(B * n, dtype=torch.uint8, device=dev)

    def run(self):
        n = self.n
        out = engine.vehicle_start(self.T, self.fidx_v, self.vehid, self.q, self.rows,
                                   qidx=self.qidx)
        price, who, Rt = out["price"], out["who"], out["Rt"]
        for _ in range(2 * n):
            cp = price.index_select(0, self.cand_row)
            cw = who.index_select(0, self.cand_row)
            engine.cbaa_step(self.T, self.fidx_v, self.vehid, self.q_v, Rt, self.start0, price,
                             who, self.cand_off, self.cand_vehid, cp, cw)
        return who


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, r


def bench(n, B, F, reps, warmup, dev, latencies=(), losses=()):
    T, adj, fidx, q = make_case(n, B, F, 1000 + n, dev)
    d_max = int(adj.sum(axis=2).max())
    ticks = 2 * n * d_max + 8
    cmd = torch.full((B, n), L.FLEET_START, dtype=torch.uint8, device=dev)
    fa = engine.FleetAuction(T, fidx)
    ws = torch.zeros(fa.workspace_bytes(), dtype=torch.uint8, device=dev)
    paced = Paced(T, adj, fidx, q)

    def fleet():
        f = engine.FleetAuction(T, fidx)  # fresh auctioneers (not timed)
        f.ws = ws.zero_()
        dt, _ = timed(lambda: f.run(ticks, q=q, cmd=cmd), dev)
        return dt, f

    def delay(lat):
        # (a bid crosses a link in lat ticks instead of 1: lat times the ticks are enough)
        d = engine.FleetAuction(T, fidx, latency=lat)
        d.ws = torch.zeros(d.workspace_bytes(), dtype=torch.uint8, device=dev)
        dt, _ = timed(lambda: d.run(ticks * lat, q=q, cmd=cmd), dev)
        return dt, d

    def lossy(lat, loss):
        d = engine.FleetAuction(T, fidx, latency=lat, loss=loss, loss_seed=1)
        d.ws = torch.zeros(d.workspace_bytes(), dtype=torch.uint8, device=dev)
        dt, _ = timed(lambda: d.run(ticks * lat, q=q, cmd=cmd), dev)
        return dt, d

    t_fleet, t_paced, t_delay, last = [], [], {lat: [] for lat in latencies}, {}
    pairs = [(lat, k) for lat in latencies for k in losses]
    t_lossy, last_lossy = {pk: [] for pk in pairs}, {}
    for r in range(warmup + reps):
        dt_f, f = fleet()
        for lat in latencies:
            dt_d, last[lat] = delay(lat)
            if r >= warmup:
                t_delay[lat].append(dt_d)
            for k in losses:
                dt_l, last_lossy[lat, k] = lossy(lat, k)
                if r >= warmup:
                    t_lossy[lat, k].append(dt_l)
        dt_p, who_p = timed(paced.run, dev)
        if r >= warmup:
            t_fleet.append(dt_f)
            t_paced.append(dt_p)
    st = f.status()
    assert (st["flags"] == L.FLEET_QUIESCENT).all() and (st["n_open"] == 0).all()
    same = bool((f.final_who.reshape(B * n, n) == who_p).all())
    assert same, "the paced loop and the fleet call disagree"
    mf, mp = statistics.median(t_fleet), statistics.median(t_paced)
    tr = int(st["ticks_run"].max())
    delays = []
    for lat in latencies:
        d, sd = last[lat], last[lat].status()
        assert (sd["flags"] == L.FLEET_QUIESCENT).all() and (sd["n_open"] == 0).all()
        assert bool((d.final_who == f.final_who).all()), "the delay entry's tables differ"
        md, trd = statistics.median(t_delay[lat]), int(sd["ticks_run"].max())
        delays.append(dict(latency=lat, delay_ms=md * 1e3,
                           delay_ms_all=[x * 1e3 for x in t_delay[lat]],
                           ticks_run_max=trd, ticks_run_min=int(sd["ticks_run"].min()),
                           delay_us_per_tick=md * 1e6 / trd, delay_over_fleet=md / mf,
                           workspace_bytes=d.workspace_bytes(), tables_equal=True,
                           thrown=int(d.n_thrown.sum().item())))
    lossies = []
    for lat, k in pairs:
        d, sd = last_lossy[lat, k], last_lossy[lat, k].status()
        assert (sd["flags"] == L.FLEET_QUIESCENT).all()
        ml, md = statistics.median(t_lossy[lat, k]), statistics.median(t_delay[lat])
        if k == 0:
            assert (sd["n_open"] == 0).all() and not bool(d.n_lost.any())
            assert bool((d.final_who == f.final_who).all()), "the lossy entry's tables differ"
        done = sd["n_open"] == 0
        lossies.append(dict(latency=lat, loss=k, lossy_ms=ml * 1e3,
                            lossy_ms_all=[x * 1e3 for x in t_lossy[lat, k]],
                            lossy_over_delay=ml / md, consensus_share=float(done.mean()),
                            ticks_run_max=int(sd["ticks_run"].max()),
                            ticks_run_median=float(np.median(sd["ticks_run"])),
                            ticks_run_min=int(sd["ticks_run"].min()),
                            lost=int(d.n_lost.sum().item()),
                            swarms_with_a_lost_bid=int((d.n_lost.sum(dim=1) > 0).sum().item())))
    return dict(delay=delays, lossy=lossies, n=n, B=B, formations=F, d_max=d_max, queue_cap=fa.queue_cap,
                ticks_run_max=tr, ticks_run_min=int(st["ticks_run"].min()),
                fleet_ms=mf * 1e3, fleet_ms_all=[x * 1e3 for x in t_fleet],
                fleet_us_per_tick=mf * 1e6 / tr,
                paced_ms=mp * 1e3, paced_ms_all=[x * 1e3 for x in t_paced],
                paced_launches=2 * n + 1, paced_candidate_rows=paced.K,
                paced_over_fleet=mp / mf, tables_equal=same,
                workspace_bytes=fa.workspace_bytes(),
                workspace_bytes_per_swarm=fa.workspace_bytes() // B,
                thrown=int(f.n_thrown.sum().item()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20x4096,100x256", help="n x B, comma-separated")
    ap.add_argument("--formations", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--latency", default="", help="uniform link latencies in ticks, "
                    "comma-separated: also time acl_fleet_delay_auction_batch at each")
    ap.add_argument("--loss", default="", help="loss thresholds 0..65535, comma-separated: also "
                    "time acl_fleet_lossy_auction_batch at each --latency and each of these")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_auction",
                                                  "latency.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = []
    for s in a.shapes.split(","):
        n, B = (int(x) for x in s.split("x"))
        r = bench(n, B, a.formations, a.reps, a.warmup, dev,
                  [int(x) for x in a.latency.split(",") if x],
                  [int(x) for x in a.loss.split(",") if x])
        print(json.dumps(r), flush=True)
        res.append(r)
    doc = dict(device=torch.cuda.get_device_name(dev), reps=a.reps, warmup=a.warmup,
               timing="wall clock between synchronisations, medians, paths alternated",
               results=res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
