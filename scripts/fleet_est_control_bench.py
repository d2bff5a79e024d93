#!/usr/bin/env python3
"""Time of one control step from own estimates (acl_fleet_est_control_batch)
beside acl_control_batch on the same swarms.

B swarms of n vehicles (fleet_episode_bench's workload: simform formations,
5-plane gains, identity assignments), each `uncrowded` (the workload's start
positions, 1.5 m apart at least) and `crowded` (the same positions shrunk to
40 %: most vehicles have several others within d_avoid_thresh). est is q
broadcast to every vehicle and every row is the identity, so both entries
compute the same commands, which is checked (u and u_safe within 1e-5
relative, equal flags).

  est      engine.fleet_est_control: reads B n^2 24 B of tables (its byte
           floor, reported as a share of the 8 TB/s peak) and B n^2 2 B of rows
  control  engine.control: reads B n 24 B of positions

`inner` calls between two synchronisations, wall clock, medians of `reps` after
a warm-up, the two alternated in one session. Writes one JSON document (--out)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from aclswarm_amd import engine, workload  # noqa: E402
from fleet_auction_bench import timed  # noqa: E402

PEAK_BYTES_PER_S = 8e12


def bench(n, B, F, reps, warmup, inner, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(500 + n)
    w = workload.simform_workload(B, n, gen, dev, F=F, complete=False, planes=5)
    T = engine.FormationTable(w["n"], w["p"], w["bits"], w["gains"], w["gain_off"], w["planes"])
    T.tile_gains()
    rows = torch.arange(n, dtype=torch.int16, device=dev).repeat(B, n, 1).contiguous()
    out = dict(n=n, B=B, formations=F, est_bytes=B * n * n * 24, cases=[])
    for name, scale in (("uncrowded", 1.0), ("crowded", 0.4)):
        q = w["q"].clone()
        q[:, :, :2] *= scale
        est = q.unsqueeze(1).expand(B, n, n, 3).contiguous()

        def own():
            r = None
            for _ in range(inner):
                r = engine.fleet_est_control(T, w["fidx"], est, w["vel"], rows)
            return r

        def ctl():
            r = None
            for _ in range(inner):
                r = engine.control(T, w["fidx"], q, w["vel"], w["P_in"])
            return r

        te, tc = [], []
        for r in range(warmup + reps):
            de, oe = timed(own, dev)
            dc, oc = timed(ctl, dev)
            if r >= warmup:
                te.append(de / inner)
                tc.append(dc / inner)
        for k in ("u", "u_safe"):
            err = ((oe[k] - oc[k]).abs() / oc[k].abs().clamp(min=1.0)).max().item()
            assert err <= 1e-5, f"{name}: {k} differs by {err:.3e}"
        assert bool((oe["ca_flag"] == oc["ca_flag"]).all()), f"{name}: ca_flag differs"
        n_ca = int(oe["ca_flag"].sum().item())
        assert n_ca == int(oe["status"][:, 0].sum().item())
        me, mc = statistics.median(te), statistics.median(tc)
        out["cases"].append(dict(
            case=name, est_ms=me * 1e3, est_ms_all=[x * 1e3 for x in te], control_ms=mc * 1e3,
            control_ms_all=[x * 1e3 for x in tc], est_over_control=me / mc,
            est_read_share_of_peak=out["est_bytes"] / me / PEAK_BYTES_PER_S,
            commands_equal=True, n_ca=n_ca, ca_share=n_ca / (B * n)))
        del est
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20x4096,100x256,100x4096", help="n x B, comma-separated")
    ap.add_argument("--formations", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--inner", type=int, default=10, help="calls between two synchronisations")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_est_control",
                                                  "control.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = []
    for s in a.shapes.split(","):
        n, B = (int(x) for x in s.split("x"))
        r = bench(n, B, a.formations, a.reps, a.warmup, a.inner, dev)
        print(json.dumps(r), flush=True)
        res.append(r)
    doc = dict(device=torch.cuda.get_device_name(dev), reps=a.reps, warmup=a.warmup, inner=a.inner,
               timing="wall clock between synchronisations over `inner` calls, medians, "
                      "the two entries alternated",
               peak_bytes_per_s=PEAK_BYTES_PER_S, results=res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
