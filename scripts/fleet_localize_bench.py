#!/usr/bin/env python3
"""Time of fleet localization (acl_fleet_localize_batch), two ways, and of the
own-estimate auction entry beside the lossy one.

B swarms of n vehicles (fleet_auction_bench's formations, identity rows) run
`rounds` gossip rounds from fresh trackers:

  kernel  one acl_fleet_localize_batch call (engine.FleetLocalization);
  torch   the same rounds written with torch ops on the device, which was the
          only way to run them before: per round one gather of the subscribed
          senders' stamps, a max over them, and a where (and a gather of the
          winners' positions); with loss, the link hash in int64 arithmetic.
          Its stamps and positions must equal the kernel's.

Each at loss 0 (the lossless instantiation) and at every --loss threshold on
every link. Then one clean auction (every link 1 tick, loss 0, START from one
snapshot, to quiescence) on

  lossy   acl_fleet_lossy_auction_batch from q, and
  est     acl_fleet_est_auction_batch from est broadcast from q,

whose final tables must be equal. All are timed wall-clock between
synchronisations after a warm-up, alternated in one session, medians reported.
Writes one JSON document (--out)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from aclswarm_amd import _lib as L  # noqa: E402
from aclswarm_amd import engine  # noqa: E402
from fleet_auction_bench import make_case, timed  # noqa: E402

M32 = 0xFFFFFFFF


def _mix(h, word):
    h = ((h ^ word) * 0x9E3779B1) & M32
    return h ^ (h >> 15)


def link_hash_t(seed, w, u, pub, it):
    """The header's link_hash on int64 tensors (values below 2^32)."""
    h = _mix(_mix(_mix(seed, (w << 16) | u), pub), it)
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


class TorchRounds:
    """The rounds with torch ops (identity rows: vehicle w hears adj[w])."""

    def __init__(self, adj, fidx, q, loss, seed0):
        dev = q.device
        B, n = q.shape[0], q.shape[1]
        a = torch.from_numpy(adj.astype("int64")).to(dev)[fidx.long()]  # [B][n][n]
        D = int(a.sum(dim=2).max())
        # the subscribed senders of every receiver, ascending, padded with the receiver
        order = torch.argsort(1 - a, dim=2, stable=True)[:, :, :D]
        self.valid = torch.gather(a, 2, order) != 0
        w = torch.arange(n, device=dev).view(1, n, 1).expand(B, n, D)
        self.idx = torch.where(self.valid, order, w).contiguous()
        self.q, self.B, self.n, self.D, self.loss = q, B, n, D, int(loss)
        self.seed = ((torch.arange(B, device=dev) + seed0) & M32).view(B, 1, 1)
        self.w = w
        self.diag = torch.arange(n, device=dev)

    def run(self, rounds):
        B, n, D, dev = self.B, self.n, self.D, self.q.device
        stamp = torch.zeros((B, n, n), dtype=torch.int32, device=dev)
        est = torch.zeros((B, n, n, 3), dtype=torch.float64, device=dev)
        gi = self.idx.unsqueeze(-1).expand(B, n, D, n)
        for r in range(rounds):
            stamp[:, self.diag, self.diag] = r + 1
            est[:, self.diag, self.diag] = self.q
            ok = self.valid
            if self.loss:
                h = link_hash_t(self.seed, self.w, self.idx, r, M32)
                lost = (h >> 16) < self.loss if self.loss != 0xFFFF else torch.ones_like(ok)
                ok = ok & ~lost
            cand = stamp.unsqueeze(1).expand(B, n, n, n).gather(2, gi)  # [B][w][d][i]
            cand = torch.where(ok.unsqueeze(-1), cand, torch.zeros_like(cand))
            best = cand.amax(dim=2)
            # the first (lowest id) of the senders that hold the largest stamp
            d = (cand == best.unsqueeze(2)).to(torch.uint8).argmax(dim=2)
            take = best > stamp
            u = torch.gather(self.idx, 2, d)  # [B][w][i]
            moved = est.gather(1, u.unsqueeze(-1).expand(B, n, n, 3))
            est = torch.where(take.unsqueeze(-1), moved, est)
            stamp = torch.where(take, best, stamp)
        return stamp, est


def bench(n, B, F, rounds, losses, reps, warmup, dev):
    T, adj, fidx, q = make_case(n, B, F, 1000 + n, dev)
    out = dict(n=n, B=B, formations=F, rounds=rounds, gossip=[])
    for loss in [0] + list(losses):
        tr = TorchRounds(adj, fidx, q, loss, 1)

        def kernel():
            loc = engine.FleetLocalization(T, fidx, loss=loss or None,
                                           loss_seed=1 if loss else None)  # fresh (not timed)
            dt, _ = timed(lambda: loc.run(rounds, q), dev)
            return dt, loc

        tk, tt = [], []
        for r in range(warmup + reps):
            dk, loc = kernel()
            dtt, (st, es) = timed(lambda: tr.run(rounds), dev)
            if r >= warmup:
                tk.append(dk)
                tt.append(dtt)
        assert bool((st == loc.stamp).all()), "the torch rounds and the kernel disagree (stamp)"
        assert bool((es.view(torch.int64) == loc.est.view(torch.int64)).all()), "... (est)"
        stt = loc.status()
        mk, mt = statistics.median(tk), statistics.median(tt)
        out["gossip"].append(dict(
            loss=loss, kernel_ms=mk * 1e3, kernel_ms_all=[x * 1e3 for x in tk],
            kernel_us_per_round=mk * 1e6 / rounds, torch_ms=mt * 1e3,
            torch_ms_all=[x * 1e3 for x in tt], torch_us_per_round=mt * 1e6 / rounds,
            torch_over_kernel=mt / mk, results_equal=True, d_max=tr.D,
            n_unknown_max=int(stt["n_unknown"].max()), max_age_max=int(stt["max_age"].max()),
            lost=int(loc.n_lost.sum().item()) if loss else 0))
        del tr
    # the own-estimate entry beside the lossy one: one clean auction
    d_max = int(adj.sum(axis=2).max())
    ticks = 2 * n * d_max + 8
    cmd = torch.full((B, n), L.FLEET_START, dtype=torch.uint8, device=dev)
    est = q.unsqueeze(1).expand(B, n, n, 3).contiguous()

    def auction(own):
        f = engine.FleetAuction(T, fidx, latency=1, loss=0, loss_seed=1)
        f.ws = torch.zeros(f.workspace_bytes(), dtype=torch.uint8, device=dev)
        if own:
            dt, _ = timed(lambda: f.run(ticks, cmd=cmd, est=est), dev)
        else:
            dt, _ = timed(lambda: f.run(ticks, q=q, cmd=cmd), dev)
        return dt, f

    tl, te = [], []
    for r in range(warmup + reps):
        dl, fl = auction(False)
        de, fe = auction(True)
        if r >= warmup:
            tl.append(dl)
            te.append(de)
    assert (fe.status()["n_open"] == 0).all()
    assert bool((fe.final_who == fl.final_who).all()) and bool((fe.ws == fl.ws).all())
    ml, me = statistics.median(tl), statistics.median(te)
    out["auction"] = dict(ticks_run_max=int(fe.status()["ticks_run"].max()), lossy_ms=ml * 1e3,
                          lossy_ms_all=[x * 1e3 for x in tl], est_ms=me * 1e3,
                          est_ms_all=[x * 1e3 for x in te], est_over_lossy=me / ml,
                          tables_and_workspace_equal=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20x4096,100x256", help="n x B, comma-separated")
    ap.add_argument("--formations", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=64)
    ap.add_argument("--loss", default="4096", help="thresholds 1..65535, comma-separated")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_localize",
                                                  "rounds.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = []
    for s in a.shapes.split(","):
        n, B = (int(x) for x in s.split("x"))
        r = bench(n, B, a.formations, a.rounds, [int(x) for x in a.loss.split(",") if x],
                  a.reps, a.warmup, dev)
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
