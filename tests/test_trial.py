"""CPU suite for batched Monte-Carlo trials (acl_trial_batch):
the supervisor restatement (oracle/trial_oracle.py) on scripted signals
against supervisor.py's rules, a whole CPU trial on swarm6_3d, the cases of
the GPU parity tests above one wave (tests/trial_cases.py: their gains, and
that each still reaches the edge it is for), engine.Trial's argument checks,
and the trial ABI (struct layout, defaults, argument errors) without a GPU."""
import ctypes as ct
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import trial_cases as C
import trial_oracle as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tp(**kw):
    tp = T.default_params()
    tp["ep"] = dict(tp["ep"], bufflen=3)
    tp.update(hover_wait=0.1, formation_received_wait=0.04, converged_wait=0.04, **kw)
    return tp


def test_supervisor_scripted_cycle():
    """HOVERING -(HOVER_WAIT)-> WAITING -(assignment)-> FLYING -(wait, then a
    full window of small |u|)-> IN_FORMATION -(CONVERGED_WAIT)-> HOVERING ...
    -> COMPLETE, with supervisor.py's timer arithmetic: a state entered at a
    tick runs its first body at the next tick with timer_ticks = 0, and
    has_elapsed(s) is timer_ticks / 50 >= s."""
    n, K = 3, 2
    s = T.Supervisor(n, K, _tp())
    q = np.zeros((n, 3))
    zero, big = np.zeros(n), np.full(n, 5.0)
    no = np.zeros(n, bool)
    seq = []
    for tick in range(60):
        step = 2 * tick
        if s.state == T.WAITING and s.timer_ticks == 1:
            s.assignment_msg()
        speeds = big if tick < 20 else zero
        s.tick(step, speeds, no, q)
        seq.append(s.state)
        if s.done_step >= 0:
            break
    # hover_wait 0.1 s = 5 ticks: the 6th tick (timer 5) leaves HOVERING
    assert seq[:5] == [T.HOVERING] * 5 and seq[5] == T.WAITING
    assert s.formation == K - 1 and s.state == T.COMPLETE and s.done_step >= 0
    r = s.record()
    assert r["assignments"] == [1, 1] and all(t > 0 for t in r["time"])
    assert r["time_avoidance"] == [0.0, 0.0]


def test_supervisor_gridlock_and_release():
    """FLYING -> GRIDLOCK when a vehicle's CA flag is on for > 95% of a full
    window; has_left_gridlock needs a full window again (next_state clears the
    buffers); time_avoidance keeps the gridlock's duration."""
    n = 2
    s = T.Supervisor(n, 1, _tp(gridlock_timeout=100.0))
    s.state, s.formation, s.logging, s.timer_ticks = T.FLYING, 0, True, 10
    q = np.zeros((n, 3))
    on = np.array([True, False])
    big = np.full(n, 5.0)
    step = 0
    for _ in range(3):
        s.tick(step, big, on, q)
        step += 2
    assert s.state == T.GRIDLOCK and s.t_grid == 4
    for _ in range(2):          # the window refills: no decision yet
        s.tick(step, big, ~on & on, q)
        step += 2
        assert s.state == T.GRIDLOCK
    s.tick(step, big, ~on & on, q)
    assert s.state == T.FLYING
    assert s.time_avoidance[0] == (step - 4) * 0.01


def test_cpu_trial_swarm6_runs_to_an_end():
    pts, adj, gains, q0 = H.swarm6()
    forms = list(zip(pts, adj, gains))
    tp = _tp(settle_steps=10)
    tp["ep"] = dict(tp["ep"], auction_every=20, bufflen=10)
    q = q0.copy()
    q[:, 2] = 1.0
    t, qf, vf, states = T.run_trial(q, np.zeros_like(q), [0, 1, 2], forms, tp, 3000)
    assert t.done and t.sup.state in (T.COMPLETE, T.TERMINATE)
    assert np.isfinite(qf).all()
    assert t.counts["auctions"] > 0


# -- the cases of the GPU parity tests above one wave (tests/trial_cases.py) --

@pytest.mark.parametrize("n", [5, 65])
def test_closed_form_gains(n):
    """Zero row sums, the formation in the kernel, the reference's block
    structure [a b 0; -b a 0; 0 0 c] on every edge (and on the diagonal)."""
    p, _ = C.formation_points(n)
    G = C.closed_form_gains(p)
    assert G.shape == (3 * n, 3 * n)
    assert np.abs(G.reshape(3 * n, n, 3).sum(axis=1)).max() < 1e-12
    assert np.abs(G @ p.ravel()).max() < 1e-10
    Gb = G.reshape(n, 3, n, 3).transpose(0, 2, 1, 3)       # [i][j] 3 x 3
    assert (Gb[..., 0, 0] == Gb[..., 1, 1]).all() and (Gb[..., 0, 1] == -Gb[..., 1, 0]).all()
    assert (Gb[..., :2, 2] == 0).all() and (Gb[..., 2, :2] == 0).all()
    off = ~np.eye(n, dtype=bool)
    assert (np.abs(Gb[off][:, 0, 0]) > 0).any() and (np.abs(Gb[off][:, 0, 1]) > 0).any()
    assert (np.abs(Gb[off][:, 2, 2]) > 0).any()
    # the kernel also holds the formation turned and scaled in xy: what the
    # swarm flies into
    z = (p[:, 0] + 1j * p[:, 1]) * (0.7 - 0.4j)
    pr = np.c_[z.real, z.imag, 2.0 * p[:, 2] + 1.0]
    assert np.abs(G @ pr.ravel()).max() < 1e-10
    # negative semidefinite: the flight is stable
    assert np.linalg.eigvalsh(0.5 * (G + G.T)).max() < 1e-12


def _fly(case, steps):
    """One case alone on the CPU restatement, with the batch's parameters;
    per-step states, CA flags, commands and the assignment counts."""
    tp = C.oracle_params(case)
    forms = list(zip(case["pts"], case["adj"], case["gains"]))
    out = []
    for b in range(case["q"].shape[0]):
        t = T.TrialSwarm(case["q"].shape[1], case["fseq"][b], forms, tp)
        q, vel = case["q"][b].copy(), case["vel"][b].copy()
        states, us, cas, rise = [], [], [], -1
        for k in range(steps):
            q, vel, u, ca = t.step(k, q, vel)
            states.append(t.sup.state); us.append(u); cas.append(ca)
            if rise < 0 and max(t.sup.assignments) >= 2:
                rise = k
            if t.done:
                break
        out.append(dict(t=t, states=np.array(states), u=np.array(us), ca=np.array(cas),
                        rise=rise))
    return out, tp


def _check_cases_on_cpu(n, steps, steps_e):
    case = C.batch([C.calm(n), C.late_last(n), C.pair_last(n), C.reassign(n)])
    (a, b, c, d), tp = _fly(case, steps)
    L, every = tp["ep"]["bufflen"], tp["ep"]["sample_every"]
    for x in (a, b):
        assert x["t"].sup.state == T.COMPLETE and x["t"].done
        assert not x["ca"].any() and (x["t"].state.P == np.arange(n)).all()
    # late_last: the last vehicle alone vetoes has_converged for a window
    in_a, in_b = (C.first_step(x["states"], T.IN_FORMATION) for x in (a, b))
    assert in_a > 0 and in_b >= in_a + 2 * L, (in_a, in_b)
    assert b["states"][in_a] == T.FLYING
    u = b["u"][in_a - every * (L - 1):in_a + 1:every]
    m = np.sqrt((u * u).sum(axis=2)).mean(axis=0)
    thr = tp["ep"]["orig_zero_vel_thr"]
    assert (m[:n - 1] < thr).all() and m[n - 1] >= thr, (m[:n - 1].max(), m[n - 1])
    # pair_last: the last two vehicles alone hold the collision avoidance
    s = c["t"].sup
    assert (s.state, s.last_state) == (T.TERMINATE, T.GRIDLOCK) and c["t"].done
    assert not c["ca"][:, :n - 2].any() and c["ca"][:, n - 2].any() and c["ca"][:, n - 1].any()
    assert (c["t"].state.P == np.arange(n)).all()
    # reassign: a counted assignment message within the steps of the batch
    assert 0 < d["rise"] < steps, d["rise"]
    # two_formations: a whole record
    (e,), _ = _fly(C.batch([C.two_formations(n)]), steps_e)
    r = e["t"].sup.record()
    assert r["state"] == T.COMPLETE and r["assignments"] == [1, 1] and min(r["time"]) > 0


def test_trial_cases_reach_their_ends_on_cpu():
    """What tests/test_gpu_trial.py flies at n = 65 covers its edges on the
    restatement alone (the steps are that test's)."""
    _check_cases_on_cpu(65, 240, 390)


@pytest.mark.slow
def test_trial_cases_reach_their_ends_on_cpu_n129():
    _check_cases_on_cpu(129, 246, 620)


# -- engine.Trial: the arguments ------------------------------------------

def _tables():
    import torch  # noqa: F401
    from aclswarm_amd import engine
    pts, adj, gains, _ = H.swarm6()
    return (engine.FormationTable.from_host(pts, adj, gains, device="cpu"),
            engine.FormationTable.from_host(pts, adj, gains, device="meta"))


def test_engine_trial_validates_before_anything_runs(monkeypatch):
    """Each malformed argument raises ValueError before the library is loaded
    or anything is allocated (host and meta tensors: no device is touched)."""
    import torch
    from aclswarm_amd import _lib as L
    from aclswarm_amd import engine
    Tc, Tm = _tables()

    def no_lib():
        raise AssertionError("Trial loaded the library")
    monkeypatch.setattr(L, "lib", no_lib)
    n, B, K = Tc.n, 4, 2
    meta = torch.device("meta")

    def good(dev="cpu"):
        return dict(fseq=torch.zeros((B, K), dtype=torch.int32, device=dev),
                    q=torch.zeros((B, n, 3), dtype=torch.float64, device=dev),
                    vel=torch.zeros((B, n, 3), dtype=torch.float64, device=dev))
    g = good()
    bad = [
        ("fseq", g["fseq"].to(torch.int64)),                          # dtype
        ("q", g["q"].to(torch.float32)),
        ("vel", g["vel"].to(torch.float32)),
        ("fseq", torch.zeros(B, dtype=torch.int32)),                  # shape
        ("fseq", torch.zeros((B + 1, K), dtype=torch.int32)),
        ("fseq", torch.zeros((B, 0), dtype=torch.int32)),             # K >= 1
        ("q", torch.zeros((B, n + 1, 3), dtype=torch.float64)),       # n is the table's
        ("q", torch.zeros((B, n), dtype=torch.float64)),
        ("vel", torch.zeros((B + 1, n, 3), dtype=torch.float64)),
        ("vel", torch.zeros((B, n, 2), dtype=torch.float64)),
        ("fseq", torch.zeros((K, B), dtype=torch.int32).t()),         # not contiguous
        ("q", torch.zeros((B, 3, n), dtype=torch.float64).transpose(1, 2)),
        ("vel", torch.zeros((2 * B, n, 3), dtype=torch.float64)[::2]),
        ("fseq", torch.zeros((B, K), dtype=torch.int32, device=meta)),   # mixed devices
        ("vel", torch.zeros((B, n, 3), dtype=torch.float64, device=meta)),
        ("fseq", np.zeros((B, K), np.int32)),                         # not tensors
        ("q", np.zeros((B, n, 3))),
        ("vel", None),
    ]
    for name, t in bad:
        kw = dict(g)
        kw[name] = t
        with pytest.raises(ValueError, match="Trial: " + name):
            engine.Trial(Tc, **kw)
    with pytest.raises(ValueError, match="formation table"):
        engine.Trial(Tm, **g)
    with pytest.raises(ValueError, match="formation table"):
        engine.Trial(Tc, **good(meta))
    # consistent tensors that are not on a CUDA device
    with pytest.raises(ValueError, match="CUDA"):
        engine.Trial(Tc, **g)
    with pytest.raises(ValueError, match="CUDA"):
        engine.Trial(Tm, **good(meta))


# -- ABI ------------------------------------------------------------------

_LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "aclswarm_amd.h"
#define P(T, f) printf("%s.%s %zu\n", #T, #f, offsetof(T, f));
int main(void) {
  printf("params %zu status %zu args %zu\n", sizeof(acl_trial_params_t),
         sizeof(acl_trial_status_t), sizeof(acl_trial_args_t));
  P(acl_trial_params_t, tick_rate) P(acl_trial_params_t, settle_steps)
  P(acl_trial_params_t, hover_wait) P(acl_trial_params_t, alpha)
  P(acl_trial_status_t, next_auction) P(acl_trial_status_t, done_step)
  P(acl_trial_status_t, n_auctions) P(acl_trial_status_t, n_disagree)
  P(acl_trial_status_t, per_vehicle)
  P(acl_trial_args_t, fseq) P(acl_trial_args_t, n_assign) P(acl_trial_args_t, step0)
  P(acl_trial_args_t, steps) P(acl_trial_args_t, q_hist) P(acl_trial_args_t, state_hist)
  P(acl_trial_args_t, workspace) P(acl_trial_args_t, cntrl) P(acl_trial_args_t, safety)
  P(acl_trial_args_t, tp)
  return 0;
}
"""


def test_trial_struct_layout_matches_ctypes(tmp_path):
    from aclswarm_amd import _lib as L
    src = tmp_path / "layout.c"
    src.write_text(_LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split("\n")
    sizes = out[0].split()
    assert int(sizes[1]) == ct.sizeof(L.TrialParams)
    assert int(sizes[3]) == L.TRIAL_STATUS_DTYPE.itemsize == 80
    assert int(sizes[5]) == ct.sizeof(L.TrialArgs)
    cls = {"acl_trial_params_t": L.TrialParams, "acl_trial_args_t": L.TrialArgs}
    for line in out[1:]:
        if not line:
            continue
        name, off = line.split()
        Tn, f = name.split(".")
        if Tn == "acl_trial_status_t":
            assert L.TRIAL_STATUS_DTYPE.fields[f][1] == int(off), name
        else:
            assert getattr(cls[Tn], f).offset == int(off), name


def test_trial_defaults_and_argument_errors_without_gpu():
    from aclswarm_amd import _lib as L
    lib = L.lib()
    t = L.default_trial_params()
    assert (t.tick_rate, t.settle_steps) == (50, 150)
    assert (t.hover_wait, t.assignment_timeout, t.formation_received_wait, t.converged_wait,
            t.gridlock_timeout, t.trial_timeout, t.alpha) == (5.0, 20.0, 1.0, 1.0, 90.0, 600.0, 0.98)
    assert t.ep.auction_every == 120 and t.ep.assignment == 0
    oracle = T.default_params()
    for k in ("tick_rate", "settle_steps", "hover_wait", "gridlock_timeout", "trial_timeout"):
        assert oracle[k] == getattr(t, k)
    assert lib.acl_trial_workspace_bytes(100, 16) > lib.acl_episode_workspace_bytes(100, 16)
    a = L.TrialArgs()
    a.B, a.K, a.tp = 4, 2, t
    assert lib.acl_trial_init(ct.byref(a), 6, None) != 0
    assert b"required pointer" in lib.acl_last_error()
    a.K = 0
    assert lib.acl_trial_init(ct.byref(a), 6, None) != 0
    assert b"K >= 1" in lib.acl_last_error()
    for k in [f[0] for f in L.TrialArgs._fields_ if f[1] is ct.c_void_p]:
        setattr(a, k, 16)  # non-NULL placeholders: argument checks only
    a.K = 2
    a.tp.ep.auction_latency = 3
    assert lib.acl_trial_init(ct.byref(a), 6, None) != 0
    assert b"auction_latency" in lib.acl_last_error()
    a.tp.ep.auction_latency = 0
    a.tp.ep.assignment = 7
    assert lib.acl_trial_init(ct.byref(a), 6, None) != 0
    assert b"assignment" in lib.acl_last_error()
