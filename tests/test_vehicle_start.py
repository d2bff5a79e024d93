"""CPU suite of acl_vehicle_start_batch (one vehicle's auction start, added
within ABI 11): the struct layout, the host argument errors (no GPU: every
call below fails its checks before anything is launched) and the Python
wrapper's validation."""
import ctypes as ct
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_FIELDS = ("V", "S", "fidx", "vehid", "qidx", "q", "Pt", "Rt", "price", "who", "task", "flags")

_LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "aclswarm_amd.h"
#define P(f) printf(#f " %zu\n", offsetof(acl_vehicle_start_args_t, f));
int main(void) {
  printf("sizeof %zu abi %d\n", sizeof(acl_vehicle_start_args_t), ACL_ABI_VERSION);
  P(V) P(S) P(fidx) P(vehid) P(qidx) P(q) P(Pt) P(Rt) P(price) P(who) P(task) P(flags)
  return 0;
}
"""


def test_vehicle_start_struct_layout_matches_ctypes(tmp_path):
    from aclswarm_amd import _lib as L
    src = tmp_path / "layout.c"
    src.write_text(_LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split("\n")
    head = out[0].split()
    assert int(head[1]) == ct.sizeof(L.VehicleStartArgs)
    assert int(head[3]) == L.ABI_VERSION == 11  # an added symbol: the ABI number stays
    seen = []
    for line in out[1:]:
        if line:
            f, off = line.split()
            assert getattr(L.VehicleStartArgs, f).offset == int(off), f
            seen.append(f)
    assert tuple(seen) == _FIELDS == tuple(f for f, _ in L.VehicleStartArgs._fields_)


def _args(L, **kw):
    """Every pointer a dummy non-null address (never dereferenced)."""
    a = L.VehicleStartArgs()
    a.V, a.S = 2, 2
    for f in _FIELDS[2:]:
        setattr(a, f, 0x1000)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_vehicle_start_argument_errors_without_gpu():
    from aclswarm_amd import _lib as L
    lib = L.lib()
    call = lib.acl_vehicle_start_batch

    def table(n=10, F=1, p=0x1000, adj=0x1000):
        return L.Formations(n, F, p, adj, None, None, 9, None)

    def fails(F, a, text):
        rc = call(ct.byref(F) if F is not None else None,
                  ct.byref(a) if a is not None else None, None)
        assert rc != 0
        msg = lib.acl_last_error()
        assert b"acl_vehicle_start_batch" in msg and text in msg, msg

    fails(None, _args(L), b"null argument")
    fails(table(), None, b"null argument")
    fails(table(n=0), _args(L), b"n out of range")
    fails(table(n=513), _args(L), b"n out of range")
    fails(table(), _args(L, V=-1), b"V < 0")
    fails(table(), _args(L, S=-1), b"S < 0")
    fails(table(F=0), _args(L), b"formation table is empty")
    fails(table(p=None), _args(L), b"NULL")
    fails(table(adj=None), _args(L), b"NULL")
    for f in ("fidx", "vehid", "q", "Pt", "Rt", "flags"):
        fails(table(), _args(L, **{f: None}), b"NULL")
    # price / who / task: all or none
    for f in ("price", "who", "task"):
        fails(table(), _args(L, **{f: None}), b"all given or all NULL")
        two = {g: None for g in ("price", "who", "task") if g != f}
        fails(table(), _args(L, **two), b"all given or all NULL")
    # no qidx: snapshot k of vehicle k needs S >= V
    fails(table(), _args(L, qidx=None, S=1), b"S < V")
    # an empty batch is no error, whatever else is in the struct
    a = L.VehicleStartArgs()
    assert call(ct.byref(table()), ct.byref(a), None) == 0
    assert call(ct.byref(table(F=0)), ct.byref(_args(L, V=0)), None) == 0


class _Table:
    """What engine.vehicle_start reads of a FormationTable before it runs."""

    def __init__(self, n, device):
        self.n = n
        self.F = 1
        self.p = torch.zeros((1, n, 3), dtype=torch.float64, device=device)

    def struct(self):
        raise AssertionError("vehicle_start reached the native call")


def _good(n, V, S, dev):
    return dict(fidx=torch.zeros(V, dtype=torch.int32, device=dev),
                vehid=torch.zeros(V, dtype=torch.int32, device=dev),
                q=torch.zeros((S, n, 3), dtype=torch.float64, device=dev),
                Pt=torch.zeros((V, n), dtype=torch.int16, device=dev))


def test_engine_vehicle_start_validates_before_anything_runs(monkeypatch):
    """Each malformed argument raises ValueError before the library is loaded
    or anything is allocated (host and meta tensors: no device is touched;
    the table's struct() and the library loader would fail the test)."""
    from aclswarm_amd import _lib as L
    from aclswarm_amd import engine

    def no_lib():
        raise AssertionError("vehicle_start loaded the library")
    monkeypatch.setattr(L, "lib", no_lib)
    n, V, S = 5, 4, 4
    cpu, meta = torch.device("cpu"), torch.device("meta")
    g = _good(n, V, S, cpu)
    bad = [
        ("fidx", g["fidx"].to(torch.int64)),                       # dtype
        ("vehid", g["vehid"].to(torch.int16)),
        ("q", g["q"].to(torch.float32)),
        ("Pt", g["Pt"].to(torch.int32)),
        ("qidx", torch.zeros(V, dtype=torch.int64)),
        ("fidx", torch.zeros(V + 1, dtype=torch.int32)),           # shape
        ("vehid", torch.zeros((V, 1), dtype=torch.int32)),
        ("q", torch.zeros((S, n + 1, 3), dtype=torch.float64)),
        ("q", torch.zeros((S, n), dtype=torch.float64)),
        ("Pt", torch.zeros((V, n + 1), dtype=torch.int16)),
        ("qidx", torch.zeros(V + 2, dtype=torch.int32)),
        ("Pt", torch.zeros((n, V), dtype=torch.int16).t()),        # not contiguous
        ("q", torch.zeros((S, 3, n), dtype=torch.float64).transpose(1, 2)),
        ("fidx", torch.zeros(2 * V, dtype=torch.int32)[::2]),
        ("fidx", torch.zeros(V, dtype=torch.int32, device=meta)),  # mixed devices
        ("q", torch.zeros((S, n, 3), dtype=torch.float64, device=meta)),
        ("Pt", torch.zeros((V, n), dtype=torch.int16, device=meta)),
        ("qidx", torch.zeros(V, dtype=torch.int32, device=meta)),
    ]
    for name, t in bad:
        kw = dict(g)
        kw[name] = t
        with pytest.raises(ValueError, match=name):
            engine.vehicle_start(_Table(n, cpu), **kw)
    # S < V with qidx None ...
    kw = dict(g)
    kw["q"] = torch.zeros((V - 1, n, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match="S = 3 < V = 4"):
        engine.vehicle_start(_Table(n, cpu), **kw)
    # ... is fine once qidx says which snapshot: the next check speaks
    with pytest.raises(ValueError, match="CUDA"):
        engine.vehicle_start(_Table(n, cpu), qidx=torch.zeros(V, dtype=torch.int32), **kw)
    # the table on another device than the vehicles
    with pytest.raises(ValueError, match="formation table"):
        engine.vehicle_start(_Table(n, meta), **g)
    # consistent tensors that are not on a CUDA device
    with pytest.raises(ValueError, match="CUDA"):
        engine.vehicle_start(_Table(n, cpu), **g)
    with pytest.raises(ValueError, match="CUDA"):
        engine.vehicle_start(_Table(n, meta), want_bid=False, **_good(n, V, S, meta))
    # not tensors at all
    with pytest.raises(ValueError, match="torch tensor"):
        engine.vehicle_start(_Table(n, cpu), np.zeros(V, np.int32), g["vehid"], g["q"], g["Pt"])
