"""bench.py on the GPU at a toy size (C3's shape, B = 96 swarms), run in
process: a plain run prints the headline line only and --dump-outputs writes
what its last timed step computed -- the same arrays on a second run with
the same arguments, and what engine.solve gives for the same seeded
workload; --full adds the per-kernel, margin, probe and CPU-baseline legs,
whose parity sample must be exact."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

from aclswarm_amd import engine, workload  # noqa: E402

pytestmark = pytest.mark.gpu
B, N, SEED = 96, 100, 11
PLAIN_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "gen_s"}
FULL_KEYS = {"margin", "ca_probe", "stats", "cpu_baseline"}


def _bench(monkeypatch, capsys, *extra):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
                                      "--B", str(B), "--seed", str(SEED)] + list(extra))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert bench.main() == 0
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_run_and_dump(monkeypatch, capsys, tmp_path):
    line = _bench(monkeypatch, capsys, "--dump-outputs", str(tmp_path / "a"))
    assert set(line) == PLAIN_KEYS
    assert line["steps"] == 3 and line["warmup"] == 1 and line["dtype"] == "f64"
    assert line["unit"] == "solves/s" and line["higher_is_better"] is True
    assert line["value"] == pytest.approx(B / (line["ms_per_step"] * 1e-3))
    assert "kernels" not in line["roofline"] and line["roofline"]["frac"] > 0
    a = _load(tmp_path / "a")
    assert set(a) == {"P_out", "u", "u_safe", "ca_flag", "sample_rows", "status_flags",
                      "status_eff_rounds", "status_rounds", "status_n_invalid", "status_n_ca",
                      "status_margin"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert (a["sample_rows"] == np.arange(B)).all()
    # the same arguments: the same inputs, so the same outputs
    _bench(monkeypatch, capsys, "--dump-outputs", str(tmp_path / "b"))
    b = _load(tmp_path / "b")
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    # and they are the timed path's outputs: bench.py's workload solved directly
    # (the headline does not track the decision margin)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED)
    w = workload.simform_workload(B, N, gen, dev, L=40.0, complete=False, planes=5, seed0=0)
    T = engine.FormationTable(w["n"], w["p"], w["bits"], w["gains"], w["gain_off"], w["planes"])
    out = engine.solve(T, w["fidx"], w["q"], w["vel"], w["P_in"], margin=False)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(a["P_out"], out["P_out"].cpu().numpy().astype(np.float32))
    np.testing.assert_array_equal(a["u"], out["u"].cpu().numpy())
    np.testing.assert_array_equal(a["u_safe"], out["u_safe"].cpu().numpy())
    np.testing.assert_array_equal(a["ca_flag"], out["ca_flag"].cpu().numpy().astype(np.float32))
    st = engine.status_to_numpy(out["status"])
    for f in st.dtype.names:
        np.testing.assert_array_equal(a["status_" + f], st[f].astype(a["status_" + f].dtype))
    # every swarm adopted a permutation of 0..n-1
    assert (np.sort(a["P_out"], axis=1) == np.arange(N)).all()
    assert np.isfinite(a["u_safe"]).all()


def test_full_run_adds_the_other_legs(monkeypatch, capsys):
    line = _bench(monkeypatch, capsys, "--full", "--cpu-budget", "1")
    assert set(line) == PLAIN_KEYS | FULL_KEYS
    assert set(line["roofline"]["kernels"]) == {"auction", "gain", "ca"}
    assert line["margin"]["value_margin_on"] > 0 and line["stats"]["valid"] == B
    assert line["ca_probe"]["ca_active_swarms"] > 0
    ps = line["cpu_baseline"]["parity_sample"]
    assert ps["assignments_bit_exact"] and ps["status_and_margin_exact"]
    assert ps["u_safe_max_rel_err"] <= 1e-5
