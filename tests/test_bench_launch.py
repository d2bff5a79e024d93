"""CPU suite: bench.py's multi-rank launch path. `bench.py --gpus N` started
directly spawns its N ranks (the torchrun environment contract) before any
GPU call; --dry-run runs the same launch + gather + max-over-ranks timing on
gloo with synthetic outputs, so the path the driver's SCALE run takes is
exercised without a GPU; --dump-outputs and its seeded row sample likewise."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None, timeout=240):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e,
                          capture_output=True, text=True, timeout=timeout)


def _json_lines(stdout):
    return [json.loads(x) for x in stdout.splitlines() if x.startswith("{")]


def test_gpus2_spawns_two_ranks():
    r = _run(["--gpus", "2", "--dry-run", "--steps", "3", "--warmup", "1", "--B", "512"])
    assert r.returncode == 0, r.stderr
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout          # rank 0 only
    d = lines[0]
    assert d["n_gpus"] == 2 and d["dry_run"] is True
    assert d["config"]["B_per_gpu"] == 512 and d["config"]["B_total"] == 1024
    assert d["gathered"] == {"swarms": 1024, "status_records": 1024}
    assert d["stats"]["swarms"] == 1024
    assert d["scaling"] == "weak"


def test_gpus4_c4_shard_sizes():
    r = _run(["--gpus", "4", "--dry-run", "--config", "c4", "--steps", "2", "--warmup", "1"])
    assert r.returncode == 0, r.stderr
    d = _json_lines(r.stdout)[0]
    assert d["n_gpus"] == 4 and d["config"]["n"] == 500
    assert d["config"]["B_total"] == 4 * 2048 == d["gathered"]["swarms"]


def test_world_size_mismatch_is_an_error():
    r = _run(["--gpus", "1", "--dry-run", "--steps", "1"], env={"WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode == 2 and "WORLD_SIZE" in r.stderr


def test_graph_group_times_exactly_the_steps():
    """--graph-steps G: the timed K steps are K / G' replays of a graph of G'
    steps, G' the largest divisor of K not above G (so no step is dropped or
    added)."""
    sys.path.insert(0, ROOT)
    import bench
    assert bench.graph_group(10, 20) == 10
    assert bench.graph_group(10, 25) == 5
    assert bench.graph_group(10, 7) == 7
    assert bench.graph_group(10, 13) == 1
    assert bench.graph_group(1, 20) == 1
    assert bench.graph_group(0, 20) == 1
    for K in range(1, 60):
        for G in range(0, 15):
            g = bench.graph_group(G, K)
            assert K % g == 0 and 1 <= g <= max(1, G)


def test_dump_outputs_dry_run(tmp_path):
    """--dump-outputs writes the gathered outputs of the last step as float
    .npy files, the status records field by field; --full is accepted."""
    import numpy as np
    d = tmp_path / "dump"
    r = _run(["--gpus", "1", "--dry-run", "--steps", "2", "--warmup", "1", "--B", "64", "--full",
              "--dump-outputs", str(d)])
    assert r.returncode == 0, r.stderr
    line = _json_lines(r.stdout)[0]
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    P = np.load(d / "P_out.npy")
    assert P.dtype == np.float32 and P.shape == (64, 100)
    assert (P == np.arange(100, dtype=np.float32)).all()
    assert (np.load(d / "sample_rows.npy") == np.arange(64)).all()
    eff = np.load(d / "status_eff_rounds.npy")
    assert eff.dtype == np.float32 and (eff == 3).all()
    assert np.load(d / "status_flags.npy").dtype == np.float64
    assert (np.load(d / "status_margin.npy") == np.float32(0.5)).all()
    total = sum(f.stat().st_size for f in d.iterdir())
    assert total <= 64 << 20


def test_dump_outputs_sample_is_fixed(tmp_path, monkeypatch):
    """Above the byte budget a sorted sample of rows is written, the same
    rows for the same seed, and every array holds those rows."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    B = 1000
    x = torch.arange(B * 6, dtype=torch.float64).reshape(B, 2, 3)
    k = torch.arange(B, dtype=torch.int32)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 100 * (8 + 48 + 8))
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), {"x": x, "k": k}, seed=5)
    bench.dump_outputs(str(tmp_path / "c"), {"x": x, "k": k}, seed=6)
    rows = np.load(tmp_path / "a" / "sample_rows.npy")
    assert rows.shape == (100,) and (np.diff(rows) > 0).all()
    assert (rows == np.load(tmp_path / "b" / "sample_rows.npy")).all()
    assert not (rows == np.load(tmp_path / "c" / "sample_rows.npy")).all()
    xa, ka = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "a" / "k.npy")
    assert xa.dtype == np.float64 and ka.dtype == np.float64
    assert (ka == rows).all() and (xa == x.numpy()[rows.astype(int)]).all()
    assert (xa == np.load(tmp_path / "b" / "x.npy")).all()
