"""bench.py's driver contract on the CPU: ONE JSON line from rank 0 with the required keys, for one
process and for a 2-rank torchrun over gloo (rendezvous on 127.0.0.1)."""
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config")
CONFIG_KEYS = ("model", "global_batch", "seq_len", "parallelism")


def _json_lines(out: str):
    return [json.loads(l) for l in out.splitlines() if l.startswith("{") and '"metric"' in l]


def _check(d, n):
    for k in KEYS:
        assert k in d, k
    for k in CONFIG_KEYS:
        assert k in d["config"], k
    assert d["n_gpus"] == n and d["config"]["parallelism"] == f"dp{n}"
    assert d["metric"] == "train_rows_per_sec" and d["higher_is_better"] is True
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 1 and d["warmup"] == 0
    assert abs(d["value"] - d["config"]["global_batch"] * 1000.0 / d["ms_per_step"]) < 1e-3 * d["value"] + 1e-6


def _env():
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return env


def test_bench_single_process_json_line():
    r = subprocess.run([sys.executable, "bench.py", "--steps", "1", "--warmup", "0", "--rows", "600"], cwd=ROOT,
                       env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout
    _check(lines[0], 1)


def test_bench_plain_run_stops_after_the_clock_and_full_adds_the_rest(tmp_path):
    """A plain run reports the timed steps only; ``--full`` adds the held-out scores of the untimed
    evaluated fit; ``--dump-outputs`` writes the last timed step's outputs as float32 / float64
    ``.npy`` files below 64 MB, identical from run to run (seeded inputs, deterministic host path)."""
    import numpy as np

    def run(*extra):
        r = subprocess.run([sys.executable, "bench.py", "--steps", "2", "--warmup", "0", "--rows", "300", *extra],
                           cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = _json_lines(r.stdout)
        assert len(lines) == 1, r.stdout
        return lines[0]

    plain = run("--dump-outputs", str(tmp_path / "a"))
    full = run("--full", "--dump-outputs", str(tmp_path / "b"))
    assert "auroc" not in plain and "average_precision" not in plain
    assert 0.5 < full["auroc"] <= 1.0 and 0.0 < full["average_precision"] <= 1.0
    for d in (plain, full):
        assert d["steps"] == 2 and len(d["diag"]["step_ms"]) == 2
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in d, k
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"selected.npy", "final_coef.npy", "final_intercept.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64), (n, x.dtype)
        assert x.size > 0 and np.isfinite(x).all(), n
        assert np.array_equal(x, y), n
        total += os.path.getsize(tmp_path / "a" / n)
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "selected.npy").sum() == 17


def test_dump_outputs_samples_large_arrays_within_the_budget(tmp_path, monkeypatch):
    """An output above its share of the byte budget is written as a fixed, seeded sample of its
    rows (the same rows in every run) with the row indices next to it; small outputs are whole."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1 << 16)
    big = torch.arange(50000, dtype=torch.float32)[:, None] * torch.ones(1, 3)
    arrays = {"big": big, "small": np.arange(7, dtype=np.int32), "scalar": torch.tensor(2.5, dtype=torch.float64)}
    bench._dump_outputs(str(tmp_path / "a"), arrays)
    bench._dump_outputs(str(tmp_path / "b"), arrays)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["big.npy", "big.rows.npy", "scalar.npy", "small.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 1 << 16
    x, rows = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "a" / "big.rows.npy")
    assert x.dtype == np.float32 and rows.dtype == np.float64 and 100 < x.shape[0] < 50000
    assert np.array_equal(x[:, 0], rows) and np.all(np.diff(rows) > 0)
    assert np.load(tmp_path / "a" / "small.npy").dtype == np.float64
    assert float(np.load(tmp_path / "a" / "scalar.npy")) == 2.5
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f


def test_bench_torchrun_two_ranks_one_json_line():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "2", "--steps", "1",
           "--warmup", "0", "--rows", "600"]
    r = subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout
    _check(lines[0], 2)
