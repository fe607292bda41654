"""Pin the driver-facing bench.py contract: one JSON line on stdout with
the schema the round-end harness parses (metric/config per BASELINE.json).
Runs the CPU smoke path (seq clamps small off-GPU) — the schema is the
same object the MI355X run prints."""

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLAIN_ARGS = ["--steps", "3", "--warmup", "1"]


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    """One plain bench.py process, shared: (completed process, dump dir)."""
    dump = tmp_path_factory.mktemp("bench") / "dump"
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py")] + PLAIN_ARGS
        + ["--dump-outputs", str(dump)],
        capture_output=True, text=True, timeout=600, cwd=REPO)
    return r, dump


def test_bench_json_contract(plain_run):
    r, _ = plain_run
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config"):
        assert key in out, key
    assert out["metric"] == "attention tokens/sec"
    assert out["unit"] == "tokens/s"
    assert out["n_gpus"] == 1 and out["steps"] == 3 and out["warmup"] == 1
    assert out["higher_is_better"] is True and out["scaling"] == "weak"
    assert out["dtype"] == "bf16" and out["data"] == "synthetic"
    assert out["value"] > 0 and out["ms_per_step"] > 0
    cfg = out["config"]
    for key in ("model", "global_batch", "seq_len", "num_heads",
                "head_dim", "parallelism"):
        assert key in cfg, key
    assert cfg["num_heads"] == 32 and cfg["head_dim"] == 128
    assert cfg["parallelism"] == "sp1"
    # whole-job aggregate: tokens attended / s == B*seq*steps / elapsed
    expect = (cfg["global_batch"] * cfg["seq_len"] * out["steps"]
              / (out["ms_per_step"] * out["steps"] / 1e3))
    assert abs(expect - out["value"]) / out["value"] < 1e-6


def test_dump_outputs_samples_large_output(tmp_path):
    """An output over the 64 MB budget is written as a fixed, seeded sample:
    the same elements every time, well under the budget."""
    import numpy as np
    import torch

    sys.path.insert(0, REPO)
    import bench

    n = bench._DUMP_MAX_ELEMS + 1
    out = torch.arange(n, dtype=torch.int32).reshape(1, 1, n, 1)
    bench.dump_outputs(out, str(tmp_path / "a"))
    bench.dump_outputs(out, str(tmp_path / "b"))
    a = np.load(tmp_path / "a" / "out.npy")
    b = np.load(tmp_path / "b" / "out.npy")
    assert a.dtype == np.float32 and a.shape == (bench._DUMP_SAMPLE_ELEMS,)
    assert a.nbytes <= 64 << 20
    np.testing.assert_array_equal(a, b)
    # spread over the whole output, not a prefix of it
    assert a.max() > 0.99 * n and a.min() < 0.01 * n


def test_bench_dump_outputs_reproducible(plain_run, tmp_path, capsys):
    """--dump-outputs writes the last timed step's output as float32
    DIR/out.npy; the inputs are seeded, so a second run with the same
    arguments (here in-process, and with --full, which adds nothing to a
    plain run's dump) agrees with the shared plain process."""
    import numpy as np

    sys.path.insert(0, REPO)
    import bench

    r, dump = plain_run
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(dump)) == ["out.npy"]
    a = np.load(dump / "out.npy")
    assert a.dtype == np.float32 and a.shape == (1, 32, 1, 128)
    assert np.isfinite(a).all() and np.abs(a).max() > 0

    bench.main(PLAIN_ARGS + ["--full", "--dump-outputs", str(tmp_path)])
    line, = [l for l in capsys.readouterr().out.splitlines()
             if l.startswith("{")]
    assert json.loads(line)["steps"] == 3
    b = np.load(tmp_path / "out.npy")
    # same seeded inputs, same build, and no atomics in the kernels (the
    # split-KV partials merge in a fixed order): bit-identical
    assert b.dtype == a.dtype and b.shape == a.shape
    np.testing.assert_array_equal(a, b)


