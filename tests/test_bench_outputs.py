"""bench.py's plain run and ``--dump-outputs``: the plain line carries the headline only, and the dump holds what the
last timed step computed -- the same arrays whether or not ``--full`` measured everything else around it."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pred", "target", "loss", "params", "buffers")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


class _Opt:
    def __init__(self, n):
        self.flat_param = torch.arange(n, dtype=torch.float32)


def test_dump_outputs_writes_float32_arrays(tmp_path):
    bench = _bench()
    model = torch.nn.BatchNorm1d(4)
    model.running_mean.fill_(0.5)
    res = {"pred": torch.randn(5, 3, 3), "target": torch.randn(5, 3, 3, dtype=torch.float64), "loss": torch.tensor(0.25)}
    shapes = bench.dump_outputs(str(tmp_path / "d"), res, model, _Opt(10))
    assert sorted(os.listdir(tmp_path / "d")) == sorted(n + ".npy" for n in NAMES)
    got = {n: np.load(tmp_path / "d" / (n + ".npy")) for n in NAMES}
    assert all(v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["pred"], res["pred"].numpy()) and got["target"].shape == (5, 3, 3)
    assert got["loss"].shape == () and got["loss"] == np.float32(0.25)
    assert np.array_equal(got["params"], np.arange(10, dtype=np.float32))
    # running_mean then running_var (num_batches_tracked is an integer buffer: not an output of the arithmetic)
    assert np.array_equal(got["buffers"], np.array([0.5] * 4 + [1.0] * 4, dtype=np.float32))
    assert shapes["pred"] == [5, 3, 3] and shapes["loss"] == []


def test_dump_outputs_samples_to_the_size_cap(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 65536 + 4000)
    res = {"pred": torch.randn(1000), "target": torch.randn(1000), "loss": torch.tensor(1.0)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), res, torch.nn.Identity(), _Opt(100_000))
    size = sum(os.path.getsize(tmp_path / "a" / (n + ".npy")) for n in NAMES)
    assert size <= bench.DUMP_BYTES_MAX
    p = np.load(tmp_path / "a" / "params.npy")
    assert 0 < p.size < 100_000 and np.all(np.diff(p) > 0)          # a sample of arange, kept in order
    for n in NAMES:                                                   # the sample is fixed: the same elements every run
        assert np.array_equal(np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy")))


def _run(tmp_path, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
           "--preroll-steps", "10"] + list(extra)
    out = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_line_and_dump_match_a_full_run(tmp_path):
    plain = _run(tmp_path, "--dump-outputs", str(tmp_path / "plain"))
    assert plain["full"] is False and plain["steps"] == 3 and plain["warmup"] == 2
    assert plain["unit"] == "graphs/s" and plain["higher_is_better"] is True and plain["dtype"] == "f32"
    assert plain["value"] > 0 and abs(plain["value"] - 64 * 3 / (plain["ms_per_step"] * 3e-3)) / plain["value"] < 1e-3
    assert plain["untimed_steps_total"] == 10 + 2 + plain["spinup"]
    for k in ("roofline", "cpu_baseline", "cold", "sustained", "telemetry", "calibration", "bf16x3", "jarvis_bf16"):
        assert k not in plain, k
    full = _run(tmp_path, "--full", "--no-subconfigs", "--no-cpu-baseline", "--sustain-seconds", "0",
                "--dump-outputs", str(tmp_path / "full"))
    assert full["full"] is True and "roofline" in full and "cold" in full
    assert full["untimed_steps_total"] == plain["untimed_steps_total"]
    a = {n: np.load(tmp_path / "plain" / (n + ".npy")) for n in NAMES}
    b = {n: np.load(tmp_path / "full" / (n + ".npy")) for n in NAMES}
    assert a["params"].size == 2_498_438 and a["pred"].shape[0] == a["target"].shape[0] > 0
    assert np.isfinite(a["loss"]) and abs(float(a["loss"]) - float(np.abs(a["pred"] - a["target"]).mean())) < 1e-4
    for n in NAMES:     # same inputs, same number of steps before the last timed one: the same arithmetic
        err = float(np.abs(a[n] - b[n]).max()) / max(float(np.abs(b[n]).max()), 1e-30)
        assert a[n].shape == b[n].shape and err <= 1e-5, (n, err)
