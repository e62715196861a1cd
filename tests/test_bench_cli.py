"""bench.py's command line: what a plain run does, what --full adds, and --dump-outputs."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = ("attribution", "cpu_baseline", "roofline", "fwd_line")


def _parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_has_the_extras_off(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert [getattr(a, k) for k in EXTRAS] == [0, 0, 0, 0]


def test_full_turns_the_extras_on_and_each_switch_overrides(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert [getattr(a, k) for k in EXTRAS] == [1, 1, 1, 1]
    a = _parse(monkeypatch, "--full", "--cpu-baseline", "0")
    assert [getattr(a, k) for k in EXTRAS] == [1, 0, 1, 1]
    a = _parse(monkeypatch, "--roofline", "1")
    assert [getattr(a, k) for k in EXTRAS] == [0, 0, 1, 0]


def test_dump_outputs_writes_float32_and_samples_past_the_budget(tmp_path, monkeypatch):
    import bench
    g = torch.Generator().manual_seed(3)
    arrays = {"out": torch.randn(5, 1, generator=g), "loss": torch.tensor(2.5, dtype=torch.float64),
              "big": torch.randn(700, 1000, generator=g)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    got = {n: np.load(tmp_path / "a" / n) for n in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["big.npy", "loss.npy", "out.npy"]
    assert all(v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["big.npy"], arrays["big"].numpy()) and got["loss.npy"] == np.float32(2.5)
    # past the budget: small arrays whole, the large one a fixed sample of its elements that fits
    monkeypatch.setattr(bench, "DUMP_BUDGET", 1 << 20)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    b = {n: np.load(tmp_path / "b" / n) for n in os.listdir(tmp_path / "b")}
    c = {n: np.load(tmp_path / "c" / n) for n in os.listdir(tmp_path / "c")}
    assert sum(v.nbytes for v in b.values()) <= 1 << 20
    assert np.array_equal(b["out.npy"], got["out.npy"])
    assert b["big.npy"].ndim == 1 and 0 < b["big.npy"].size < 700 * 1000
    assert np.isin(b["big.npy"], got["big.npy"]).all()
    assert all(np.array_equal(b[n], c[n]) for n in b)


@pytest.mark.gpu
def test_plain_bench_line_and_dump(tmp_path):
    """A plain run: --steps timed steps, ms_per_step in the line, nothing of --full measured, and the last
    step's outputs and gradients written as finite float32 arrays."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--bs", "32", "--settle-s", "0", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "graphs/s" and d["dtype"] == "fp32"
    assert d["higher_is_better"] is True and d["ms_per_step"] > 0
    assert abs(d["value"] - 32 / d["ms_per_step"] * 1e3) <= 1e-3 * d["value"]
    for k in ("attribution", "roofline", "roofline_hbm", "roofline_fwd", "cpu_baseline", "parity"):
        assert d[k] is None
    names = sorted(os.listdir(out))
    assert {"out.npy", "loss.npy", "dX.npy", "dW.npy", "grad.layer0.cv1.weight.npy"} <= set(names)
    assert len(names) == 4 + 50
    for n in names:
        a = np.load(out / n)
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
    assert np.load(out / "out.npy").shape[0] == 32
