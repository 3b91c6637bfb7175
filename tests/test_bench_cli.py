"""bench.py's command line: a plain run does only the timed steps, --full adds the other legs, and
--dump-outputs writes what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def test_full_and_dump_options_default_off(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 4
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_float32_limit_and_fixed_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT", 64 << 10)     # the same rule at 64 KB
    g = torch.Generator().manual_seed(3)
    big = torch.randn(40000, generator=g).to(torch.bfloat16)   # 160 KB as float32: sampled
    arrays = {"loss": torch.tensor(0.25), "stats": torch.tensor([1.0, 2.0, 3.0]), "output": big}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    total = 0
    for name, t in arrays.items():
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b)
        total += os.path.getsize(tmp_path / "a" / f"{name}.npy")
        if name != "output":
            assert np.array_equal(a, t.float().numpy())
    assert total <= 64 << 10
    out = np.load(tmp_path / "a" / "output.npy")
    assert out.ndim == 1 and 10000 < out.size < big.numel()
    ref = big.float().numpy()
    # the sample keeps the order of the flattened array: it is a subsequence of it
    pos = 0
    for v in out:
        while pos < ref.size and ref[pos] != v:
            pos += 1
        assert pos < ref.size
        pos += 1


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_identical_outputs(tmp_path):
    """A plain run carries no roofline / cpu_baseline / reference_architecture, --steps sets the timed
    steps, and two runs with the same arguments write the same outputs (same weights, batches and
    step order; the kernels sum in a fixed order)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    base = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
            "--img", "256", "--batch", "2"]
    recs = []
    for tag in ("a", "b"):
        r = subprocess.run(base + ["--dump-outputs", str(tmp_path / tag)], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-3000:]
        recs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    rec = recs[0]
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["unit"] == "images/sec" and rec["higher_is_better"]
    assert abs(rec["value"] - 2 * 1e3 / rec["ms_per_step"]) < 1e-2 * rec["value"]
    assert rec["roofline"] is None and rec["cpu_baseline"] is None and "reference_architecture" not in rec
    out = np.load(tmp_path / "a" / "output.npy")
    loss = np.load(tmp_path / "a" / "loss.npy")
    stats = np.load(tmp_path / "a" / "stats.npy")
    assert out.dtype == np.float32 and out.shape == (2, 1, 256, 256) and (out >= 0).all() and (out <= 1).all()
    assert stats.shape == (3,) and round(float(loss), 5) == rec["final_loss"]
    for name in ("output", "loss", "stats"):
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")), name
