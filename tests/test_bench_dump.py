"""bench.py --dump-outputs: the arrays of the last timed step as float32 .npy files, within 64 MB, sampled at fixed positions;
--steps sets the number of timed steps.  CPU: the dump helper and the argument checks.  GPU: bench.py end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402

NAMES = ("loss", "logits", "params_sample", "grads_sample")


def _model():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.Linear(32, 4))
    m[0].bias.requires_grad_(False)                     # frozen parameters are not part of the dump
    out = m(torch.randn(8, 16))
    loss = out.square().mean()
    loss.backward()
    return m, loss, out


def test_dump_writes_float32_arrays(tmp_path):
    m, loss, out = _model()
    bench.dump_outputs(str(tmp_path), loss, out, m)
    got = {n: np.load(tmp_path / f"{n}.npy") for n in NAMES}
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in NAMES)
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["loss"].shape == (1,) and got["loss"][0] == pytest.approx(loss.item())
    np.testing.assert_array_equal(got["logits"], out.detach().numpy())
    params = [p for p in m.parameters() if p.requires_grad]
    np.testing.assert_array_equal(got["params_sample"], torch.cat([p.detach().reshape(-1) for p in params]).numpy())
    np.testing.assert_array_equal(got["grads_sample"], torch.cat([p.grad.reshape(-1) for p in params]).numpy())


def test_dump_samples_large_arrays_at_fixed_positions(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", {"logits": 10, "params_sample": 50, "grads_sample": 50})
    m, loss, out = _model()
    bench.dump_outputs(str(tmp_path / "a"), loss, out, m)
    bench.dump_outputs(str(tmp_path / "b"), loss, out, m)
    for n in NAMES:
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy"))
    lg = np.load(tmp_path / "a" / "logits.npy")
    assert lg.shape == (10,) and np.isin(lg, out.detach().numpy().reshape(-1)).all()
    params = [p for p in m.parameters() if p.requires_grad]
    flat = torch.cat([p.detach().reshape(-1) for p in params]).numpy()
    ps, gs = np.load(tmp_path / "a" / "params_sample.npy"), np.load(tmp_path / "a" / "grads_sample.npy")
    assert ps.shape == gs.shape == (50,) and np.isin(ps, flat).all()
    # parameters and gradients are sampled at the same positions
    idx = [int(np.flatnonzero(flat == v)[0]) for v in ps]
    flat_g = torch.cat([p.grad.reshape(-1) for p in params]).numpy()
    np.testing.assert_array_equal(gs, flat_g[idx])


def test_dump_budget_is_within_64_mb():
    assert 4 * (1 + sum(bench.DUMP_MAX_ELEMS.values())) <= 64 << 20


@pytest.mark.parametrize("args", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_rejects_bad_step_counts(args, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + args)
    with pytest.raises(SystemExit):
        bench.parse()


def test_bench_full_is_opt_in(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert bench.parse().full is False                  # a plain run measures the headline alone
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert bench.parse().full is True


def _run_bench(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--no-cpu-baseline", "--no-by-config", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_dump_outputs_and_step_count(tmp_path):
    one, three = _run_bench(tmp_path / "s1", 1), _run_bench(tmp_path / "s3", 3)
    assert one["steps"] == 1 and three["steps"] == 3
    # every hot-path kernel launches three times as often in three timed steps as in one
    assert set(one["kernels"]) == set(three["kernels"]) and one["kernels"]
    for k, v in one["kernels"].items():
        assert three["kernels"][k]["launches"] == 3 * v["launches"], k
    for d, res in ((tmp_path / "s1", one), (tmp_path / "s3", three)):
        got = {n: np.load(d / f"{n}.npy") for n in NAMES}
        assert sum(os.path.getsize(d / f"{n}.npy") for n in NAMES) <= 64 << 20
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
        assert got["loss"][0] == pytest.approx(res["loss"], abs=1e-5)
        assert got["logits"].shape == (3 * 5, 3, 256, 256)           # (batch * clip_length, classes, H, W)
        assert got["params_sample"].shape == got["grads_sample"].shape == (bench.DUMP_MAX_ELEMS["params_sample"],)
    # more optimizer steps moved the parameters further
    assert not np.array_equal(np.load(tmp_path / "s1" / "params_sample.npy"), np.load(tmp_path / "s3" / "params_sample.npy"))
