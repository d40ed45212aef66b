"""bench.py contract tests: single-process CPU run and the driver's
torchrun world=2 launch (gloo on CPU), validating the JSON line schema."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]

REQUIRED_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup",
                 "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                 "dtype", "data", "config"}


def _last_json_line(stdout: str) -> dict:
    for line in reversed(stdout.strip().splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise AssertionError(f"no JSON line in output: {stdout[-500:]}")


@pytest.mark.slow
def test_bench_single_process_cpu():
    r = subprocess.run(
        [sys.executable, "bench.py", "--steps", "2", "--warmup", "1",
         "--full"],
        capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    res = _last_json_line(r.stdout)
    assert REQUIRED_KEYS <= set(res)
    assert res["n_gpus"] == 1
    assert res["metric"] == "images/sec"
    # a --full run measures BOTH headline models (BASELINE.json names
    # "ResNet-50 & ViT-B/16"); value is the ResNet-50 number
    assert res["config"]["model"] == "resnet50 & vit_b16"
    assert set(res["config"]["models"]) == {"resnet50", "vit_b16"}
    assert res["config"]["models"]["vit_b16"]["images_per_sec"] > 0
    assert res["value"] == res["config"]["models"]["resnet50"]["images_per_sec"]
    assert res["value"] > 0


@pytest.mark.slow
def test_bench_plain_run_and_dump_outputs_cpu(tmp_path):
    """A plain run measures only the headline model, and --dump-outputs writes
    the loss and the updated parameters of the LAST timed step: they match an
    independent plain-PyTorch recomputation of the 3 SGD steps, differ from
    the seeded init, and are identical from run to run on the CPU."""
    import numpy as np
    import torch
    import torch.nn.functional as F

    from deeplearning_amd.data.synthetic import DeviceBatchLoader
    from deeplearning_amd.models import build_model

    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    dumps = []
    for sub in ("a", "b"):
        out = tmp_path / sub
        r = subprocess.run(
            [sys.executable, "bench.py", "--gpus", "1", "--steps", "2",
             "--warmup", "1", "--batch-size", "2", "--lr", "0.1",
             "--dump-outputs", str(out)],
            capture_output=True, text=True, timeout=600, cwd=REPO, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        res = _last_json_line(r.stdout)
        assert REQUIRED_KEYS <= set(res)
        assert res["steps"] == 2 and res["ms_per_step"] > 0
        assert res["config"]["model"] == "resnet50"
        assert "models" not in res["config"]
        assert sorted(p.name for p in out.iterdir()) == [
            "resnet50.loss.npy", "resnet50.params_sample.npy"]
        dumps.append({p.name: np.load(p) for p in out.iterdir()})
    a, b = dumps
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for name, arr in a.items():
        assert arr.dtype == np.float32 and np.isfinite(arr).all(), name
        np.testing.assert_array_equal(arr, b[name])

    # the same 1 warmup + 2 timed steps in plain PyTorch: seeds, batch
    # rotation and optimizer as documented for the benchmark
    torch.manual_seed(1234)
    model = build_model("resnet50", num_classes=1000)
    params = [p for p in model.parameters() if p.requires_grad]
    n = sum(p.numel() for p in params)
    idx = np.sort(np.random.default_rng(2024).choice(
        n, size=1 << 20, replace=False))

    def sample():
        flat = torch.cat([p.detach().reshape(-1) for p in params])
        return flat.numpy()[idx]

    init = sample()
    opt = torch.optim.SGD(params, lr=0.1, momentum=0.9, weight_decay=1e-4)
    batches = DeviceBatchLoader(2, (3, 224, 224), 1000, steps=3,
                                device=torch.device("cpu"), distinct=2,
                                seed=42).batches
    for i in range(3):
        x, y = batches[i % 2]
        loss = F.cross_entropy(model(x), y)
        loss.backward()
        opt.step()
        opt.zero_grad()
    got, want = a["resnet50.params_sample.npy"], sample()
    assert got.shape == (1 << 20,) and a["resnet50.loss.npy"].shape == (1,)
    # fp32 on both sides, same operations: only summation order may differ
    np.testing.assert_allclose(a["resnet50.loss.npy"][0], loss.item(),
                               rtol=1e-4)
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5)
    # the step moved the parameters: the dump is not the seeded init
    assert np.abs(got - init).max() > 1e-3


@pytest.mark.slow
@pytest.mark.timeout(600)
def test_bench_torchrun_world2_cpu():
    """Exactly the driver's launch: torch.distributed.run, nproc 2, gloo."""
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29531", "bench.py", "--gpus", "2",
         "--steps", "2", "--warmup", "1"],
        capture_output=True, text=True, timeout=560, cwd=REPO, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    res = _last_json_line(r.stdout)
    assert res["n_gpus"] == 2
    assert res["config"]["parallelism"] == "dp2"
    # whole-job value: global batch = 2x per-rank batch
    assert res["config"]["global_batch"] == 16  # 8 per rank on CPU


@pytest.mark.slow
@pytest.mark.timeout(600)
def test_classification_cli_torchrun_world2(tmp_path):
    """Full classification training CLI under torchrun world=2 (gloo):
    DDP wrap, DistributedSampler, rank-0 checkpointing."""
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29533",
         "projects/classification/mnist/train.py", "--epochs", "1",
         "--batch-size", "8", "--synthetic-size", "32", "--workers", "0",
         "--device", "cpu", "--output", str(tmp_path)],
        capture_output=True, text=True, timeout=560, cwd=REPO, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    weights = tmp_path / "mnist" / "weights"
    assert (weights / "model_0.pth").exists()
    assert (weights / "best_model.pth").exists()
