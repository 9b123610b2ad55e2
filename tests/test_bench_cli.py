"""bench.py's command line: the plain run's line, --full, --dump-outputs and the argument checks."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
BENCH = ROOT / "bench.py"
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("stage_seconds", "verified", "dense_floor", "hard_workload", "roofline", "cpu_baseline")
DUMPED = ("centroids", "tokens_train", "tokens_val", "kmeans_objective")


def _bench(*args, timeout=600):
    return subprocess.run([sys.executable, str(BENCH), *args], cwd=ROOT, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("args, message", [
    (["--steps", "0"], "--steps must be at least 1"),
    (["--warmup", "-1"], "--warmup at least 0"),
    (["--host-waves"], "--host-waves is one of the --full measurements"),
])
def test_bad_arguments_fail_before_any_work(args, message):
    r = _bench(*args, timeout=120)
    assert r.returncode == 2 and message in r.stderr, r.stderr


def test_dump_outputs_writes_float32_and_a_fixed_sample(tmp_path, monkeypatch):
    import bench
    from audio_tokens_amd.pipeline import PipelineResult

    monkeypatch.setattr(bench, "DUMP_TOKENS", 1000)
    g = torch.Generator().manual_seed(7)
    res = PipelineResult(torch.randn(64, 16, generator=g), torch.randint(0, 64, (5000,), generator=g),
                         torch.randint(0, 64, (600,), generator=g), 10,
                         kmeans_stats=[[dict(obj=float(np.float32(o)))] for o in (3.5, 2.25)])
    bench.dump_outputs(res, tmp_path / "a")
    bench.dump_outputs(res, tmp_path / "b")
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in DUMPED}
    assert all(a.dtype == np.float32 for a in got.values())
    for n in DUMPED:
        assert np.array_equal(got[n], np.load(tmp_path / "b" / f"{n}.npy")), n
    np.testing.assert_array_equal(got["centroids"], res.centroids.numpy())
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, 5000, 1000))
    np.testing.assert_array_equal(got["tokens_train"], res.tokens_train.numpy()[idx].astype(np.float32))
    np.testing.assert_array_equal(got["tokens_val"], res.tokens_val.numpy().astype(np.float32))   # small enough: whole
    np.testing.assert_array_equal(got["kmeans_objective"], np.float32([3.5, 2.25]))


TINY = ["--gpus", "1", "--train-clips", "40", "--val-clips", "8", "--clip-seconds", "1", "--vocab", "1024"]


@pytest.mark.gpu
def test_plain_and_full_runs(tmp_path):
    r = _bench(*TINY, "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "plain"))
    assert r.returncode == 0, r.stderr[-2000:]
    plain = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(k in plain for k in HEADLINE) and not any(k in plain for k in FULL_ONLY), sorted(plain)
    assert plain["steps"] == 2 and plain["ms_per_step"] > 0 and plain["value"] > 0 and plain["full"] is False
    assert plain["unit"] == "frames/s" and plain["higher_is_better"] is True and plain["dtype"] == "f32"

    r = _bench(*TINY, "--steps", "1", "--warmup", "1", "--full", "--cpu-clips", "8",
               "--dump-outputs", str(tmp_path / "full"))
    assert r.returncode == 0, r.stderr[-2000:]
    full = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(k in full for k in HEADLINE + FULL_ONLY), sorted(full)
    assert full["verified"] is True and full["roofline"]["kernel_classes"] and full["cpu_baseline"]["value"] > 0

    for n in DUMPED:   # the same inputs every run: the plain and the full run computed the same
        a, b = np.load(tmp_path / "plain" / f"{n}.npy"), np.load(tmp_path / "full" / f"{n}.npy")
        assert a.dtype == np.float32 and a.size > 0, n
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), n
    assert np.load(tmp_path / "plain" / "tokens_train.npy").size == 40 * full["config"]["frames_per_step"] // 48
