"""bench.py's launch contract (BASELINE.json metric "1/2/4/8-GPU"): `--gpus N` starts N ranks
when no launcher did, and refuses a launcher whose WORLD_SIZE disagrees with --gpus."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def test_world_size_mismatch_is_an_error():
    """A launcher's WORLD_SIZE that disagrees with --gpus exits non-zero before any GPU call."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--no-cpu-baseline"],
                       env=_env(WORLD_SIZE="3", RANK="0", LOCAL_RANK="0"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 2, r.stderr
    assert "WORLD_SIZE=3" in r.stderr


@pytest.mark.gpu
def test_gpus_flag_spawns_ranks(cuda):
    """`bench.py --gpus 2` with no launcher runs two ranks (here both on cuda:0 over gloo, the
    one-GPU rehearsal of the driver's multi-GPU run) and rank 0 reports n_gpus = 2."""
    r = subprocess.run([sys.executable, "-u", BENCH, "--gpus", "2", "--same-device", "--dist-backend",
                        "gloo", "--steps", "2", "--warmup", "1", "--bags", "4", "--no-cpu-baseline",
                        "--busy-seconds", "1", "--no-calibration"],
                       env=_env(), capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2
    assert out["config"]["global_batch_bags"] == 8
    assert out["value"] > 0


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_outputs(cuda, tmp_path):
    """A run without --full times its --steps steps and measures nothing else (the keys of the
    moved measurements are null), and --dump-outputs writes the last timed step's outputs as
    float32 .npy: 4 bags of N = 2048, T = 100, C = 2 (the two-kernel path at this batch size)."""
    import numpy as np
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, "-u", BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--bags", "4", "--dump-outputs", str(d)],
                       env=_env(), capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["dtype"] == "bf16"
    assert out["ms_per_step"] > 0
    assert abs(out["value"] - 4 * 100 / (out["ms_per_step"] * 1e-3)) <= 1e-9 * out["value"]
    for key in ("cold_start", "shared_heads", "fp32_reference_precision", "single_bag", "cpu_baseline"):
        assert out[key] is None, key
    assert out["mfma_calibration"] == {} and out["roofline"]["clock_mhz"] is None
    assert out["busy_warmup_s"] < 5.0
    B, N, T, C = 4, 2048, 100, 2
    shapes = {"Y": (B, T, C), "A": (T * C * B * N,), "A_mean": (C * B * N,), "A_var": (C * B * N,)}
    assert sorted(p.name for p in d.iterdir()) == sorted(k + ".npy" for k in shapes)
    arrs = {k: np.load(d / (k + ".npy")) for k in shapes}
    for k, a in arrs.items():
        assert a.dtype == np.float32 and a.shape == shapes[k] and np.isfinite(a).all(), k
    # per bag A is [T, C, N], a softmax over the N instances; A_mean is its mean over the T passes
    A = arrs["A"].reshape(B, T, C, N).astype(np.float64)
    assert np.abs(A.sum(-1) - 1).max() < 1e-5
    # (an fp32 running mean of T terms <= max A: up to 4 roundings of 2^-24 relative per term)
    assert np.abs(A.mean(1) - arrs["A_mean"].reshape(B, C, N)).max() <= 4 * T * 2.0 ** -24 * A.max()


def test_dump_outputs_sample_is_fixed():
    """An output above DUMP_MAX_ELEMS elements is dumped at the same sorted sample of positions
    every time; smaller ones whole, in float32."""
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    import bench
    import tempfile
    big = torch.arange(bench.DUMP_MAX_ELEMS + 1000, dtype=torch.float64)
    small = torch.arange(12, dtype=torch.bfloat16).reshape(3, 4)
    got = []
    for _ in range(2):
        with tempfile.TemporaryDirectory() as d:
            bench.dump_outputs({"big": big, "small": small}, d)
            assert sorted(os.listdir(d)) == ["big.npy", "small.npy"]
            got.append((np.load(os.path.join(d, "big.npy")), np.load(os.path.join(d, "small.npy"))))
    assert got[0][0].dtype == np.float32 and got[0][0].shape == (bench.DUMP_MAX_ELEMS,)
    assert np.array_equal(got[0][0], got[1][0]) and np.all(np.diff(got[0][0]) >= 0)
    assert got[0][1].dtype == np.float32 and np.array_equal(got[0][1], np.arange(12).reshape(3, 4))
    assert 4 * 4 * bench.DUMP_MAX_ELEMS <= 64e6       # four outputs stay under 64 MB


def test_cpu_baseline_core_count_has_provenance():
    """cpu_baseline times the reference on every CPU this process may use: its affinity mask,
    capped by the cgroup CPU quota; the line records both (verdict r04, item 7)."""
    sys.path.insert(0, REPO)
    import bench
    n, prov = bench.host_cores()
    assert prov["affinity_cpus"] == len(os.sched_getaffinity(0))
    assert 1 <= n <= prov["affinity_cpus"]
    if prov["cgroup_cpu_quota"] is not None:
        assert n <= max(1, int(prov["cgroup_cpu_quota"]))
