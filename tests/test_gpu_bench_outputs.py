"""bench.py's plain run and --dump-outputs: the plain line carries the headline figure and nothing measured besides it,
and the dumped C of the last timed step is the product of the benchmark's seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(extra)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    return subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)


def test_dump_outputs_is_refused_for_a_workload_with_state():
    out = run_bench("--workload", "train", "--dump-outputs", "unused")
    assert out.returncode == 2 and "--dump-outputs" in out.stderr


@pytest.mark.gpu
def test_plain_run_dumps_the_product_of_its_inputs(tmp_path):
    out = run_bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["config"]["timed_steps"] == 3 and line["ms_per_step"] > 0
    assert line["unit"] == "GFLOP/s" and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert abs(line["value"] - 2.0 * 4096 ** 3 / (line["ms_per_step"] * 1e-3) / 1e9) <= 1e-3 * line["value"]
    for moved in ("extra", "cpu_baseline", "value_cold", "end_to_end", "scaling_series_n1"):
        assert moved not in line, moved

    # the inputs as bench.py draws them (torch's generator on the device, seed 2 + rank)
    import torch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    a = torch.rand((4096, 4096), device="cuda", dtype=torch.float32, generator=gen).cpu().numpy()
    b = torch.rand((4096, 4096), device="cuda", dtype=torch.float32, generator=gen).cpu().numpy()
    c = np.load(os.path.join(str(tmp_path), "c.npy"))
    assert c.dtype == np.float32 and c.nbytes <= 64 * 2 ** 20
    rows = np.sort(np.random.default_rng(0).choice(4096, size=c.shape[0], replace=False))
    want = a[rows].astype(np.float64) @ b.astype(np.float64)
    assert float(np.max(np.abs(c - want)) / np.max(np.abs(want))) <= 1e-5
