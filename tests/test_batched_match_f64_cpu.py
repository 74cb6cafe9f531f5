"""match_batched_gemm (csrc/host/match.cpp) on the `kd 1 f64` text of the programs of tests/batched_programs.py: the
matcher answers for a float64 program what it answers for the float32 one.  Built like tests/test_batched_match_cpu.py:
its driver (tests/batched_match_driver.cpp) with the host compiler, no device."""
import os
import subprocess

import pytest

import batched_programs as bp
from exprgrad_amd import dsl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exprgrad_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("batched64") / "batched_match_driver")
    units = [os.path.join(ROOT, "tests", "batched_match_driver.cpp")] + [os.path.join(CSRC, u) for u in
                                                                         ("host/kd.cpp", "host/match.cpp", "kernels/gemm_plan.cpp", "error.cpp")]
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC] + units + ["-o", exe],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def matches(exe, tmp_path, name, graphs):
    prog = dsl.to_program(*graphs())
    prog.scalar = "f64"
    text = prog.to_text()
    assert text.splitlines()[0].split()[:3] == ["kd", "1", "f64"]
    path = str(tmp_path / (name + ".kd"))
    with open(path, "w") as f:
        f.write(text)
    out = subprocess.run([exe, "match", path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = [dict(kv.split("=", 1) for kv in line.split()) for line in out.stdout.splitlines()]
    assert all(r["match"] == "0" for r in rows if r["loops"] != "4")
    return [(r["target"],) + ((int(r["collapsed"]), int(r["row_k"]), int(r["ta"]), int(r["tb"])) if r["match"] == "1" else (None,))
            for r in rows if r["loops"] == "4"]


def test_the_three_batched_forms_f64(driver, tmp_path):
    assert matches(driver, tmp_path, "forward", bp.batched_forward) == [("out", 0, 0, 0, 0)]
    fit = [m[1:] for m in matches(driver, tmp_path, "training", bp.batched_training(5, 33, 20, 17)) if m[0] == "fit"]
    assert sorted(fit) == [(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0)]


def test_the_three_shared_weight_forms_f64(driver, tmp_path):
    fit = [m[1:] for m in matches(driver, tmp_path, "shared", bp.shared_training(10, 24, 8)) if m[0] == "fit"]
    assert sorted(fit) == [(1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 1), (1, 1, 1, 0), (1, 1, 1, 0)]


@pytest.mark.parametrize("name", sorted(bp.NEAR_MISSES))
def test_near_misses_stay_generated_f64(driver, tmp_path, name):
    assert matches(driver, tmp_path, name, bp.NEAR_MISSES[name]) == [("out", None)]
