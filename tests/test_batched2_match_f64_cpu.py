"""match_batched2_gemm (csrc/host/match.cpp) on the `kd 1 f64` text of the programs of tests/multihead_programs.py and of the
attention training program (tests/attention_programs.py): the matcher answers for a float64 program what it answers for
the float32 one — the model route of eg_model_batched2_f64 takes exactly the kernels a float32 model runs as eg_bgemm2.
Built like tests/test_batched2_cpu.py: its driver (tests/batched2_driver.cpp), which prints the two-index match, with the
host compiler, no device."""
import os
import subprocess

import pytest

import attention_programs as ap
import multihead_programs as mh
from exprgrad_amd import dsl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exprgrad_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("batched2_64") / "batched2_driver")
    units = [os.path.join(ROOT, "tests", "batched2_driver.cpp")] + [os.path.join(CSRC, u) for u in
                                                                    ("host/kd.cpp", "host/match.cpp", "kernels/gemm_plan.cpp", "error.cpp")]
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC] + units + ["-o", exe],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def rows_of(exe, tmp_path, name, graphs, scalar):
    prog = dsl.to_program(*graphs())
    prog.scalar = scalar
    text = prog.to_text()
    assert text.splitlines()[0].split()[:3] == ["kd", "1", scalar]
    path = str(tmp_path / ("%s_%s.kd" % (name, scalar)))
    with open(path, "w") as f:
        f.write(text)
    out = subprocess.run([exe, "match", path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = [dict(kv.split("=", 1) for kv in line.split()) for line in out.stdout.splitlines()]
    for r in rows:
        del r["file"]
    return rows


def both(exe, tmp_path, name, graphs):
    f32, f64 = rows_of(exe, tmp_path, name, graphs, "f32"), rows_of(exe, tmp_path, name, graphs, "f64")
    assert f64 == f32, name
    return f64


def hits(rows, target):
    return sorted((r["ta"], r["tb"]) for r in rows if r["target"] == target and r["match"] == "1")


def test_the_two_forward_products(driver, tmp_path):
    s, = both(driver, tmp_path, "scores", mh.scores_forward)
    assert (s["match"], s["ta"], s["tb"], s["a"], s["b"]) == ("1", "0", "1", "q", "kk")
    o, = both(driver, tmp_path, "context", mh.context_forward)
    assert (o["match"], o["ta"], o["tb"], o["a"], o["b"]) == ("1", "0", "0", "p", "v")
    assert (o["c_batch"], o["c_row"]) == ("0,2", "1")      # o[b,i,h,d]: the items of C interleave


def test_scores_training_holds_three_products(driver, tmp_path):
    rows = both(driver, tmp_path, "training", mh.scores_training(2, 3, 33, 20, 16))
    assert hits(rows, "fit") == [("0", "0"), ("0", "1"), ("1", "0")] and hits(rows, "out") == [("0", "1")]
    assert all(r["match"] == "0" for r in rows if r["loops"] != "5")


def test_attention_training_holds_six_products(driver, tmp_path):
    """scores NT and context NN forward; the softmax's gradient p' = do * v^T (NT), dv = p^T * do (TN), dq = ds * kk (NN),
    dk = ds^T * q (TN)."""
    rows = both(driver, tmp_path, "attention", ap.attention_training(*ap.TRAINING_SHAPE))
    assert hits(rows, "out") == [("0", "0"), ("0", "1")]
    assert hits(rows, "fit") == [("0", "0"), ("0", "0"), ("0", "1"), ("0", "1"), ("1", "0"), ("1", "0")]
    assert all(r["match"] == "0" for r in rows if r["loops"] != "5")


@pytest.mark.parametrize("name", sorted(mh.NEAR_MISSES))
def test_near_misses_stay_generated_f64(driver, tmp_path, name):
    row, = both(driver, tmp_path, name, mh.NEAR_MISSES[name])
    assert row["match"] == "0"
