"""match_attention (csrc/host/match_attention.cpp) without a device: a driver built with the host compiler from kd.cpp,
match.cpp, match_attention.cpp and error.cpp alone prints, for every live position of every target of a program, the chain
found there or the reason of the refusal."""
import os
import subprocess

import pytest

import attention_fused_programs as fp
import attention_programs as ap
import refcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exprgrad_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("attention_match") / "attention_match_driver")
    units = [os.path.join(ROOT, "tests", "attention_match_driver.cpp")] + [os.path.join(CSRC, u) for u in (
        "host/kd.cpp", "host/match.cpp", "host/match_attention.cpp", "error.cpp")]
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC] + units + ["-o", exe],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def rows(exe, tmp_path, name, graphs):
    path = str(tmp_path / (name + ".kd"))
    with open(path, "w") as f:
        f.write(refcases.program_text(graphs()))
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return [dict(kv.split("=", 1) for kv in line.split()) for line in out.stdout.splitlines()]


def hits(found, target="out"):
    return [r for r in found if r["target"] == target and r["match"] == "1"]


@pytest.mark.parametrize("name,graphs,n,scale,scaled", [
    ("forward", fp.attention_forward(), 5, "0.125", "scaled"), ("unscaled", fp.attention_forward_unscaled, 4, "1", "-"),
    ("scale_first", fp.attention_forward_scale_first, 5, "0.125", "scaled")])
def test_the_out_targets_match_once(driver, tmp_path, name, graphs, n, scale, scaled):
    found = rows(driver, tmp_path, name, graphs)
    got = hits(found)
    assert len(got) == 1, found
    assert got[0] == {"target": "out", "pos": "0", "match": "1", "n": str(n), "scale": scale, "q": "q", "kk": "kk", "v": "v", "out": "context",
                      "scores": "scores", "scaled": scaled, "sums": "softmax.sums", "softmax": "softmax"}


def test_the_training_program(driver, tmp_path):
    """its `out` target holds the chain at positions 0..4; its `fit` target, whose gradient kernels read the scores and the
    softmax, matches nowhere"""
    found = rows(driver, tmp_path, "training", ap.attention_training(*ap.TRAINING_SHAPE))
    got = hits(found)
    assert len(got) == 1 and got[0]["pos"] == "0" and got[0]["n"] == "5" and got[0]["scale"] == "0.125", found
    fit = [r for r in found if r["target"] == "fit"]
    assert len(fit) >= 10 and not hits(found, "fit"), fit
    assert "an_intermediate_is_read_outside_the_chain" in {r["why"] for r in fit}, fit


REASONS = {
    "causal_mask": "the_row_sum_is_not_a_sum_of_exp_alone",
    "bounded_columns": "the_row_sum_has_loop_bounds,_computed_indices_or_another_rank",
    "transposed_operand": "the_row_sum_does_not_read_the_scaled_scores_alone",
    "sum_over_queries": "the_row_sum_does_not_run_over_the_last_axis",
    "softmax_of_the_transpose": "a_register_of_the_softmax_is_not_in_the_position_of_the_scores",
    "rank3": "the_first_kernel_is_not_an_NT_product_with_two_batch_indices",
    "rank5": "the_first_kernel_is_not_an_NT_product_with_two_batch_indices",
    "scale_by_a_tensor": "the_kernel_behind_the_scores_is_neither_a_scale_map_over_them_nor_the_row_sum",
    "scale_by_division": "the_scale_is_not_one_multiplication_by_a_literal",
    "scores_read_again": "an_intermediate_is_read_outside_the_chain",
    "softmax_is_the_output": "the_chain_ends_behind_the_target's_last_kernel",
}


@pytest.mark.parametrize("name", sorted(fp.NEAR_MISSES))
def test_near_misses_are_refused(driver, tmp_path, name):
    found = rows(driver, tmp_path, name, fp.NEAR_MISSES[name][0])
    assert found and not hits(found), found
    first = [r for r in found if r["pos"] == "0"][0]
    assert first["why"] == REASONS[name], first
