"""plan_attention_grad_f64 (csrc/kernels/attention_plan.cpp) without a device, through a driver built from that unit alone: each
kernel's step (from the constexpr functions the kernels are instantiated on), the LDS bytes in doubles, the even rule of
eg_dgemm_batched2 for all nine operands, the refusals and the cut."""
import os
import subprocess

import pytest

from test_attention_grad_plan_cpu import CSRC, LDS_PER_CU, OPERANDS, ROOT, plan



@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("attention_grad_f64_plan") / "attention_grad_f64_plan_driver")
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "attention_grad_f64_plan_driver.cpp"),
                          os.path.join(CSRC, "kernels", "attention_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


@pytest.mark.parametrize("kp,dp", [(kp, dp) for kp in (32, 64, 128) for dp in (32, 64, 128)])
def test_the_steps_are_the_constexpr_functions_and_fit_the_lds(driver, kp, dp):
    p = plan(driver, 2, 3, 70, 130, kp, dp)
    assert p["supported"] == 1 and p["reason"] == "" and (p["kp"], p["dp"], p["block"], p["dq_tile"], p["dkv_tile"]) == (kp, dp, 256, 64, 64)
    assert (p["dq_step"], p["dkv_step"]) == (p["fn_dq_step"], p["fn_dkv_step"]) and {p["dq_step"], p["dkv_step"]} <= {64, 32}
    # rows of width + 18 for tiles read both ways, width + 2 for the dQ kernel's V tile, the waves' [4][16][step + 18], 64 x 2 doubles
    tj, ti = p["dq_step"], p["dkv_step"]
    assert p["dq_lds"] == p["fn_dq_lds"] == 8 * (tj * (kp + 18) + tj * (dp + 2) + 64 * (tj + 18) + 128)
    assert p["dkv_lds"] == p["fn_dkv_lds"] == 8 * (ti * (kp + 18) + ti * (dp + 18) + 64 * (ti + 18) + 128)
    assert 0 < p["dq_lds"] <= LDS_PER_CU and 0 < p["dkv_lds"] <= LDS_PER_CU
    assert tj == (64 if p["dq_lds64"] <= LDS_PER_CU else 32)      # the dQ kernel: the LDS alone decides
    assert (kp, dp) != (128, 128) or (tj, ti, p["dq_lds64"], p["dkv_lds64"], p["dq_lds"], p["dkv_lds"]) == (32, 32, 184320, 192512, 97280, 101376)
    assert (kp, dp) != (32, 32) or (tj, ti) == (64, 64)
    assert (kp, dp) not in ((128, 64), (64, 128)) or (p["dq_lds64"], p["dkv_lds64"]) == (151552, 159744)


def test_head_dimensions_above_128_are_refused_with_the_reason(driver):
    got = [plan(driver, 2, 3, 70, 70, K, D) for K, D in ((129, 64), (64, 129))]
    assert [(p["supported"], p["reason"]) for p in got] == [(0, "K above 128"), (0, "D above 128")]


def test_sixteen_byte_accesses_exactly_under_the_even_rule(driver):
    """per operand, outputs included; 2 (mod 4) and a stride of 0 qualify; one odd value turns that operand's flag off and no other"""
    good = (66, 4226, 66, 1)
    all_good = {name: good for name in OPERANDS}
    p = plan(driver, 2, 3, 64, 64, 62, 62, **all_good)
    assert [p["vec_" + name] for name in OPERANDS] == [1] * 9
    bad = {"pointer": (66, 4226, 66, 0), "ld": (67, 4288, 66, 1), "stride0": (66, 4227, 66, 1), "stride1": (66, 4226, 65, 1)}
    for which in OPERANDS:
        for name, op in bad.items():
            p = plan(driver, 2, 3, 64, 64, 62, 62, **dict(all_good, **{which: op}))
            assert {x: p["vec_" + x] for x in OPERANDS} == {x: int(x != which) for x in OPERANDS}, (which, name, p)
    p = plan(driver, 2, 3, 64, 64, 64, 64, k=(64, 0, 0, 1), v=(64, 0, 0, 1))
    assert p["vec_k"] == 1 and p["vec_v"] == 1


@pytest.mark.parametrize("b0,b1,I,J", [(2, 3, 33, 70), (70000, 70, 1, 130), (70000, 70, 130, 1), (1, (1 << 22) + 1, 1, 1)])
def test_both_kernels_are_cut_past_2_22_blocks(driver, b0, b1, I, J):
    p = plan(driver, b0, b1, I, J, 8, 8)
    assert p["supported"] == 1 and p["items"] == b0 * b1 and p["max_blocks"] == 1 << 22
    for kernel, tiles in (("dq", -(-I // 64)), ("dkv", -(-J // 64))):
        per = p[kernel + "_items_per_launch"]
        assert p[kernel + "_tiles"] == tiles and p[kernel + "_grid"] == b0 * b1 * tiles and per == max(1, p["max_blocks"] // tiles)
        assert p[kernel + "_launches"] == -(-p["items"] // per) and (p[kernel + "_launches"] > 1) == (p[kernel + "_grid"] > p["max_blocks"])
