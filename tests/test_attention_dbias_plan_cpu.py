"""plan_attention_dbias (csrc/kernels/attention_plan.cpp) without a device: a driver built from that unit alone prints the plan
of a problem — supported or not and why, the cells and what a block sums, the tiles per cell, the row fold, the access width
of each operand, the cut into launches and the LDS bytes."""
import os
import subprocess

import pytest

from test_attention_grad_plan_cpu import CSRC, LDS_PER_CU, ROOT, dense

OPERANDS = ("q", "k", "v", "o", "s", "do", "b", "db")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("attention_dbias_plan") / "attention_dbias_plan_driver")
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "attention_dbias_plan_driver.cpp"),
                          os.path.join(CSRC, "kernels", "attention_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def form(name, b1, I, J):
    """(ld, stride0, stride1, aligned) of a bias or its gradient"""
    return {"full": dense(b1, I, J), "heads": (J, 0, I * J, 1), "causal": (J, 0, 0, 1), "padding": (0, J, 0, 1), "slope": (0, 0, J, 1)}[name]


def plan(exe, b0, b1, I, J, K, D, bias="full", **changed):
    ops = {"q": dense(b1, I, K), "k": dense(b1, J, K), "v": dense(b1, J, D), "o": dense(b1, I, D), "s": (0, b1 * I, I, 1), "do": dense(b1, I, D),
           "b": form(bias, b1, I, J), "db": form(bias, b1, I, J)}
    ops.update(changed)
    out = subprocess.run([exe] + [str(x) for x in (b0, b1, I, J, K, D) + tuple(y for name in OPERANDS for y in ops[name])], capture_output=True,
                         text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    head, reason = lines[0].split(" reason=")
    p = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in head.split()}
    p["reason"] = reason
    p["launch"] = [tuple(int(x) for x in line.split()[1:]) for line in lines[1:]]
    return p


@pytest.mark.parametrize("bias,cells,sums,fold", [("full", (2, 3), (1, 1), 0), ("heads", (1, 3), (2, 1), 0), ("causal", (1, 1), (2, 3), 0),
                                                  ("padding", (2, 1), (1, 3), 1), ("slope", (1, 3), (2, 1), 1)])
@pytest.mark.parametrize("I,J", [(33, 70), (130, 129), (64, 64), (200, 7)])
def test_cells_and_tiles_of_each_broadcast_form(driver, bias, cells, sums, fold, I, J):
    p = plan(driver, 2, 3, I, J, 16, 16, bias=bias)
    ti, tj = -(-I // 64), -(-J // 64)
    tiles = tj if fold else ti * tj
    assert p["supported"] == 1 and p["row_fold"] == fold and p["block"] == 256
    assert (p["cells0"], p["cells1"], p["cells"]) == cells + (cells[0] * cells[1],) and (p["sum0"], p["sum1"]) == sums
    assert (p["tiles_i"], p["tiles_j"], p["tiles"], p["grid"]) == (ti, tj, tiles, p["cells"] * tiles)
    assert p["launch"] == ([(0, p["cells"], p["grid"])] if tiles else []) and p["launches"] == (1 if tiles else 0)


@pytest.mark.parametrize("kp", [32, 64, 128])
@pytest.mark.parametrize("dp", [32, 64, 128])
def test_every_instantiation_fits_the_lds(driver, kp, dp):
    """four NT tiles of width + 4 floats, 64 x 2 floats; the look-ahead exactly where two blocks do not fit a CU"""
    p = plan(driver, 2, 3, 70, 70, kp, dp)
    lds = 4 * (2 * 64 * (kp + 4) + 2 * 64 * (dp + 4) + 128)
    assert (p["supported"], p["kp"], p["dp"], p["lds"], p["ahead"]) == (1, kp, dp, lds, int(2 * lds > LDS_PER_CU)) and lds <= LDS_PER_CU


def test_refusals(driver):
    for K, D in ((129, 64), (64, 129), (129, 129)):
        p = plan(driver, 2, 3, 70, 70, K, D)
        assert p["supported"] == 0 and "128" in p["reason"] and p["reason"].startswith("K" if K > 128 else "D"), p
    assert plan(driver, 0, 3, 70, 70, 16, 16)["supported"] == 0 and plan(driver, 2, 0, 70, 70, 16, 16, bias="heads")["supported"] == 0
    assert plan(driver, 0, 3, 70, 70, 16, 16, bias="heads")["supported"] == 1   # an empty sum is a plan
    p = plan(driver, 1, 1, 64 * 4096, 64 * 2048, 16, 16)
    assert p["supported"] == 0 and "tiles" in p["reason"], p
    assert plan(driver, 1, 1, 64 * 4096, 64 * 2048, 16, 16, bias="padding")["supported"] == 1


def test_sixteen_byte_accesses_exactly_under_the_rule(driver):
    """per operand, dBias included; the bias itself has no flag: it is read element by element"""
    names = [n for n in OPERANDS if n != "b"]
    good = (64, 4096, 64, 1)
    all_good = {name: good for name in OPERANDS}
    assert [plan(driver, 2, 3, 64, 64, 64, 64, **all_good)["vec_" + n] for n in names] == [1] * 7
    for which in names:
        for op in ((64, 4096, 64, 0), (66, 4224, 64, 1), (64, 4098, 64, 1), (64, 4096, 62, 1)):   # pointer, ld, stride0, stride1
            p = plan(driver, 2, 3, 64, 64, 62, 62, **dict(all_good, **{which: op}))
            assert {n: p["vec_" + n] for n in names} == {n: int(n != which) for n in names}, (which, op, p)
    assert plan(driver, 2, 3, 64, 64, 64, 64, bias="padding")["vec_db"] == 1   # steps of 0 are multiples of 4


@pytest.mark.parametrize("b0,b1,I,J,bias", [(70000, 70, 1, 130, "full"), (2049, 2048, 64, 64, "full"), (1, (1 << 22) + 1, 1, 1, "heads"),
                                            ((1 << 21) + 3, 5, 7, 129, "padding")])
def test_the_cut_covers_every_cell_once(driver, b0, b1, I, J, bias):
    """past 2^22 blocks the flattened cell range is cut: by arithmetic only, nothing is launched"""
    p = plan(driver, b0, b1, I, J, 8, 8, bias=bias)
    assert p["supported"] == 1 and p["grid"] > p["max_blocks"]
    per = p["items_per_launch"]
    assert per == max(1, p["max_blocks"] // p["tiles"]) and p["launches"] == -(-p["cells"] // per) == len(p["launch"]) > 1
    nxt = 0
    for first, items, grid in p["launch"]:
        assert first == nxt and items >= 1 and grid == items * p["tiles"] and grid <= p["max_blocks"]
        nxt = first + items
    assert nxt == p["cells"]
