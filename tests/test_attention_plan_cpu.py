"""plan_attention (csrc/kernels/attention_plan.cpp) without a device: a driver built from that unit alone prints the plan of a
problem — supported or not and why, the tile, the load width per operand, the grid, the cut into launches, the LDS bytes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exprgrad_amd", "csrc")
LDS_PER_CU = 163840


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("attention_plan") / "attention_plan_driver")
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "attention_plan_driver.cpp"),
                          os.path.join(CSRC, "kernels", "attention_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def dense(b1, R, C):
    """[b0, b1, R, C] nested, 16-byte aligned: (ld, stride0, stride1, aligned)"""
    return (C, b1 * R * C, R * C, 1)


def plan(exe, b0, b1, I, J, K, D, q=None, k=None, v=None):
    ops = [q or dense(b1, I, K), k or dense(b1, J, K), v or dense(b1, J, D)]
    out = subprocess.run([exe] + [str(x) for x in (b0, b1, I, J, K, D) + tuple(y for o in ops for y in o)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    head, reason = lines[0].split(" reason=")
    p = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in head.split()}
    p["reason"] = reason
    p["launch"] = [tuple(int(x) for x in line.split()[1:]) for line in lines[1:]]
    return p


@pytest.mark.parametrize("K,D", [(129, 64), (64, 129), (129, 129), (4096, 8)])
def test_head_dimensions_above_128_are_unsupported(driver, K, D):
    p = plan(driver, 2, 3, 70, 70, K, D)
    assert p["supported"] == 0 and "128" in p["reason"], p


@pytest.mark.parametrize("K,D", [(128, 128), (128, 1), (1, 128), (64, 64), (0, 16), (33, 1)])
def test_supported_head_dimensions_fit_the_lds(driver, K, D):
    p = plan(driver, 2, 3, 70, 70, K, D)
    assert p["supported"] == 1 and p["reason"] == "", p
    assert p["kp"] >= K and p["dp"] >= D and p["kp"] in (32, 64, 128) and p["dp"] in (32, 64, 128)
    assert 0 < p["lds"] <= LDS_PER_CU
    # K, V and E rows as attention_plan.hpp pads them
    assert p["lds"] == 4 * (p["tile_j"] * (p["kp"] + 4) + p["tile_j"] * (p["dp"] + 16) + 4 * 16 * (p["tile_j"] + 4))
    assert p["block"] == 256


@pytest.mark.parametrize("b0,b1,I", [(2, 3, 33), (1, 1, 1), (8, 16, 512), (3, 2, 64), (1, 2, 130), (5, 1, 65)])
def test_the_grid_is_items_times_row_tiles(driver, b0, b1, I):
    p = plan(driver, b0, b1, I, 70, 16, 16)
    tiles = -(-I // p["tile_i"])
    assert p["tiles_i"] == tiles and p["items"] == b0 * b1 and p["grid"] == b0 * b1 * tiles
    assert p["launches"] == 1 and p["launch"] == [(0, b0 * b1, p["grid"])]


@pytest.mark.parametrize("b0,b1,I", [(70000, 70, 1), (70000, 70, 130), (2049, 2048, 64), (1, (1 << 22) + 1, 1)])
def test_the_cut_covers_every_item_once(driver, b0, b1, I):
    """past 2^22 blocks the flattened item range is cut: by arithmetic only, nothing is launched"""
    p = plan(driver, b0, b1, I, 8, 8, 8)
    assert p["supported"] == 1 and p["grid"] > p["max_blocks"]
    assert p["items_per_launch"] == max(1, p["max_blocks"] // p["tiles_i"])
    assert p["launches"] == -(-p["items"] // p["items_per_launch"]) and len(p["launch"]) == p["launches"] > 1
    nxt = 0
    for first, items, grid in p["launch"]:
        assert first == nxt and items >= 1 and grid == items * p["tiles_i"] and grid <= p["max_blocks"]
        nxt = first + items
    assert nxt == p["items"] == b0 * b1


def test_sixteen_byte_loads_exactly_under_the_rule(driver):
    """pointer 16-byte aligned, leading dimension and both strides multiples of 4 — per operand; a stride of 0 qualifies"""
    good = (64, 4096, 64, 1)
    assert [plan(driver, 2, 3, 64, 64, 64, 64, q=good, k=good, v=good)[x] for x in ("vec_q", "vec_k", "vec_v")] == [1, 1, 1]
    bad = {"pointer": (64, 4096, 64, 0), "ld": (66, 4224, 64, 1), "stride0": (64, 4098, 64, 1), "stride1": (64, 4096, 62, 1)}
    for which in ("q", "k", "v"):
        for name, op in bad.items():
            p = plan(driver, 2, 3, 64, 64, 62, 62, **dict({"q": good, "k": good, "v": good}, **{which: op}))
            want = {"vec_q": 1, "vec_k": 1, "vec_v": 1}
            want["vec_" + which] = 0
            assert {x: p[x] for x in want} == want, (which, name, p)
    shared = (64, 0, 0, 1)
    p = plan(driver, 2, 3, 64, 64, 64, 64, k=shared, v=shared)
    assert p["vec_k"] == 1 and p["vec_v"] == 1
    # the head dimension itself need not be a multiple of 4: a row's last chunk is read element by element
    assert plan(driver, 2, 3, 7, 200, 33, 1, q=(36, 504, 252, 1))["vec_q"] == 1
