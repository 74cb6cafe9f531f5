"""plan_attention_f64 (csrc/kernels/attention_plan.cpp) without a device, reached the way tests/test_attention_plan_cpu.py
reaches plan_attention: a driver built from that unit alone prints the float64 plan of a problem and the float32 plan of the
same problem.

What float64 decides in the planner: the key tile (64 keys, or 32 where the three LDS tiles of 64 do not fit the 160 KiB of a
CU), the LDS bytes in doubles, and 16-byte loads under the even / aligned rule of eg_dgemm_batched2.  The cut is the item
grid's, and the float32 plans are what they were."""
import os
import subprocess

import pytest

from test_attention_plan_cpu import CSRC, LDS_PER_CU, ROOT, dense, driver as f32_driver, plan as f32_plan     # noqa: F401 (a fixture)

PADS = (32, 64, 128)
PAIRS = [(kp, dp) for kp in PADS for dp in PADS]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("attention_f64_plan") / "attention_f64_plan_driver")
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "attention_f64_plan_driver.cpp"),
                          os.path.join(CSRC, "kernels", "attention_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def plans(exe, b0, b1, I, J, K, D, q=None, k=None, v=None):
    """(the float64 plan, the float32 plan) of one problem"""
    ops = [q or dense(b1, I, K), k or dense(b1, J, K), v or dense(b1, J, D)]
    out = subprocess.run([exe] + [str(x) for x in (b0, b1, I, J, K, D) + tuple(y for o in ops for y in o)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    got = {}
    for line in lines[:2]:
        which, rest = line.split(" ", 1)
        head, reason = rest.split(" reason=")
        p = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in head.split()}
        p["reason"] = reason
        got[which] = p
    got["f64"]["launch"] = [tuple(int(x) for x in line.split()[1:]) for line in lines[2:]]
    return got["f64"], got["f32"]


def lds_f64(kp, dp, tj):
    """K rows [tj][kp + 2], V rows [tj][dp + 16], E rows [4 waves][16][tj + 18], in doubles"""
    return 8 * (tj * (kp + 2) + tj * (dp + 16) + 4 * 16 * (tj + 18))


@pytest.mark.parametrize("kp,dp", PAIRS)
def test_the_key_tile_is_the_largest_that_fits(driver, kp, dp):
    """at the smallest and the largest K and D of the pair"""
    for K, D in ((kp // 2 + 1, dp // 2 + 1), (kp, dp)):
        p, _ = plans(driver, 2, 3, 70, 130, K, D)
        assert p["supported"] == 1 and p["reason"] == "" and (p["kp"], p["dp"]) == (kp, dp), p
        assert p["tile_i"] == 64 and p["block"] == 256 and p["tile_j"] in (64, 32)
        assert p["lds"] == lds_f64(kp, dp, p["tile_j"]) and 0 < p["lds"] <= LDS_PER_CU
        assert (p["lds64"], p["lds32"]) == (lds_f64(kp, dp, 64), lds_f64(kp, dp, 32)) and p["key_tile"] == p["tile_j"]
        assert p["tile_j"] == (64 if lds_f64(kp, dp, 64) <= LDS_PER_CU else 32), p


def test_only_the_largest_pair_steps_down_to_32_keys(driver):
    """with the f32 row paddings 64 keys at (128, 128) would need 176 128 bytes; in doubles with these rows, 182 272"""
    tiles = {pair: plans(driver, 1, 1, 64, 64, *pair)[0]["tile_j"] for pair in PAIRS}
    assert tiles == {pair: 32 if pair == (128, 128) else 64 for pair in PAIRS}
    assert lds_f64(128, 128, 64) > LDS_PER_CU >= lds_f64(128, 128, 32)


@pytest.mark.parametrize("K,D", [(129, 64), (64, 129), (129, 129), (4096, 8)])
def test_head_dimensions_above_128_are_unsupported(driver, K, D):
    p, _ = plans(driver, 2, 3, 70, 70, K, D)
    assert p["supported"] == 0 and "128" in p["reason"], p


def test_sixteen_byte_loads_exactly_under_the_even_rule(driver):
    """pointer 16-byte aligned, leading dimension and both strides even — per operand; a stride of 0 qualifies; a multiple of
    2 that is no multiple of 4 qualifies for doubles where it does not for floats"""
    good = (66, 4226, 66, 1)
    both = plans(driver, 2, 3, 64, 64, 62, 62, q=good, k=good, v=good)
    assert [both[0][x] for x in ("vec_q", "vec_k", "vec_v")] == [1, 1, 1]
    assert [both[1][x] for x in ("vec_q", "vec_k", "vec_v")] == [0, 0, 0]
    bad = {"pointer": (66, 4226, 66, 0), "ld": (67, 4288, 66, 1), "stride0": (66, 4227, 66, 1), "stride1": (66, 4226, 65, 1)}
    for which in ("q", "k", "v"):
        for name, op in bad.items():
            p, _ = plans(driver, 2, 3, 64, 64, 62, 62, **dict({"q": good, "k": good, "v": good}, **{which: op}))
            want = {"vec_q": 1, "vec_k": 1, "vec_v": 1}
            want["vec_" + which] = 0
            assert {x: p[x] for x in want} == want, (which, name, p)
    shared = (64, 0, 0, 1)
    p, _ = plans(driver, 2, 3, 64, 64, 64, 64, k=shared, v=shared)
    assert p["vec_k"] == 1 and p["vec_v"] == 1
    # the head dimension itself need not be even: a row's odd last element is read alone
    assert plans(driver, 2, 3, 7, 200, 33, 1, q=(34, 476, 238, 1))[0]["vec_q"] == 1


@pytest.mark.parametrize("b0,b1,I", [(2, 3, 33), (1, 1, 1), (3, 2, 64), (1, 2, 130), (70000, 70, 130), (1, (1 << 22) + 1, 1)])
def test_the_cut_is_the_item_grids(driver, b0, b1, I):
    """items x row tiles of 64 query rows, cut into launches of at most 2^22 blocks exactly as for float32"""
    p, p32 = plans(driver, b0, b1, I, 70, 16, 16)
    tiles = -(-I // 64)
    assert p["supported"] == 1 and p["tiles_i"] == tiles and p["items"] == b0 * b1 and p["grid"] == b0 * b1 * tiles
    assert p["items_per_launch"] == max(1, p["max_blocks"] // tiles) and p["launches"] == -(-p["items"] // p["items_per_launch"])
    for key in ("tiles_i", "items", "grid", "items_per_launch", "launches"):
        assert p[key] == p32[key], key
    if p["launches"] <= 64:
        nxt = 0
        for first, items, grid in p["launch"]:
            assert first == nxt and items >= 1 and grid == items * tiles and grid <= p["max_blocks"]
            nxt = first + items
        assert nxt == b0 * b1 and len(p["launch"]) == p["launches"]


@pytest.mark.parametrize("K,D", [(128, 128), (128, 1), (1, 128), (64, 64), (0, 16), (33, 1), (129, 8)])
def test_the_f32_plans_are_what_they_were(driver, f32_driver, K, D):
    """plan_attention beside plan_attention_f64 in one process gives what the float32 driver alone gives, and that is the
    one tile of 64 keys with the float32 rows"""
    q = (K + 4 - K % 4, 3 * 70 * (K + 4), 70 * (K + 4), 1)
    _, p32 = plans(driver, 2, 3, 70, 70, K, D, q=q)
    alone = f32_plan(f32_driver, 2, 3, 70, 70, K, D, q=q)
    for key, value in alone.items():
        if key != "launch":
            assert p32[key] == value, key
    if alone["supported"]:
        assert p32["tile_j"] == 64 and p32["lds"] == 4 * (64 * (p32["kp"] + 4) + 64 * (p32["dp"] + 16) + 4 * 16 * 68)
