"""plan_attention_grad (csrc/kernels/attention_plan.cpp) without a device: a driver built from that unit alone prints the plan
of a problem — supported or not and why, the padded head dimensions, the access width of each of the nine operands, and for
each of the two kernels its blocks, its cut into launches and its LDS bytes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exprgrad_amd", "csrc")
LDS_PER_CU = 163840
OPERANDS = ("q", "k", "v", "o", "s", "do", "dq", "dk", "dv")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("attention_grad_plan") / "attention_grad_plan_driver")
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "attention_grad_plan_driver.cpp"),
                          os.path.join(CSRC, "kernels", "attention_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def dense(b1, R, C):
    """[b0, b1, R, C] nested, 16-byte aligned: (ld, stride0, stride1, aligned)"""
    return (C, b1 * R * C, R * C, 1)


def plan(exe, b0, b1, I, J, K, D, **changed):
    ops = {"q": dense(b1, I, K), "k": dense(b1, J, K), "v": dense(b1, J, D), "o": dense(b1, I, D), "s": (0, b1 * I, I, 1), "do": dense(b1, I, D),
           "dq": dense(b1, I, K), "dk": dense(b1, J, K), "dv": dense(b1, J, D)}
    ops.update(changed)
    out = subprocess.run([exe] + [str(x) for x in (b0, b1, I, J, K, D) + tuple(y for name in OPERANDS for y in ops[name])], capture_output=True,
                         text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    head, reason = lines[0].split(" reason=")
    p = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in head.split()}
    p["reason"] = reason
    for kernel in ("dq", "dkv"):
        p[kernel] = [tuple(int(x) for x in line.split()[1:]) for line in lines[1:] if line.split()[0] == kernel]
    return p


@pytest.mark.parametrize("K,D", [(129, 64), (64, 129), (129, 129), (4096, 8)])
def test_head_dimensions_above_128_are_unsupported(driver, K, D):
    p = plan(driver, 2, 3, 70, 70, K, D)
    assert p["supported"] == 0 and "128" in p["reason"], p
    assert p["reason"].startswith("K" if K > 128 else "D"), p


@pytest.mark.parametrize("n,padded", [(0, 32), (1, 32), (32, 32), (33, 64), (64, 64), (65, 128), (128, 128)])
def test_the_table_of_padded_dimensions(driver, n, padded):
    assert plan(driver, 2, 3, 70, 70, n, 16)["kp"] == padded
    assert plan(driver, 2, 3, 70, 70, 16, n)["dp"] == padded


def test_every_instantiation_fits_the_lds(driver):
    out = subprocess.run([driver, "lds"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    rows = [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]
    assert sorted((kp, dp) for kp, dp, _, _ in rows) == [(kp, dp) for kp in (32, 64, 128) for dp in (32, 64, 128)]
    for kp, dp, dq, dkv in rows:
        # rows of width + 20 for tiles read both ways, width + 4 for the dQ kernel's V tile, the waves' [4][16][68], 64 x 2 floats
        assert dq == 4 * (64 * (kp + 20) + 64 * (dp + 4) + 4 * 16 * 68 + 128)
        assert dkv == 4 * (64 * (kp + 20) + 64 * (dp + 20) + 4 * 16 * 68 + 128)
        assert 0 < dq <= LDS_PER_CU and 0 < dkv <= LDS_PER_CU
        p = plan(driver, 2, 3, 70, 70, kp, dp)
        assert (p["supported"], p["dq_lds"], p["dkv_lds"], p["block"]) == (1, dq, dkv, 256)


@pytest.mark.parametrize("b0,b1,I,J", [(2, 3, 33, 70), (1, 1, 1, 1), (8, 16, 512, 2048), (3, 2, 64, 65), (1, 1, 200, 7), (5, 1, 0, 9), (5, 1, 9, 0)])
def test_the_grids_are_items_times_tiles(driver, b0, b1, I, J):
    p = plan(driver, b0, b1, I, J, 16, 16)
    ti, tj = -(-I // 64), -(-J // 64)
    assert p["supported"] == 1 and p["items"] == b0 * b1
    assert (p["dq_tile"], p["dq_tiles"], p["dq_grid"]) == (64, ti, b0 * b1 * ti)
    assert (p["dkv_tile"], p["dkv_tiles"], p["dkv_grid"]) == (64, tj, b0 * b1 * tj)
    assert p["dq"] == ([(0, b0 * b1, p["dq_grid"])] if ti else []) and p["dq_launches"] == (1 if ti else 0)
    assert p["dkv"] == ([(0, b0 * b1, p["dkv_grid"])] if tj else []) and p["dkv_launches"] == (1 if tj else 0)


@pytest.mark.parametrize("b0,b1,I,J", [(70000, 70, 1, 130), (70000, 70, 130, 1), (2049, 2048, 64, 64), (1, (1 << 22) + 1, 1, 1)])
def test_the_cut_covers_every_item_once(driver, b0, b1, I, J):
    """past 2^22 blocks the flattened item range is cut, per kernel: by arithmetic only, nothing is launched"""
    p = plan(driver, b0, b1, I, J, 8, 8)
    assert p["supported"] == 1 and max(p["dq_grid"], p["dkv_grid"]) > p["max_blocks"]
    for kernel in ("dq", "dkv"):
        tiles, per = p[kernel + "_tiles"], p[kernel + "_items_per_launch"]
        assert per == max(1, p["max_blocks"] // tiles)
        assert p[kernel + "_launches"] == -(-p["items"] // per) == len(p[kernel])
        assert (p[kernel + "_launches"] > 1) == (p[kernel + "_grid"] > p["max_blocks"])
        nxt = 0
        for first, items, grid in p[kernel]:
            assert first == nxt and items >= 1 and grid == items * tiles and grid <= p["max_blocks"]
            nxt = first + items
        assert nxt == p["items"] == b0 * b1


def test_sixteen_byte_accesses_exactly_under_the_rule(driver):
    """pointer 16-byte aligned, leading dimension and both strides multiples of 4 — per operand, outputs included; a stride
    of 0 qualifies; the row sums have no leading dimension"""
    good = (64, 4096, 64, 1)
    all_good = {name: good for name in OPERANDS}
    p = plan(driver, 2, 3, 64, 64, 64, 64, **all_good)
    assert [p["vec_" + name] for name in OPERANDS] == [1] * 9
    bad = {"pointer": (64, 4096, 64, 0), "ld": (66, 4224, 64, 1), "stride0": (64, 4098, 64, 1), "stride1": (64, 4096, 62, 1)}
    for which in OPERANDS:
        for name, op in bad.items():
            p = plan(driver, 2, 3, 64, 64, 62, 62, **dict(all_good, **{which: op}))
            want = {"vec_" + x: 1 for x in OPERANDS}
            want["vec_" + which] = 0
            assert {x: p[x] for x in want} == want, (which, name, p)
    shared = (64, 0, 0, 1)
    p = plan(driver, 2, 3, 64, 64, 64, 64, k=shared, v=shared)
    assert p["vec_k"] == 1 and p["vec_v"] == 1
    p = plan(driver, 2, 3, 64, 64, 64, 64, s=(0, 192, 64, 1))
    assert p["vec_s"] == 1
    # the head dimension itself need not be a multiple of 4: a row's last chunk is accessed element by element
    p = plan(driver, 2, 3, 7, 200, 33, 1, q=(36, 504, 252, 1), dq=(36, 504, 252, 1))
    assert p["vec_q"] == 1 and p["vec_dq"] == 1
