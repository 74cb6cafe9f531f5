"""The float64 convolution planner (csrc/kernels/gemm_plan.cpp: plan_conv64) on the CPU: a small driver
(tests/conv64_plan_driver.cpp) is built with the host compiler against gemm_plan.cpp alone and fed one call per line.
What is checked is what a wrong answer would break on the GPU: a tile missing or run twice, a 16-byte load of a misaligned
address, pixels of the filter gradient summed twice or not at all, slabs written past the workspace, a block id mapped
outside the launch, and a 32-bit index that wraps."""
import os
import subprocess

import pytest

import conv64_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exprgrad_amd", "csrc")
FWD, GIMG, GFLT = 1, 2, 3
KTILE = 16


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("conv64") / "conv64_plan_driver")
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(CSRC, "kernels", "gemm_plan.cpp"),
                          os.path.join(ROOT, "tests", "conv64_plan_driver.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def plans(exe, calls):
    """calls: (role, shape, img_aligned, flt_aligned, gout_aligned, cus) -> [plan, ...]"""
    text = "".join(" ".join(str(int(v)) for v in (role, *shape, ia, fa, ga, cus)) + "\n" for role, shape, ia, fa, ga, cus in calls)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = [{k: int(v) for k, v in (f.split("=", 1) for f in line.split()[1:])} for line in out.stdout.splitlines()]
    assert len(rows) == len(calls)
    return rows


def call(role, shape, ia=1, fa=1, ga=1, cus=256):
    return (role, shape, ia, fa, ga, cus)


def contraction(role, shape):
    N, H, W, C, F, FH, FW = shape
    P = N * (H - FH + 1) * (W - FW + 1)
    return {FWD: (P, F, FH * FW * C), GIMG: (N * H * W, C, FH * FW * F), GFLT: (F, FH * FW * C, P)}[role]


SHAPES = cc.CASES + [(1, 256, 256, 64, 64, 3, 3), (32, 28, 28, 32, 64, 3, 3), (3, 12, 12, 24, 20, 3, 3), (64, 66, 66, 128, 256, 3, 3)]


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_tiles_cover_the_output_exactly_once(driver, cus):
    calls = [call(role, s, cus=cus) for s in SHAPES for role in (FWD, GIMG, GFLT)]
    for (role, s, *_), p in zip(calls, plans(driver, calls)):
        M, N, K = contraction(role, s)
        assert p["ok"] == 1 and (p["M"], p["N"], p["K"]) == (M, N, K), (role, s, p)
        assert (p["config"], p["bm"], p["bn"]) in ((0, 128, 128), (2, 64, 64)) and (p["wr"], p["wc"]) == (2, 4)
        # tile (i, j) is rows [i * bm, ...), columns [j * bn, ...): a cover without overlap needs exactly ceil counts
        assert p["tiles_m"] == -(-M // p["bm"]) and p["tiles_n"] == -(-N // p["bn"])
        assert p["grid_x"] == p["tiles_m"] * p["tiles_n"] and p["grid_y"] == p["slices"] >= 1
        # the kernel's remap (tile = (id & 7) * (grid >> 3) + (id >> 3)) is a permutation of [0, grid) only for a multiple of 8
        assert p["remap"] == int(p["grid_x"] % 8 == 0 and p["grid_x"] >= 16), (role, s, p)
        if p["remap"]:
            g = p["grid_x"]
            assert sorted((b & 7) * (g >> 3) + (b >> 3) for b in range(g)) == list(range(g))
        assert p["aux_doubles"] == (s[3] * s[5] * s[6] * s[4] if role == GIMG else 0)


def test_remap_occurs_and_does_not(driver):
    got = plans(driver, [call(FWD, (1, 34, 34, 32, 32, 3, 3)), call(FWD, (1, 9, 10, 17, 17, 3, 3)), call(GFLT, (1, 256, 256, 64, 64, 3, 3))])
    assert [p["remap"] for p in got] == [1, 0, 0] and got[0]["grid_x"] == 16 and got[2]["grid_x"] == 9


def test_sixteen_byte_loads(driver):
    even, odd_c, odd_f = (2, 12, 11, 24, 40, 3, 3), (2, 12, 11, 17, 40, 3, 3), (2, 12, 11, 24, 33, 3, 3)
    cases = {
        "forward, all even and aligned": (call(FWD, even), (1, 1)),
        "forward, odd C: the window and the bank's rows (K odd)": (call(FWD, odd_c), (0, 0)),
        "forward, odd F alone does not matter": (call(FWD, odd_f), (1, 1)),
        "forward, image not aligned": (call(FWD, even, ia=0), (0, 1)),
        "forward, bank not aligned": (call(FWD, even, fa=0), (1, 0)),
        "forward, gout's alignment is not its business": (call(FWD, even, ga=0), (1, 1)),
        "filter gradient, all even and aligned": (call(GFLT, even), (1, 1)),
        "filter gradient, odd C: the window": (call(GFLT, odd_c), (1, 0)),
        "filter gradient, odd F: gout's rows": (call(GFLT, odd_f), (0, 1)),
        "filter gradient, image not aligned": (call(GFLT, even, ia=0), (1, 0)),
        "filter gradient, gout not aligned": (call(GFLT, even, ga=0), (0, 1)),
        "image gradient, all even and aligned": (call(GIMG, even), (1, 1)),
        "image gradient, odd F: the window of gout and the flipped bank's rows": (call(GIMG, odd_f), (0, 0)),
        "image gradient, odd C alone does not matter": (call(GIMG, odd_c), (1, 1)),
        "image gradient, gout not aligned": (call(GIMG, even, ga=0), (0, 1)),
        "image gradient, the bank is read from the flipped copy": (call(GIMG, even, fa=0), (1, 1)),
    }
    got = plans(driver, [c for c, _ in cases.values()])
    for (name, (_, want)), p in zip(cases.items(), got):
        assert (p["vec_a"], p["vec_b"]) == want, (name, p)


@pytest.mark.parametrize("cus", [1, 64, 256, 304])
def test_filter_gradient_slices_cover_the_pixels_exactly_once(driver, cus):
    calls = [call(GFLT, s, cus=cus) for s in SHAPES + [(1, 19, 18, 24, 20, 3, 3), (1, 258, 3, 17, 17, 3, 3), (7, 31, 29, 20, 24, 2, 4)]]
    sliced = 0
    for (_, s, *_), p in zip(calls, plans(driver, calls)):
        F, taps, P = contraction(GFLT, s)
        per, n = p["pixels_per_slice"], p["slices"]
        assert per > 0 and per % KTILE == 0
        bounds = [(i * per, min(P, (i + 1) * per)) for i in range(n)]      # the kernel: [y * per, min(K, y * per + per))
        assert bounds[0][0] == 0 and bounds[-1][1] == P and all(b > a for a, b in bounds)
        assert all(bounds[i][1] == bounds[i + 1][0] and bounds[i][1] % KTILE == 0 for i in range(n - 1))
        if n == 1:
            assert p["reduce"] == 0 and p["workspace_doubles"] == 0
        else:
            sliced += 1
            assert p["reduce"] == 1 and p["workspace_doubles"] == n * F * taps == n * s[4] * s[5] * s[6] * s[3]
    assert sliced > 0 or cus == 1     # (one compute unit: a few tiles fill it)


def test_the_sliced_case_slices_on_256_compute_units(driver):
    p, = plans(driver, [call(GFLT, cc.SLICED_CASE, cus=256)])
    assert p["slices"] > 1 and p["reduce"] == 1


def test_forward_and_image_gradient_never_slice(driver):
    calls = [call(role, s, cus=cus) for s in SHAPES for role in (FWD, GIMG) for cus in (1, 256)]
    for p in plans(driver, calls):
        assert p["slices"] == 1 and p["reduce"] == 0 and p["workspace_doubles"] == 0 and p["grid_y"] == 1


def test_indices_of_2_to_the_31_are_refused(driver):
    """The kernels hold pixels and taps in 32 bits: a contraction with 2^31 rows, columns or terms is not planned."""
    lim = 1 << 31
    cases = {
        "forward, P = 2^31": (call(FWD, (lim, 1, 2, 17, 17, 1, 2)), 0),
        "forward, P = 2^31 - 1": (call(FWD, (lim - 1, 1, 2, 17, 17, 1, 2)), 1),
        "forward, K = 2^31": (call(FWD, (1, 1, 2, lim // 2, 17, 1, 2)), 0),
        "filter gradient, P = 2^31": (call(GFLT, (lim, 1, 2, 17, 17, 1, 2)), 0),
        "filter gradient, taps = 2^31": (call(GFLT, (1, 1, 2, lim // 2, 17, 1, 2)), 0),
        "image gradient, N*H*W = 2^31": (call(GIMG, (lim // 2, 1, 2, 17, 17, 1, 2)), 0),
        "image gradient, N*H*W = 2^31 - 2": (call(GIMG, (lim // 2 - 1, 1, 2, 17, 17, 1, 2)), 1),
        "image gradient, K = FH*FW*F = 2^31": (call(GIMG, (1, 1, 2, 17, lim // 2, 1, 2)), 0),
    }
    got = plans(driver, [c for c, _ in cases.values()])
    for (name, (_, want)), p in zip(cases.items(), got):
        assert p["ok"] == want and p["max_index"] == lim, (name, p)
