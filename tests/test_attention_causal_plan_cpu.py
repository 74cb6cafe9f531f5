"""The causal tile bounds (csrc/kernels/attention_plan.hpp: causal_visible_keys, causal_key_tiles, causal_first_row_tile,
causal_tile_cut) without a device, against a brute-force count over every pair (i, j) with j <= i + offset: the functions the
kernels of eg_attention_causal and eg_attention_causal_grad call."""
import os
import subprocess

import numpy as np
import pytest

from test_attention_grad_plan_cpu import CSRC, ROOT

SIZES = [1, 63, 64, 65, 130, 200]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("attention_causal_plan") / "attention_causal_plan_driver")
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "attention_causal_plan_driver.cpp"),
                          "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


@pytest.mark.parametrize("offset", [0, 1, 63, 64, 65, 199, 500])
def test_bounds_against_brute_force(driver, offset):
    for I in SIZES:
        for J in SIZES:
            out = subprocess.run([driver, str(I), str(J), str(offset)], capture_output=True, text=True, timeout=60)
            assert out.returncode == 0, out.stderr
            lines = out.stdout.splitlines()
            visible = np.arange(J)[None, :] <= np.arange(I)[:, None] + offset
            tiles_i, tiles_j = -(-I // 64), -(-J // 64)
            tile = lambda x, t, u: x[64 * t:64 * t + 64, 64 * u:64 * u + 64]
            assert lines[0] == "visible=%d" % (np.flatnonzero(visible.any(0)).max() + 1), (I, J, lines[0])
            for t in range(tiles_i):
                # the forward and dQ visit exactly the key tiles that hold a visible pair, and select exactly where a masked pair is too
                visited = [u for u in range(tiles_j) if tile(visible, t, u).any()]
                cut = [u for u in visited if not tile(visible, t, u).all()]
                assert visited == list(range(len(visited)))
                assert lines[1 + t] == "row %d key_tiles=%d cut=%s" % (t, len(visited), "".join("%d," % u for u in cut)), (I, J, lines[1 + t])
            for u in range(tiles_j):
                # dK/dV start at the first row tile with a visible row; -1: none has one
                rows = [t for t in range(tiles_i) if tile(visible, t, u).any()]
                assert lines[1 + tiles_i + u] == "key %d first_row_tile=%d" % (u, rows[0] if rows else -1), (I, J, lines[1 + tiles_i + u])
