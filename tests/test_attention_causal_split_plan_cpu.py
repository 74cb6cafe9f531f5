"""plan_attention_causal_split and the decode of a block's index (csrc/kernels/attention_plan.hpp: causal_piece_decode and the
closed form under it) without a device, against a brute-force enumeration of the row tiles, their visible key tiles and their
pieces; and eg_attention_causal_split at the drop-in boundary."""
import os
import subprocess

import pytest

from test_attention_cabi import declaration
from test_attention_grad_plan_cpu import CSRC, ROOT


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("attention_causal_split_plan") / "attention_causal_split_plan_driver")
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "attention_causal_split_plan_driver.cpp"),
                          os.path.join(CSRC, "kernels", "attention_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def plan(exe, *args):
    out = subprocess.run([exe] + [str(x) for x in args], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    head, reason = lines[0].split(" reason=")
    p = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in head.split()}
    p["reason"] = reason
    p["blocks"] = [tuple(int(x) for x in line.split()[1:]) for line in lines[1:]]
    return p


@pytest.mark.parametrize("I", [1, 16, 17, 64, 65, 130, 300])
@pytest.mark.parametrize("chunk", [1, 2, 3, 5, 100])
def test_decode_and_workspace_against_brute_force(driver, I, chunk):
    for J in (1, 64, 65, 200, 400):
        for offset in sorted({0, 1, 37, 64, max(J - I, 0), J, J + 70}):
            p = plan(driver, I, J, offset, chunk)
            rows16 = I <= 16
            # key tiles of a row tile: those that hold a pair (i, j) with j <= i + offset, j < J
            row_tiles = [(0, I)] if rows16 else [(i0, min(i0 + 64, I)) for i0 in range(0, I, 64)]
            n = [min(J - 1, i1 - 1 + offset) // 64 + 1 for _, i1 in row_tiles]
            pieces = [-(-x // min(chunk, max(n))) for x in n]
            want, slot = [], 0
            for t, (x, P) in enumerate(zip(n, pieces)):
                cut = rows16 or P > 1
                want += [(t, s, P, s * x // P, (s + 1) * x // P, slot + s if cut else None) for s in range(P)]
                slot += P if cut else 0
            label = (I, J, offset, chunk)
            assert p["supported"] and p["rows16"] == rows16 and p["pieces"] == len(want) and p["grid"] == 2 * len(want), label
            got = [b[:5] + (b[5] if want_b[5] is not None else None,) for b, want_b in zip(p["blocks"], want[::-1])]
            assert got == want[::-1], label   # every (row tile, piece) once, the heaviest row tile first
            for t, x in enumerate(n):   # disjoint, non-empty, covering [0, n_t)
                ranges = sorted(b[3:5] for b in p["blocks"] if b[0] == t)
                assert ranges[0][0] == 0 and ranges[-1][1] == x and all(a < b for a, b in ranges), label
                assert all(ranges[s][1] == ranges[s + 1][0] for s in range(len(ranges) - 1)), label
            assert p["forward"] == (not rows16 and max(pieces) == 1), label
            assert p["slots"] == slot and p["rows"] == (16 if rows16 else 64), label
            cut_tiles = sum(1 for P in pieces if rows16 or P > 1)
            assert p["first_cut"] == len(n) - cut_tiles and p["combine_rows"] == 2 * cut_tiles * p["rows"], label
            assert p["stats_offset"] == 2 * slot * p["rows"] * p["dp"], label
            assert p["workspace"] == (0 if p["forward"] else 4 * (p["stats_offset"] + 2 * slot * 2 * p["rows"])), label


def test_refused_plans_and_auto(driver):
    assert not plan(driver, 70, 200, 0, -1)["supported"]
    p = plan(driver, 64 * 4096, 64 * 4096, 0, 1, 32, 32, 1, 256)
    assert not p["supported"] and "pieces" in p["reason"]
    # auto: one long sequence on a full machine is eg_attention_causal; a few rows against a long cache are cut to about the CUs
    assert plan(driver, 16384, 16384, 0, 0, 64, 64, 8, 256)["forward"]
    for I in (1, 16, 128):
        p = plan(driver, I, 8192, 8192 - I, 0, 128, 128, 32, 256)
        assert not p["forward"] and 2 <= p["chunk"] < p["nv"] and 128 <= p["grid"] <= 2 * 256 + 32 * p["tiles"], (I, p)


def test_exported_bound_and_wrapped():
    from exprgrad_amd import _lib, ops
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert "eg_attention_causal_split" in {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert "eg_attention_causal_split" in _lib.declared_symbols()
    assert len(_lib.lib().eg_attention_causal_split.argtypes) == 35 == len(declaration("eg_attention_causal_split"))
    assert declaration("eg_attention_causal_split") == declaration("eg_attention_causal") + ["int chunk"]
    assert callable(ops.attention_causal_split)
