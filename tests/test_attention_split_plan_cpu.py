"""plan_attention_split (csrc/kernels/attention_plan.cpp) without a device: a driver built from that unit alone prints the plan of
a problem — the mode, the key tiles and the effective splits, each split's tile range, the workspace, the partial launch's
cut, the combine launch and the LDS bytes."""
import os
import subprocess

import pytest

from test_attention_grad_plan_cpu import CSRC, ROOT


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("attention_split_plan") / "attention_split_plan_driver")
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "attention_split_plan_driver.cpp"),
                          os.path.join(CSRC, "kernels", "attention_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def plan(exe, b0, b1, I, J, K, D, splits, cus=256):
    out = subprocess.run([exe] + [str(x) for x in (b0, b1, I, J, K, D, cus, splits)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    head, reason = lines[0].split(" reason=")
    p = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in head.split()}
    p["reason"] = reason
    p["ranges"] = [tuple(int(x) for x in line.split()[1:]) for line in lines[1:]]
    return p


@pytest.mark.parametrize("I,rows16", [(1, 1), (16, 1), (17, 0), (70, 0)])
def test_the_mode_changes_between_16_and_17_rows(driver, I, rows16):
    p = plan(driver, 2, 3, I, 640, 64, 128, 5)
    tiles_i = (I + 63) // 64
    assert p["supported"] and p["rows16"] == rows16 and not p["forward"] and p["splits"] == 5 and p["tiles"] == 5 * tiles_i and p["grid"] == 30 * tiles_i
    assert p["rows_pad"] == (16 if rows16 else 64 * tiles_i)
    # O parts [items][splits][rows_pad][dp], then two rows of stats per (item, split)
    assert p["stats_offset"] == 6 * 5 * p["rows_pad"] * 128 and p["workspace"] == 4 * (p["stats_offset"] + 6 * 5 * 2 * p["rows_pad"])
    assert p["combine_rows"] == 6 * p["rows_pad"] and p["combine_rows_per_block"] == 8 and p["combine_grid"] == -(-p["combine_rows"] // 8)
    assert (p["lds"] < p["lds64"]) if rows16 else (p["lds"] == p["lds64"])


@pytest.mark.parametrize("J,splits,want", [(200, 3, 3), (200, 4, 4), (200, 1000, 4), (64, 7, 1), (0, 3, 1), (65, 2, 2)])
def test_splits_are_clamped_to_the_key_tiles_and_the_ranges_tile_them(driver, J, splits, want):
    for I in (16, 70):
        p = plan(driver, 1, 2, I, J, 20, 12, splits)
        nt = (J + 63) // 64
        assert p["supported"] and p["nt"] == nt and p["splits"] == want and len(p["ranges"]) == want
        if nt:
            assert p["ranges"][0][0] == 0 and p["ranges"][-1][1] == nt and all(a < b for a, b in p["ranges"])
            assert all(p["ranges"][s][1] == p["ranges"][s + 1][0] for s in range(want - 1))
        # nothing to split: eg_attention_stable; the 16-row mode runs its own pair of kernels also with one split
        assert p["forward"] == (J == 0 or (I > 16 and want == 1)) and (not p["forward"] or p["workspace"] == 0)


@pytest.mark.parametrize("dims", [(128, 1, 512, 512, 64, 64), (16, 16, 1, 8192, 128, 128), (256, 1, 16, 8192, 64, 64), (1, 8, 128, 64, 64, 64),
                                  (32, 1, 16, 64, 64, 64)])
def test_auto_does_not_split_a_full_machine_or_a_single_key_tile(driver, dims):
    p = plan(driver, *dims, 0)
    assert p["supported"] and p["splits"] == 1


@pytest.mark.parametrize("dims", [(32, 1, 1, 8192, 128, 128), (1, 8, 128, 16384, 64, 64), (1, 1, 16, 200, 16, 16)])
def test_auto_splits_an_idle_machine_within_its_limits(driver, dims):
    p = plan(driver, *dims, 0)
    blocks = p["items"] * p["tiles_i"]
    assert 1 <= p["splits"] <= p["nt"] and blocks * p["splits"] <= 2 * 256 + blocks
    assert p["nt"] < 8 or p["splits"] > 1
    assert all(a < b for a, b in p["ranges"])


def test_more_blocks_per_item_than_a_launch_has_is_refused(driver):
    p = plan(driver, 1, 1, 64 * 4096, 64 * 2048, 32, 32, 2048)
    assert not p["supported"] and "splits" in p["reason"] and 4096 * 2048 > p["max_blocks"]
    assert not plan(driver, 1, 1, 16, 640, 32, 32, -1)["supported"]
    assert plan(driver, 1, 1, 64 * 4096, 64 * 1024, 32, 32, 1024)["supported"]
