"""csrc/switches.hpp held to its header comment, without a GPU.

tests/switches_driver.cpp is a host-only program linked against switches.cpp alone: one truth rule for every flag row (a row
that used to be read by presence included), tuning rows behind EG_TUNING across reloads, a text() pointer that outlives the
reload which supersedes it, generation() counting reloads, eight lock-free readers against a thousand reloads, and the table
itself against the one the parent of the typed ids printed (tests/golden/switch_table_parent.tsv, recorded from its
eg_switch_table): same names, classes and order, same purposes but for the three rows that say they are fixed at first use.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exprgrad_amd", "csrc")
FIXED_AT_FIRST_USE = ("EG_HIPRTC_LIB", "EG_KERNEL_CACHE", "EG_NO_KERNEL_CACHE")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("switches") / "switches_driver")
    units = [os.path.join(ROOT, "tests", "switches_driver.cpp"), os.path.join(CSRC, "switches.cpp")]
    out = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC] + units + ["-o", exe, "-lpthread"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def run(exe, mode):
    env = {k: v for k, v in os.environ.items() if not k.startswith("EG_")}
    out = subprocess.run([exe, mode], capture_output=True, text=True, timeout=120, env=env)
    print(out.stdout[-2000:])
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    return out.stdout


def test_flag_rule_tuning_gate_text_lifetime_and_generation(driver):
    assert run(driver, "rules").strip() == "ok"


def test_table_equals_the_parent_table(driver):
    got = [line.split("\t") for line in run(driver, "table").splitlines()]
    with open(os.path.join(ROOT, "tests", "golden", "switch_table_parent.tsv")) as f:
        want = [line.rstrip("\n").split("\t") for line in f if line.strip()]
    assert len(want) == 87 and all(len(r) == 3 for r in got)
    assert [r[:2] for r in got] == [r[:2] for r in want]
    for g, w in zip(got, want):
        assert g[2] == (w[2] + " (fixed at first use)" if g[0] in FIXED_AT_FIRST_USE else w[2]), g[0]


def test_readers_see_only_published_values_during_reloads(driver):
    assert run(driver, "threads").startswith("ok")


def test_library_prints_the_same_table_as_the_driver(driver):
    from exprgrad_amd import _lib
    assert [list(t) for t in _lib.switch_table()] == [line.split("\t") for line in run(driver, "table").splitlines()]
