"""The batched contraction's matcher (csrc/host/match.cpp, match_batched_gemm) and planner (csrc/kernels/gemm_plan.cpp,
plan_gemm_batched) on the CPU: a small driver (tests/batched_match_driver.cpp) is built with the host compiler against
kd.cpp, match.cpp and gemm_plan.cpp — which shows that the new code needs no HIP — and fed kernel descriptions written with
exprgrad_amd.dsl (tests/batched_programs.py)."""
import json
import os
import subprocess

import pytest

import batched_programs as bp
import refcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exprgrad_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("batched") / "batched_match_driver")
    units = [os.path.join(ROOT, "tests", "batched_match_driver.cpp")] + [os.path.join(CSRC, u) for u in
                                                                         ("host/kd.cpp", "host/match.cpp", "kernels/gemm_plan.cpp", "error.cpp")]
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC] + units + ["-o", exe],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def run(exe, args, stdin=""):
    out = subprocess.run([exe] + args, input=stdin, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return [dict(kv.split("=", 1) for kv in line.split()) for line in out.stdout.splitlines()]


def matches(exe, tmp_path, name, graphs):
    """The four-loop kernels of a program's targets, as (target, collapsed, row_k, ta, tb) or (target, None) when unmatched."""
    path = str(tmp_path / (name + ".kd"))
    with open(path, "w") as f:
        f.write(refcases.program_text(graphs()))
    rows = [r for r in run(exe, ["match", path]) if r["loops"] == "4"]
    other = [r for r in run(exe, ["match", path]) if r["loops"] != "4"]
    assert all(r["match"] == "0" for r in other)
    return [(r["target"],) + ((int(r["collapsed"]), int(r["row_k"]), int(r["ta"]), int(r["tb"])) if r["match"] == "1" else (None,)) for r in rows]


def test_the_three_batched_forms(driver, tmp_path):
    assert matches(driver, tmp_path, "forward", bp.batched_forward) == [("out", 0, 0, 0, 0)]
    fit = [m[1:] for m in matches(driver, tmp_path, "training", bp.batched_training(5, 33, 20, 17)) if m[0] == "fit"]
    # forward NN, gradient of a: gout * b^T (NT), gradient of b: a^T * gout (TN)
    assert sorted(fit) == [(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0)]


def test_the_three_shared_weight_forms(driver, tmp_path):
    fit = [m[1:] for m in matches(driver, tmp_path, "shared", bp.shared_training(10, 24, 8)) if m[0] == "fit"]
    # two forwards (M = G * I), the input gradient of the second layer (NT, M = G * I), two weight gradients (TN, K = G * I)
    assert sorted(fit) == [(1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 1), (1, 1, 1, 0), (1, 1, 1, 0)]


@pytest.mark.parametrize("name", sorted(bp.NEAR_MISSES))
def test_near_misses_stay_generated(driver, tmp_path, name):
    assert matches(driver, tmp_path, name, bp.NEAR_MISSES[name]) == [("out", None)]


PLAN_CASES = [  # batch M N K ta tb lda ldb ldc aligned
    (512, 128, 128, 64, 0, 0, 64, 128, 128, 1), (64, 512, 512, 64, 0, 0, 64, 512, 512, 1), (4096, 32, 32, 32, 0, 1, 32, 32, 32, 1),
    (7, 65, 130, 48, 0, 0, 51, 133, 133, 0), (7, 65, 130, 48, 1, 1, 68, 51, 133, 1), (1, 1, 1, 1, 0, 0, 1, 1, 1, 1),
    (70000, 4, 4, 4, 0, 0, 4, 4, 4, 1), (5, 64, 64, 64, 0, 0, 64, 64, 64, 1), (300, 200, 24, 50, 0, 0, 50, 24, 24, 1), (3, 128, 128, 40, 1, 0, 128, 128, 128, 1),
]


def test_batched_plans_keep_their_invariants(driver):
    rows = run(driver, ["plan"], "".join(" ".join(str(v) for v in c) + "\n" for c in PLAN_CASES))
    assert len(rows) == 2 * len(PLAN_CASES)
    for c, first, second in zip(PLAN_CASES, rows[0::2], rows[1::2]):
        batch, M, N, K = c[:4]
        assert first == second, c
        bm, bn, kb = int(first["bm"]), int(first["bn"]), int(first["kb"])
        assert (bm, bn) in ((64, 64),), first   # (the tiles gemm_batched.hip has kernels for)
        assert first["route"] == "generic" and first["splits"] == "1" and first["second"] == "none" and first["workspace_floats"] == "0", first
        assert first["edge_splits"] == "0" and first["tail_tiles"] == "0" and int(first["k_per_split"]) >= K, first
        tiles = -(-M // bm) * -(-N // bn)
        assert int(first["tiles_m"]) * int(first["tiles_n"]) == tiles and int(first["grid"]) == batch * tiles, first
        whole = M % bm == 0 and N % bn == 0 and K % kb == 0
        vec = c[9] == 1 and all(v % 4 == 0 for v in (c[6], c[7], (M if c[4] else K), (K if c[5] else N)))
        # the clamped form exactly for ragged extents (and, as in the plain product, for operands without 16-byte loads)
        assert first["edge"] == ("0" if whole and vec else "1"), (c, first)
        if vec:
            assert (first["edge"] == "1") == (not whole), (c, first)


def test_plain_plans_are_unchanged_by_the_new_code(driver):
    cases = [c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_routes.json")))["cases"]
             if c["mode"] == "exact" and c["switches"] == "-"]
    picked = cases[:: max(1, len(cases) // 10)][:10]
    assert len(picked) == 10 and len({c["expect"]["route"] for c in picked}) >= 3
    lines = "".join("%d %d %d %d %d %d %d %d %d %d %d %d\n" % (c["M"], c["N"], c["K"], c["ta"], c["tb"], c["lda"], c["ldb"], c["ldc"], c["a"], c["b"],
                                                             c["c"], c["bias"]) for c in picked)
    rows = run(driver, ["route"], lines)
    for c, got in zip(picked, rows):
        for key in ("route", "grid", "block", "tiles_m", "tiles_n", "splits", "k_per_split", "edge", "second", "workspace_floats"):
            if key in c["expect"]:
                assert str(got[key]) == str(c["expect"][key]), (c, key, got)
