"""The matcher of the products with two batch indices (csrc/host/match.cpp, match_batched2_gemm) and the one rule for their
C (csrc/kernels/gemm_plan.cpp, batched2_c_distinct) on the CPU: a small driver (tests/batched2_driver.cpp) is built with the
host compiler against kd.cpp, match.cpp, gemm_plan.cpp and error.cpp — which shows that the new code needs no HIP — and fed
kernel descriptions written with exprgrad_amd.dsl (tests/multihead_programs.py, tests/batched_programs.py)."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import batched_programs as bp
import multihead_programs as mh
import refcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exprgrad_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("batched2") / "batched2_driver")
    units = [os.path.join(ROOT, "tests", "batched2_driver.cpp")] + [os.path.join(CSRC, u) for u in
                                                                    ("host/kd.cpp", "host/match.cpp", "kernels/gemm_plan.cpp", "error.cpp")]
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC] + units + ["-o", exe],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def run(exe, args, stdin=""):
    out = subprocess.run([exe] + args, input=stdin, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return [dict(kv.split("=", 1) for kv in line.split()) for line in out.stdout.splitlines()]


def rows_of(exe, tmp_path, name, graphs):
    path = str(tmp_path / (name + ".kd"))
    with open(path, "w") as f:
        f.write(refcases.program_text(graphs()))
    return run(exe, ["match", path])


def hits(rows, target):
    return [r for r in rows if r["target"] == target and r["match"] == "1"]


def test_scores_forward_is_nt_with_q_as_a(driver, tmp_path):
    rows = rows_of(driver, tmp_path, "scores", mh.scores_forward)
    assert len(rows) == 1 and rows[0]["loops"] == "5" and rows[0]["match"] == "1", rows
    r = rows[0]
    assert (r["ta"], r["tb"], r["a"], r["b"]) == ("0", "1", "q", "kk"), r
    # q[b,i,h,k]: batch registers b, h at dimensions 0, 2, the row register i at 1; kk alike; s[b,h,i,j]: 0, 1 and i at 2
    assert (r["a_batch"], r["a_row"], r["b_batch"], r["b_row"], r["c_batch"], r["c_row"]) == ("0,2", "1", "0,2", "1", "0,1", "2"), r


def test_context_forward_is_nn_with_p_as_a(driver, tmp_path):
    rows = rows_of(driver, tmp_path, "context", mh.context_forward)
    assert len(rows) == 1 and rows[0]["match"] == "1", rows
    r = rows[0]
    assert (r["ta"], r["tb"], r["a"], r["b"]) == ("0", "0", "p", "v"), r
    # the write names its batch registers b, h in that order: p[b,h,i,j] 0, 1; v[b,j,h,d] 0, 2 with the row j at 1; o[b,i,h,d] 0, 2, row i at 1
    assert (r["a_batch"], r["a_row"], r["b_batch"], r["b_row"], r["c_batch"], r["c_row"]) == ("0,1", "2", "0,2", "1", "0,2", "1"), r


def test_training_step_holds_three_products(driver, tmp_path):
    """fit: the forward product NT (A = q), the gradient of q = gs * kk (NN, A = the gradient of the scores: its last
    register j is contracted, kk[b,j,h,k] ends in n = k) and the gradient of kk = gs^T * q (TN, A = the gradient of the
    scores read along i, q[b,i,h,k] ends in n = k)."""
    rows = rows_of(driver, tmp_path, "training", mh.scores_training(2, 3, 33, 20, 16))
    fit = hits(rows, "fit")
    assert all(r["match"] == "0" for r in rows if r["loops"] != "5")
    assert sorted((r["ta"], r["tb"]) for r in fit) == [("0", "0"), ("0", "1"), ("1", "0")], fit
    by = {(r["ta"], r["tb"]): r for r in fit}
    assert (by["0", "1"]["a"], by["0", "1"]["b"]) == ("q", "kk")
    assert by["0", "0"]["b"] == "kk" and by["1", "0"]["b"] == "q"
    # A of both gradients is one tensor, the gradient of the scores, which is neither parameter
    assert by["0", "0"]["a"] == by["1", "0"]["a"] and by["0", "0"]["a"] not in ("q", "kk")
    assert len(hits(rows, "out")) == 1


@pytest.mark.parametrize("name", sorted(mh.NEAR_MISSES))
def test_near_misses_stay_generated(driver, tmp_path, name):
    rows = rows_of(driver, tmp_path, name, mh.NEAR_MISSES[name])
    assert len(rows) == 1 and rows[0]["match"] == "0", rows


def test_rank3_programs_do_not_match(driver, tmp_path):
    programs = {"forward": bp.batched_forward, "training": bp.batched_training(5, 33, 20, 17), "shared": bp.shared_training(10, 24, 8)}
    programs.update(bp.NEAR_MISSES)
    for name, graphs in programs.items():
        rows = rows_of(driver, tmp_path, "r3_" + name, graphs)
        assert rows and all(r["match"] == "0" for r in rows), (name, rows)


def crule(exe, cases):
    rows = run(exe, ["crule"], "".join(" ".join(str(v) for v in c) + "\n" for c in cases))
    assert len(rows) == len(cases)
    return [r["ok"] == "1" for r in rows]


# batch0 stride_c0 batch1 stride_c1 M ldc N
B, H, M, D = 2, 3, 33, 20
ACCEPTED = {
    "nested dense": (B, H * M * D, H, M * D, M, D, D),
    "padded": (B, H * (M * (D + 3) + 5) + 7, H, M * (D + 3) + 5, M, D + 3, D),
    "interleaved o[b,i,h,d]": (B, M * H * D, H, D, M, H * D, D),
    "one item, ldc = N": (1, 0, 1, 0, M, D, D),
    "one row, any ldc": (B, H * D, H, D, 1, 0, D),
}
REJECTED = {
    "ldc = N - 1": (B, H * M * D, H, M * D, M, D - 1, D),
    "interleaved, stride_c1 = D - 1": (B, M * H * D, H, D - 1, M, H * D, D),
    "equal batch strides": (B, M * D, H, M * D, M, D, D),
    "zero stride, extent above 1": (B, 0, H, M * D, M, D, D),
    "zero inner stride, extent above 1": (B, H * M * D, H, 0, M, D, D),
    "outer stride one short of the span": (B, H * M * D - 1, H, M * D, M, D, D),
    "interleaved, outer one short": (B, M * H * D - 1, H, D, M, H * D, D),
    "negative ldc": (B, H * M * D, H, M * D, M, -D, D),
}


def test_c_rule_accepts(driver):
    assert crule(driver, list(ACCEPTED.values())) == [True] * len(ACCEPTED), list(ACCEPTED)


def test_c_rule_rejects(driver):
    assert crule(driver, list(REJECTED.values())) == [False] * len(REJECTED), list(REJECTED)


def test_c_rule_accepts_what_the_one_index_entry_accepts(driver):
    """Nested strides (stride_c0 = batch1 * stride_c1): accepted exactly when eg_sgemm_batched's two tests hold for
    batch0 * batch1 items, ldc >= N and stride_c >= (M - 1) * ldc + N wherever there is a second item."""
    cases, want = [], []
    for b0, b1, m, n, ldc, sc in itertools.product((1, 2), (1, 3), (1, 4), (1, 5), (0, 1, 4, 5, 6), (0, 15, 19, 20, 21, 26)):
        cases.append((b0, b1 * sc, b1, sc, m, ldc, n))
        want.append((m == 1 or ldc >= n) and (b0 * b1 == 1 or sc >= (m - 1) * ldc + n))
    # (one row: the one-index entry still wants ldc >= N, which addresses nothing; the rule drops the axis)
    got = crule(driver, cases)
    assert got == want, [c for c, g, w in zip(cases, got, want) if g != w][:5]


def test_c_rule_never_accepts_a_repeated_address(driver):
    """Every small random layout against the enumeration of its addresses.  The rule is sufficient, not necessary: it
    may reject a layout without a repeated address, and the count of those is printed."""
    rng = np.random.default_rng(2)
    cases = []
    for _ in range(600):
        b0, b1, m, n = (int(v) for v in rng.integers(1, 5, 4))
        s0, s1, ldc = (int(v) for v in rng.integers(0, 41, 3))
        cases.append((b0, s0, b1, s1, m, ldc, n))
    got = crule(driver, cases)
    accepted = rejected_distinct = 0
    for c, ok in zip(cases, got):
        b0, s0, b1, s1, m, ldc, n = c
        addr = [o * s0 + i * s1 + r * ldc + x for o in range(b0) for i in range(b1) for r in range(m) for x in range(n)]
        distinct = len(set(addr)) == len(addr)
        assert distinct or not ok, c
        accepted += ok
        rejected_distinct += distinct and not ok
    print("accepted", accepted, "of", len(cases), "| rejected although no address repeats:", rejected_distinct)
    assert accepted >= 20    # the draw reaches the accepting side too
