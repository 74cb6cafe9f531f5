"""match_attention_fit (csrc/host/match_attention_grad.cpp) without a device: a driver built with the host compiler from
kd.cpp, match.cpp, match_attention.cpp, match_attention_grad.cpp and error.cpp alone prints, for every live position of every
target of a program, the training step found there or the reason of the refusal, and next to it match_attention's answer."""
import os
import subprocess

import pytest

import attention_fit_programs as fit
import attention_fused_programs as fp
import attention_programs as ap
import refcases
from test_attention_match_cpu import REASONS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exprgrad_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("attention_fit_match") / "attention_fit_match_driver")
    units = [os.path.join(ROOT, "tests", "attention_fit_match_driver.cpp")] + [os.path.join(CSRC, u) for u in (
        "host/kd.cpp", "host/match.cpp", "host/match_attention.cpp", "host/match_attention_grad.cpp", "error.cpp")]
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC] + units + ["-o", exe],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def rows(exe, tmp_path, name, text, kind="fit"):
    path = str(tmp_path / (name + ".kd"))
    with open(path, "w") as f:
        f.write(text)
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return [dict(kv.split("=", 1) for kv in line.split()[1:]) for line in out.stdout.splitlines() if line.split()[0] == kind]


def hits(found, target="fit"):
    return [r for r in found if r["target"] == target and r["match"] == "1"]


@pytest.mark.parametrize("name,kwargs,scale,forward,hidden", [
    ("scale_last", {}, "0.125", 5, 7), ("scale_first", {"scale_first": True}, "0.125", 5, 7), ("unscaled", {"scale": None}, "1", 4, 5)])
def test_the_training_program_matches_once(driver, tmp_path, name, kwargs, scale, forward, hidden):
    """all three spellings of the scale: nine tensors, the scale, and every member — thirteen with a scale map, eleven without"""
    text = fit.text_of(fit.training(*fit.SHAPE, **kwargs))
    found = rows(driver, tmp_path, name, text)
    got = hits(found)
    assert len(got) == 1 and not hits(found, "out") and not hits(found, "loss"), found
    g = got[0]
    assert (g["pos"], g["scale"], g["q"], g["kk"], g["v"], g["out"], g["sums"]) == ("0", scale, "q", "kk", "v", "context", "softmax.sums"), g
    # the gradients of the three parameters are the destinations of the program's `gradient` lines
    dest = {}
    for line in text.split("target fit")[1].split("endtarget")[0].splitlines():
        w = line.split()
        if w[:1] == ["gradient"]:
            dest[int(w[1])] = "#" + w[2]
    ids = {n: fit._tensor_id(text, n) for n in ("q", "kk", "v")}
    assert (g["dq"], g["dk"], g["dv"]) == (dest[ids["q"]], dest[ids["kk"]], dest[ids["v"]]), (g, dest)
    assert g["do"].startswith("#") and len({g["do"], g["dq"], g["dk"], g["dv"]}) == 4, g
    fwd, bwd = g["forward"].split(","), g["backward"].split(",")
    assert fwd == [str(i) for i in range(forward)] and len(bwd) == forward + 3 and int(g["members"]) == 2 * forward + 3, g
    assert int(bwd[0]) > int(fwd[-1]) and len(set(bwd)) == len(bwd), g
    names = g["hidden"].split(",")
    assert len(names) == hidden and names[:forward - 2] == (["scores", "scaled", "softmax"] if forward == 5 else ["scores", "softmax"]), g
    assert "softmax.sums" not in names and "context" not in names, g


def test_the_projected_program_matches(driver, tmp_path):
    """q, kk and v are results: the projection of v stands between the softmax and the context, its gradient between the
    gradient kernels, and the three gradients are results that the projections' gradients read"""
    found = rows(driver, tmp_path, "projected", fit.text_of(fit.projected(2, 2, 70, 8, 16, 16)))
    got = hits(found)
    assert len(got) == 1, found
    g = got[0]
    assert (g["scale"], g["q"], g["kk"], g["v"], g["out"], g["sums"], g["members"]) == ("0.125", "q", "kk", "v", "context", "softmax.sums", "13"), g
    fwd, bwd = [int(x) for x in g["forward"].split(",")], [int(x) for x in g["backward"].split(",")]
    assert len(fwd) == 5 and len(bwd) == 8 and fwd[0] == int(g["pos"]) and fwd == sorted(fwd) and bwd == sorted(bwd) and bwd[0] > fwd[-1], g
    assert fwd[-1] - fwd[0] > 4, g          # a kernel that is no member stands inside the chain
    assert len(g["hidden"].split(",")) == 7 and len({g["do"], g["dq"], g["dk"], g["dv"]}) == 4, g


MISSES = fit.near_misses()


@pytest.mark.parametrize("name", sorted(MISSES))
def test_near_misses_are_refused_each_with_its_reason(driver, tmp_path, name):
    text, reason, pos, _ = MISSES[name]
    found = rows(driver, tmp_path, name, text)
    assert found and not hits(found), found
    at = [r for r in found if r["target"] == "fit" and r["pos"] == str(pos)][0]
    assert at["why"] == reason.replace(" ", "_"), at


def test_every_reason_of_the_gradient_half_has_its_near_miss():
    own = {reason for _, reason, _, _ in MISSES.values()}
    source = open(os.path.join(CSRC, "host", "match_attention_grad.cpp")).read()
    for reason in ("a gradient kernel of the chain is missing", "an intermediate or its gradient is read outside the chain and its gradient kernels",
                   "two of the gradients of q, kk and v are one tensor", "a gradient tensor is an operand of the chain",
                   "a gradient kernel does not read its operands in the positions the forward products fix",
                   "a gradient kernel does not compute what derive makes of the chain"):
        assert reason in own and '"%s"' % reason in source, reason
    assert {"an intermediate is the target's output", "an intermediate has another writer"} <= own


# ---- match_attention answers as before ----------------------------------------------------------------------------------------
FORWARD = {"forward": fp.attention_forward(), "unscaled": fp.attention_forward_unscaled, "scale_first": fp.attention_forward_scale_first}


@pytest.mark.parametrize("name", sorted(FORWARD))
def test_match_attention_still_takes_the_forward_programs(driver, tmp_path, name):
    found = rows(driver, tmp_path, name, refcases.program_text(FORWARD[name]()), kind="fwd")
    assert [(r["pos"], r["match"]) for r in found if r["match"] == "1"] == [("0", "1")], found
    assert not hits(rows(driver, tmp_path, name, refcases.program_text(FORWARD[name]())), "out")     # no gradient kernels: no training step


@pytest.mark.parametrize("name", sorted(fp.NEAR_MISSES))
def test_match_attention_still_refuses_its_near_misses_with_the_same_reasons(driver, tmp_path, name):
    found = rows(driver, tmp_path, name, refcases.program_text(fp.NEAR_MISSES[name][0]()), kind="fwd")
    assert found and not [r for r in found if r["match"] == "1"], found
    assert [r for r in found if r["pos"] == "0"][0]["why"] == REASONS[name], found


def test_match_attention_still_refuses_every_fit_target(driver, tmp_path):
    found = rows(driver, tmp_path, "training", refcases.program_text(ap.attention_training(*ap.TRAINING_SHAPE)()), kind="fwd")
    assert [r["pos"] for r in found if r["target"] == "out" and r["match"] == "1"] == ["0"], found
    fit_rows = [r for r in found if r["target"] == "fit"]
    assert fit_rows and all(r["match"] == "0" for r in fit_rows) and fit_rows[0]["why"] == "an_intermediate_is_read_outside_the_chain", fit_rows
