"""tests/group_cases.py held to itself, without a GPU.

The oracle (oracle/kd.py, float32) and its float64 shadow agree with the plain numpy reference of every case, tensor by
tensor: the shadow within 1e-12, the oracle within 5e-6 of max|reference| (conftest's DIRECT_EXCUSE: closer than that, a correct
backend meets the direct gate of tests/parity.py against the oracle without an entry in the allow-list — at every case shape,
the 65537-row sums included).  The per-member claims of the table are held to analyse_row_kernel, analyse_wide_kernel,
analyse_sample_kernel and the sample generator's member record through tests/group_route_driver.cpp, a host-only program;
and the arithmetic behind the table's boundary claims is asserted.
"""
import os
import subprocess

import numpy as np
import pytest

import group_cases as gc
from conftest import DIRECT_EXCUSE
from generated_cases import rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exprgrad_amd", "csrc")
SHAPES = {}          # one case per (program, shapes): the switches of a case change the plan, not the values
for _c in gc.CASES:
    SHAPES.setdefault((_c.program, tuple(sorted(_c.shapes.items()))), _c.name)
SHAPE_CASES = list(SHAPES.values())

_MODELS = {}


def models(program):
    from oracle import kd
    if program not in _MODELS:
        text = gc.program_text(program)
        _MODELS[program] = (kd.Model(text, threads=4), kd.Model(text, shadow=True), gc.tensor_ids(program))
    return _MODELS[program]


def set_params(model, ids, values):
    for name, v in values.items():
        model.params[ids[name]][...] = v


@pytest.mark.parametrize("name", SHAPE_CASES)
def test_oracle_and_shadow_agree_with_the_numpy_reference(name):
    case = gc.BY_NAME[name]
    ref, exact, ids = models(case.program)
    set_params(ref, ids, case.params())
    set_params(exact, ids, case.params())
    inputs, want = case.inputs(), case.want()
    got32 = np.array(ref.call(case.target, inputs))
    got64 = np.array(exact.call(case.target, inputs))
    assert got32.dtype == np.float32 and got64.dtype == np.float64
    for tensor, w in want.items():
        a32 = got32 if tensor == "out" else ref.last[ids[tensor]]
        a64 = got64 if tensor == "out" else exact.last[ids[tensor]]
        assert a32.shape == w.shape, (name, tensor, a32.shape, w.shape)
        e32, e64 = rel(a32, w), rel(a64, w)
        print("%s %s: oracle %.3g, shadow %.3g from the numpy reference" % (name, tensor, e32, e64))
        assert e64 <= 1e-12, (name, tensor, e64)
        assert e32 <= DIRECT_EXCUSE, (name, tensor, e32)


@pytest.mark.parametrize("batch", [3, 1280])
def test_training_references_agree_with_the_oracle(batch):
    """SAMPLE_T: the hand-written gradient against the oracle's derived kernels."""
    from oracle import kd
    text = gc.program_text("sample_t")
    ids = gc.tensor_ids("sample_t")
    rng = np.random.default_rng(batch)
    inputs = {"x": gc.uniform(rng, batch, gc.ST["I"]), "t": gc.uniform(rng, batch, gc.ST["O"])}
    params = {"w1": gc.uniform(rng, gc.ST["I"], gc.ST["H"]), "b1": gc.uniform(rng, gc.ST["H"]), "w2": gc.uniform(rng, gc.ST["H"], gc.ST["O"])}
    want = gc.ref_sample_training(inputs, params)
    for shadow, tol in ((False, DIRECT_EXCUSE), (True, 1e-12)):
        m = kd.Model(text, shadow=True) if shadow else kd.Model(text)
        set_params(m, ids, params)
        assert rel(m.call("predict", {"x": inputs["x"]}), want["predict"]) <= tol
        assert rel(m.call("loss", inputs), want["loss"]) <= tol
        m.run_backward("train", inputs)
        pairs = dict(m.param_grads("train"))
        for pname in ("w1", "b1", "w2"):
            e = rel(m.last[pairs[ids[pname]]], want[pname])
            print("batch %d %s gradient of %s: %.3g" % (batch, "shadow" if shadow else "oracle", pname, e))
            assert e <= tol, (pname, e)


# ---- the analyses ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("groups") / "group_route_driver")
    units = [os.path.join(ROOT, "tests", "group_route_driver.cpp")] + [os.path.join(CSRC, u) for u in (
        "host/kd.cpp", "host/codegen.cpp", "host/match.cpp", "host/rowfuse_common.cpp", "host/rowfuse_row.cpp", "host/rowfuse_wide.cpp",
        "host/rowfuse_sample.cpp", "host/rowfuse_sample_conv.cpp", "host/rowfuse_small.cpp", "switches.cpp", "error.cpp")]
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC] + units + ["-o", exe],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def analyses(exe, tmp_path, program, target, shapes):
    path = str(tmp_path / (program + ".kd"))
    with open(path, "w") as f:
        f.write(gc.program_text(program))
    args = ["%s=%s" % (k, "x".join(str(d) for d in shp)) for k, shp in shapes.items()]
    out = subprocess.run([exe, path, target] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return [dict(kv.split("=", 1) for kv in line.split()) for line in out.stdout.splitlines()]


def said(row):
    """What the three analyses say of one kernel, in the words of the table's `members`."""
    words = []
    if row["row"] == "1":
        words.append("row raw" if row["row_raw"] == "1" else "row")
    if row["wide"] == "1":
        words.append("wide " + row["wide_kind"] + (" raw" if row["wide_raw"] == "1" else " nocol" if row["wide_col"] == "0" and row["wide_kind"] != "seed" else ""))
    if row["sample"] == "1":
        words.append("sample " + row["member"].replace("_", " "))
    return words


@pytest.mark.parametrize("name", SHAPE_CASES)
def test_member_claims_hold_in_the_analyses(driver, tmp_path, name):
    case = gc.BY_NAME[name]
    rows = analyses(driver, tmp_path, case.program, case.target, case.shapes)
    last = {r["write"]: r for r in rows}         # (a tensor written by several kernels: the members come last)
    assert case.members
    for tensor, claim in case.members.items():
        assert tensor in last, (name, tensor, sorted(last))
        assert claim in said(last[tensor]), (name, tensor, claim, said(last[tensor]))
    if case.program == "chain":
        B, W = case.shapes["a"]
        # the consumer outside the group: no wide and no sample kernel — except at B == W, where its only loop reads as the
        # batch loop and the planner's role checks must end the run (it reads a batch total of the group)
        assert (last["out"]["wide"] == "1") == (B == W and W >= 65), (name, last["out"])
        assert last["rq"]["sample"] == "0"       # a raw sum over the batch: the sample group's run ends in front of it
        if gc.sample_takes_chain_head(B, W):
            assert sum(int(last[n]["sample_work"]) for n in "usmv") == 3 * W + 1 >= gc.SAMPLE_MIN_WORK


def test_the_table_covers_what_it_claims():
    by = gc.BY_NAME
    # the register budget of a wide group: ceil(W / 64) floats each for u, v and cs, one each for rs, rq and rm
    assert gc.wide_state(2624) == 3 * 41 + 3 == 126 <= gc.WIDE_STATE_MAX < 129 == 3 * 42 + 3 == gc.wide_state(2688)
    assert gc.wide_state(2688, gc.CHAIN_ORDER[:7]) == 128 and gc.wide_state(2752, gc.CHAIN_ORDER[:5]) == 3 * 43 == 129
    assert gc.chain_wide_groups(2624) == [list(gc.CHAIN_ORDER)] and gc.chain_wide_groups(2688) == [list(gc.CHAIN_ORDER[:7])]
    assert gc.chain_wide_groups(2752) == gc.chain_wide_groups(4096) == [list(gc.CHAIN_ORDER[:4]), list(gc.CHAIN_ORDER[4:])]
    assert len(by["CHAIN_WIDE_1x2624"].lines) == 1 and len(by["CHAIN_WIDE_1x2752"].lines) == 2 and len(by["CHAIN_WIDE_1x4096"].lines) == 2
    assert by["CHAIN_WIDE_1x2688"].kept == ("u", "s", "v") and by["CHAIN_WIDE_1x4096"].kept == ("s",)
    # 80 totals: above the 64 the in-kernel fold takes; 63 and 15: below
    assert 10 * 8 == 80 > 64 and all("| row_finalize" in by["ROWS_WIDE_TOTALS_%d" % b].lines[0][1] for b in (257, 1000))
    assert 60 + 3 == 63 <= 64 and "| partial rows folded by the last block to arrive" in by["CHAIN_ROWS_257x60"].lines[0][1]
    assert 2 * 60 + 2 + 63 <= gc.LOCAL_BUDGET < 2 * 64 + 2 + 64
    assert len(by["CHAIN_ROWS_257x64"].lines) == 2 and "| row_finalize" in by["CHAIN_ROWS_257x64"].lines[1][1]
    # 65537 rows: 257 blocks, one more than the threads of the block that folds their partial rows
    assert -(-65537 // 256) == 257 and "grid 257 x 256" in by["CHAIN_ROWS_65537x12"].lines[0][1]
    # the row tail: 32768 rows on a grid of 64 blocks are two whole trips of 64 x 256 threads; 256 rows more are not
    assert 32768 == 2 * 64 * 256 and (32768 + 256) % (64 * 256) != 0
    assert "unrolled trips=2" in gc.TAIL_CASES[0][2] and not any("unrolled" in w for w in gc.TAIL_CASES[1][2])
    # which shapes a sample group takes the head of CHAIN at; each of them runs both ways
    assert not gc.sample_takes_chain_head(257, 1000) and gc.sample_takes_chain_head(2, 1365) and not gc.sample_takes_chain_head(1, 4096)
    for c in gc.CASES:
        if c.program == "chain" and c.name.startswith("CHAIN_WIDE"):
            B, W = c.shapes["a"]
            assert gc.sample_takes_chain_head(B, W) == c.name.endswith("SAMPLE"), c.name
            if c.name.endswith("_NOSAMPLE"):
                assert c.name.replace("_NOSAMPLE", "_SAMPLE") in by
    # SAMPLE_F: the item loops of 1536, 750 and 7000 items at 512 threads; 2 x 130 terms against 256; 70 terms over 16 lanes
    assert (1536 // 512, 1536 % 512) == (3, 0) and (750 // 512, 750 % 512) == (1, 238) and 7000 // 512 == 13 > 12
    assert 2 * gc.SF["RR"] > 256 and gc.SF["I"] % 16 == 6
    widths = {c.shapes["a"][1] for c in gc.CASES if c.name.startswith("CHAIN_WIDE")}
    assert {65, 127, 128, 129, 1000, 2048, 2624, 2688, 2752, 4096} <= widths
