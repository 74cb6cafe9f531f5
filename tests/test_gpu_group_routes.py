"""The fusion groups (csrc/host/rowfuse_row.cpp, rowfuse_wide.cpp, rowfuse_sample.cpp, form_* of plan_groups.cpp) on the
cases of tests/group_cases.py, member by member and route by route.

Per case: the launch lines of the plan hold the case's words (which group, which ending, which kind every member took —
words that eg_model_launch_text prints from the planner's and the generators' own records); the output and every tensor
the plan stores are held to the oracle, its float64 shadow (tests/parity.py: Trio.check) and the numpy reference of the
table (TOL on the whole tensor); a second run gives the same bits; and a tensor that a group kept in registers or LDS is
either refused by read_tensor or equal to the reference — and equal to it after keep_values(True), with the output's bits
unchanged.

One child process that starts with EG_NO_ROWFUSE=1 runs the whole table without groups: the unfused side of
every comparison, through the same gates.  Same bits are asserted only where the code's own comments claim the same
operations in the same order: EG_NO_ROW_DIRECT against `direct` and the in-kernel fold against row_finalize on the same grid
(rowfuse_row.cpp), EG_SAMPLE_KEEP_BARRIERS / EG_SAMPLE_NO_STAGE / EG_NO_NARROW_INDEX against the default sample kernel
(synchronisation, where an operand is read from and index arithmetic only), keep_values against the default plan (stores only).
Row-local maps of inputs, fused against unfused, are printed and held to the gates: no comment claims their bits.

Models are module-scoped, one per (program, shapes, switches): a case's switches are set while its plan is made.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import TOL, debug_toggles_active      # (first: puts the repository root on sys.path, also in the child)
import group_cases as gc
from generated_cases import check_against_numpy, rel

pytestmark = pytest.mark.gpu
_TROUBLE = []           # a child or a device error: nothing more runs on the GPU from this module
NAMES = list(gc.BY_NAME)
CHILD_LIMIT = 300       # seconds, as tests/test_gpu_generated_routes.py
KEEP = ["CHAIN_ROWS_257x12", "CHAIN_ROWS_257x64", "CHAIN_WIDE_5x129", "CHAIN_WIDE_257x65", "CHAIN_WIDE_1x4096", "ROWS_3D_300",
        "ROWS_3D_INLINED", "ROWS_WIDE_TOTALS_257", "SAMPLE_F_2", "SAMPLE_F_5", "SAMPLE_F_64"]
T0 = time.time()


def plan_lines(model, target):
    return [ln for ln in model.launch_plan(target).splitlines() if ln.startswith("[")]


def set_params(model, ids, values):
    for name, v in values.items():
        model.params[ids[name]] = v


def read_or_refusal(model, target, tid):
    """The tensor, or the library's message where it refuses to hand the tensor out."""
    from exprgrad_amd._lib import GpuError
    try:
        return np.array(model.read_tensor(target, tid))
    except GpuError as e:
        return str(e)


def no_gpu_work_after_trouble():
    if _TROUBLE:
        pytest.fail("no further GPU work after: " + _TROUBLE[0])


def guarded(fn, *args):
    """fn(*args); an error of the device (not a refusal of the library) ends the module's GPU work."""
    from exprgrad_amd._lib import GpuError
    no_gpu_work_after_trouble()
    try:
        return fn(*args)
    except GpuError as e:
        if "hip" in str(e).lower() or "illegal" in str(e).lower():
            _TROUBLE.append(str(e)[:500])
        raise


def run_case(model, case, ids):
    """call twice, the launch lines, every tensor of the reference by name (an array, or the refusal's text)."""
    inputs = case.inputs()
    set_params(model, ids, case.params())
    first = np.array(model.call(case.target, inputs))
    reads = {name: read_or_refusal(model, case.target, ids[name]) for name in case.want() if name != "out"}
    again = np.array(model.call(case.target, inputs))
    return {"out": first, "again": again, "plan": plan_lines(model, case.target), "reads": reads}


# ---- the child: the whole table without fusion groups ----------------------------------------------------------------------------------
def child_main(path):
    import exprgrad_amd as eg
    from exprgrad_amd import model as egm
    ctx = eg.newGpuContext()
    arrays, plans, models = {}, {}, {}
    for case in gc.CASES:
        if case.env:
            continue        # (the switches of a case only choose among groups)
        if case.program not in models:
            models[case.program] = (egm.compile(*gc.PROGRAMS[case.program](), gpu=ctx), gc.tensor_ids(case.program))
        m, ids = models[case.program]
        got = run_case(m, case, ids)
        arrays[case.name] = got["out"]
        for name, v in got["reads"].items():
            if not isinstance(v, str):
                arrays[case.name + "__" + name] = v
        plans[case.name] = got["plan"]
    ctx.sync()
    np.savez(path, __plans=np.array(json.dumps(plans)), **arrays)
    print("table ok")


_CHILD = {}


def child(tmp_path_factory):
    if "unfused" in _CHILD:
        return _CHILD["unfused"]
    no_gpu_work_after_trouble()
    path = str(tmp_path_factory.mktemp("groups") / "unfused.npz")
    started = time.time()
    try:
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "child", path], env=dict(os.environ, EG_NO_ROWFUSE="1"),
                              capture_output=True, text=True, timeout=CHILD_LIMIT)
    except subprocess.TimeoutExpired:
        _TROUBLE.append("the unfused child did not finish within %d s" % CHILD_LIMIT)
        pytest.fail(_TROUBLE[0])
    if done.returncode != 0 or "table ok" not in done.stdout:
        _TROUBLE.append("the unfused child ended with %d\n%s\n%s" % (done.returncode, done.stdout[-3000:], done.stderr[-3000:]))
        pytest.fail(_TROUBLE[0])
    print("the unfused child took %.1f s" % (time.time() - started))
    with np.load(path) as z:
        _CHILD["unfused"] = ({k: z[k] for k in z.files if k != "__plans"}, json.loads(str(z["__plans"])))
    return _CHILD["unfused"]


# ---- references: computed once per (program, shapes), shared by every test ----------------------------------------------------------------
_ORACLES, _REFS = {}, {}


def references(case):
    """name -> (oracle, shadow, numpy) for the output and every tensor of the case's reference."""
    from oracle import kd
    key = (case.program, tuple(sorted(case.shapes.items())))
    if key not in _REFS:
        if case.program not in _ORACLES:
            text = gc.program_text(case.program)
            _ORACLES[case.program] = (kd.Model(text, threads=4), kd.Model(text, shadow=True), gc.tensor_ids(case.program))
        ref, exact, ids = _ORACLES[case.program]
        for m in (ref, exact):
            for name, v in case.params().items():
                m.params[ids[name]][...] = v
        inputs, want = case.inputs(), case.want()
        r32, r64 = np.array(ref.call(case.target, inputs)), np.array(exact.call(case.target, inputs))
        _REFS[key] = {name: (r32 if name == "out" else np.array(ref.last[ids[name]]), r64 if name == "out" else np.array(exact.last[ids[name]]), w)
                      for name, w in want.items()}
    return _REFS[key]


def check_values(case, name, got, what):
    from parity import Trio
    ref, exact, want = references(case)[name]
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    print("%s: %.3g from the shadow, %.3g from the oracle, %.3g from numpy" % (what, rel(got, exact), rel(got, ref), rel(got, want)))
    Trio.check(got, ref, exact, case.rtotal, "%s %s" % (case.program, name))
    check_against_numpy(case, got, want, TOL)


def check_lines(case, plan):
    """The i-th launch of a kind holds the words of the table's i-th entry of that kind; no launch of an absent kind."""
    for kind in {k for k, _ in case.lines}:
        have = [ln for ln in plan if "] " + kind in ln]
        claims = [words for k, words in case.lines if k == kind]
        assert len(have) == len(claims), (case.name, kind, plan)
        for ln, words in zip(have, claims):
            for w in words:
                assert w in ln, (case.name, "expected", w, "in", ln)
    for kind in case.absent:       # (a kind of launch at the head of its line, any other word anywhere)
        assert not any(("] " + kind if kind.endswith("-fused") else kind) in ln for ln in plan), (case.name, "no launch may be", kind, plan)


# ---- the fused runs, in this process ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fused_models(gpu_ctx):
    from exprgrad_amd import model as egm
    made = {}

    def get(case):
        if case.model_key not in made:
            made[case.model_key] = (egm.compile(*gc.PROGRAMS[case.program](), gpu=gpu_ctx), gc.tensor_ids(case.program))
        return made[case.model_key]
    yield get
    for m, _ in made.values():
        m.close()
    print("the module took %.1f s" % (time.time() - T0))


_RUNS = {}


def fused(case, fused_models, monkeypatch):
    """The case on its model, run once: as planned and — for the cases of KEEP — under keep_values(True)."""
    if case.name not in _RUNS:
        toggles = debug_toggles_active()            # (before the case's own switches)
        for k, v in case.env.items():
            monkeypatch.setenv(k, v)
        m, ids = guarded(fused_models, case)
        got = guarded(run_case, m, case, ids)
        got["toggles"] = toggles
        if case.name in KEEP:
            m.keep_values(True)
            got["kept"] = guarded(run_case, m, case, ids)
            m.keep_values(False)
        _RUNS[case.name] = got
    return _RUNS[case.name]


@pytest.mark.parametrize("name", NAMES)
def test_route_values_and_a_second_run(name, fused_models, monkeypatch):
    case = gc.BY_NAME[name]
    got = fused(case, fused_models, monkeypatch)
    print("\n".join(got["plan"]))
    if not got["toggles"]:
        check_lines(case, got["plan"])
    check_values(case, "out", got["out"], name)
    assert gc.same_bits(got["out"], got["again"]), (name, "two runs differ")
    for tensor, v in got["reads"].items():
        if isinstance(v, str):       # refused: with a message, and only what the table says a group keeps to itself
            assert "keep_values" in v or "not materialised" in v, (name, tensor, v)
            assert got["toggles"] or tensor in case.kept + case.inlined, (name, tensor, "was refused:", v)
        else:
            assert got["toggles"] or tensor not in case.kept + case.inlined, (name, tensor, "lives in a group's registers or LDS by the table, and was read")
            check_values(case, tensor, v, "%s %s" % (name, tensor))
    for tensor in case.stored:
        assert not isinstance(got["reads"][tensor], str), (name, tensor, got["reads"][tensor])


@pytest.mark.parametrize("name", KEEP)
def test_keep_values_stores_what_a_group_kept_to_itself(name, fused_models, monkeypatch):
    """After keep_values(True) every tensor of the reference is read and equals it; the output keeps its bits (the plan
    differs by stores only)."""
    case = gc.BY_NAME[name]
    got = fused(case, fused_models, monkeypatch)
    kept = got["kept"]
    print("\n".join(kept["plan"]))
    assert case.kept
    for tensor in case.kept:
        if not got["toggles"]:
            assert isinstance(got["reads"][tensor], str), (name, tensor, "was read from a plan that does not store it")
    for tensor, v in kept["reads"].items():
        if tensor in case.inlined:      # inlined when the model was compiled: no plan has it, and the library says so
            assert isinstance(v, str) and "not materialised" in v, (name, tensor, v)
            continue
        assert not isinstance(v, str), (name, tensor, v)
        check_values(case, tensor, v, "%s %s (values kept)" % (name, tensor))
    check_values(case, "out", kept["out"], name + " (values kept)")
    assert gc.same_bits(kept["out"], got["out"]), (name, "keep_values changed the output's bits")


@pytest.mark.parametrize("name", [n for n in NAMES if not gc.BY_NAME[n].env])
def test_unfused_values(name, tmp_path_factory, fused_models, monkeypatch):
    """EG_NO_ROWFUSE=1: no group in the plan; the same gates; row-local maps of inputs are printed against the fused run."""
    case = gc.BY_NAME[name]
    arrays, plans = child(tmp_path_factory)
    assert not any("fused" in ln and "gemm" not in ln for ln in plans[name]), plans[name]
    check_values(case, "out", arrays[name], name + " (unfused)")
    for tensor in case.want():
        key = name + "__" + tensor
        if key in arrays:
            check_values(case, tensor, arrays[key], "%s %s (unfused)" % (name, tensor))
    got = fused(case, fused_models, monkeypatch)
    for tensor, v in got.get("kept", got)["reads"].items():
        if not isinstance(v, str) and name + "__" + tensor in arrays:
            print("%s %s: fused and unfused %s" % (name, tensor, "have the same bits" if gc.same_bits(v, arrays[name + "__" + tensor]) else
                                                   "differ by %.3g" % rel(v, arrays[name + "__" + tensor])))


# ---- switches that claim the same bits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plain,switched", [("CHAIN_ROWS_255x12", "CHAIN_ROWS_255x12_NODIRECT"), ("CHAIN_ROWS_1000x12", "CHAIN_ROWS_1000x12_NOTAIL")])
def test_row_endings_give_the_same_bits(plain, switched, fused_models, monkeypatch):
    """direct against partial row + row_finalize of one block; the in-kernel fold against row_finalize on the same grid."""
    a = fused(gc.BY_NAME[plain], fused_models, monkeypatch)
    b = fused(gc.BY_NAME[switched], fused_models, monkeypatch)
    assert gc.same_bits(a["out"], b["out"]), (plain, switched, rel(a["out"], b["out"]))
    for tensor in ("cs", "rs", "rq", "rm"):
        assert gc.same_bits(a["reads"][tensor], b["reads"][tensor]), (plain, switched, tensor)


@pytest.mark.parametrize("switch", ["EG_SAMPLE_KEEP_BARRIERS", "EG_SAMPLE_NO_STAGE", "EG_NO_NARROW_INDEX"])
def test_sample_switches_give_the_same_bits(switch, gpu_ctx, fused_models, monkeypatch):
    from exprgrad_amd import model as egm
    case = gc.BY_NAME["SAMPLE_F_5"]
    base = fused(case, fused_models, monkeypatch)
    toggles = debug_toggles_active()
    monkeypatch.setenv(switch, "1")
    m = egm.compile(*gc.PROGRAMS[case.program](), gpu=gpu_ctx)
    got = guarded(run_case, m, case, gc.tensor_ids(case.program))
    m.close()
    print("\n".join(got["plan"]))
    line = [ln for ln in got["plan"] if "sample-fused" in ln]
    if not toggles:
        assert len(line) == 1
        if switch == "EG_SAMPLE_KEEP_BARRIERS":
            assert "barriers=9/9" in line[0] and "barriers=9/9" not in [ln for ln in base["plan"] if "sample-fused" in ln][0], line[0]
        if switch == "EG_SAMPLE_NO_STAGE":
            assert "staged=0" in line[0]
        if switch == "EG_NO_NARROW_INDEX":
            assert " wide " in line[0] and " narrow " not in line[0]
    check_values(case, "out", got["out"], "SAMPLE_F_5 with " + switch)
    assert gc.same_bits(got["out"], base["out"]), (switch, rel(got["out"], base["out"]))


# ---- training steps through Trio.step ----------------------------------------------------------------------------------------------------
def trio_of(gpu_ctx, program, seed):
    from parity import Trio
    t = Trio(gpu_ctx, gc.PROGRAMS[program], threads=4)
    t.init_params(np.random.default_rng(seed))
    return t


@pytest.mark.parametrize("name,batch,words", gc.TAIL_CASES)
def test_row_tail_steps(name, batch, words, gpu_ctx):
    """A 2-wide regression step whose row group's last block goes on with the update: 64 blocks, the sample loop with a
    literal trip count at 32768 rows and the generic strided loop at 256 rows more.  Three steps from identical state."""
    toggles = debug_toggles_active()
    t = trio_of(gpu_ctx, "tail", batch)
    rng = np.random.default_rng(batch)
    data = {"x": gc.uniform(rng, batch, 2), "t": gc.uniform(rng, batch, 2)}
    for _ in range(3):
        guarded(t.step, "train", data, batch)
    plan = plan_lines(t.gpu, "train")
    print("\n".join(plan))
    if not toggles:
        line = [ln for ln in plan if "] row-fused" in ln]
        assert len(line) == 1, plan
        for w in words:
            assert w in line[0], (name, w, line[0])
        assert ("unrolled" in line[0]) == any("unrolled" in w for w in words), line[0]
        assert "which goes on with launch" in line[0], line[0]
    t.close()


@pytest.mark.parametrize("batch", gc.SAMPLE_T_BATCHES)
def test_sample_training_steps(batch, gpu_ctx, monkeypatch):
    """dense, leakyRelu, dense with a weight two statements use, mse, gradientDescent: three steps from identical state, the
    gradients of the first also against the gradient written by hand (group_cases.ref_sample_training)."""
    toggles = debug_toggles_active()
    monkeypatch.delenv("EG_NO_SAMPLE_FUSE", raising=False)
    t = trio_of(gpu_ctx, "sample_t", batch)
    ids = gc.tensor_ids("sample_t")
    rng = np.random.default_rng(1000 + batch)
    data = {"x": gc.uniform(rng, batch, gc.ST["I"]), "t": gc.uniform(rng, batch, gc.ST["O"])}
    params = {n: np.array(t.gpu.params[ids[n]]) for n in ("w1", "b1", "w2")}
    want = gc.ref_sample_training(data, params)
    t.call("predict", {"x": data["x"]}, n=gc.ST["I"])
    for step in range(3):
        guarded(t.step, "train", data, batch)
        if step == 0:
            pairs = dict(t.ref.param_grads("train"))
            for n in ("w1", "b1", "w2"):
                g = np.array(t.gpu.read_tensor("train", pairs[ids[n]]))
                print("batch %d gradient of %s: %.3g from the hand-written gradient" % (batch, n, rel(g, want[n])))
                assert g.shape == want[n].shape and rel(g, want[n]) <= TOL, (batch, n, rel(g, want[n]))
    plan = plan_lines(t.gpu, "train")
    print("\n".join(plan))
    if not toggles:
        line = [ln for ln in plan if "sample-fused" in ln]
        if batch > gc.SAMPLE_MAX_BATCH:
            assert not line, plan
        else:
            assert len(line) == 1 and "(%d blocks)" % batch in line[0], plan
            # four contributions to three gradients: the second one to the shared weight's adds to the block's slab row
            entries = [e.split() for e in line[0].rsplit(" | ", 1)[1].split("; ")]
            assert sum("slab+" in e for e in entries) == 1 and sum("slab" in e for e in entries) == 3, line[0]
            assert "split T=16 ragged=6" in line[0], line[0]
    t.close()


def test_apply_against_backward_then_update(gpu_ctx, monkeypatch):
    """Model.apply (the optimizer's map group adds the slab rows up itself) against run_backward + run_update (one slab pass
    between them), from identical state: two orders of the same 32 terms, held to TOL."""
    from exprgrad_amd import model as egm
    from oracle import kd
    toggles = debug_toggles_active()
    monkeypatch.delenv("EG_NO_SAMPLE_FUSE", raising=False)
    batch = 32
    rng = np.random.default_rng(7)
    data = {"x": gc.uniform(rng, batch, gc.ST["I"]), "t": gc.uniform(rng, batch, gc.ST["O"])}
    whole, split = (egm.compile(*gc.PROGRAMS["sample_t"](), gpu=gpu_ctx) for _ in range(2))
    for tid in whole.params.ids():
        whole.params[tid] = split.params[tid] = gc.uniform(rng, *whole.params[tid].shape)
    pairs = kd.Model(gc.program_text("sample_t")).param_grads("train")
    for step in range(3):
        guarded(whole.apply, "train", data)
        guarded(split.run_backward, "train", data)
        grads = {g: np.array(split.read_tensor("train", g)) for _, g in pairs}
        split.run_update("train")
        for p, g in pairs:
            gw = np.array(whole.read_tensor("train", g))
            assert np.all(np.isfinite(gw)) and rel(gw, grads[g]) <= TOL, (step, g, rel(gw, grads[g]))
            assert rel(whole.params[p], split.params[p]) <= TOL, (step, p)
            split.params[p] = whole.params[p]
    if not toggles:
        assert any("sample-fused" in ln and "folded by launch" in ln for ln in plan_lines(whole, "train")), plan_lines(whole, "train")
    whole.close()
    split.close()


if __name__ == "__main__" and sys.argv[1:2] == ["child"]:
    child_main(sys.argv[2])
