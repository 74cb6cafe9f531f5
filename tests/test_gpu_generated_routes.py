"""The generated kernels (csrc/host/codegen.cpp) on the cases of tests/generated_cases.py, every emitter route.

Three runs of the whole table, each held to the same references (the oracle, its float64 shadow and a plain numpy
restatement; tests/test_generated_cases_cpu.py holds those three to each other):

    plain     EG_NO_ROWFUSE=1 EG_NO_INLINE=1: the launch list without fusion groups, so every kernel goes through
              generate_mode_a / generate_mode_b.  The launch line of every case must hold the route words of the table (map /
              split-reduce, scatter / reduce, vec4, narrow / wide, tx=) and, for the split reductions, chunks= must make the case
              as ragged as the table says.  Each split reduction runs twice: same bits.
    wide      the same with EG_NO_NARROW_INDEX=1: every line says wide, and the results have the same bits as the plain run —
              only integer index arithmetic differs between the two bodies.
    default   in this process, through whatever groups the planner forms (the small and map groups of rowfuse_small.cpp emit
              many of these kernels with code of their own); the plan is printed, not asserted.

The first two runs are one fresh child process each, started with its switches set (subprocess of
sys.executable, one at a time, under a time limit); a child that fails in any way fails its tests and no other child is
started.  Gates: tests/parity.py (Trio.check: 1e-5 of the exact value, the direct gate against the oracle), the bound of
tests/test_gpu_f64.py for compile[float64], and generated_cases.check_against_numpy on the WHOLE result tensor — exact cases
value for value, what a bounded loop leaves alone must be zero.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import TOL, debug_toggles_active      # (first: puts the repository root on sys.path, also in the child)
import generated_cases as gc

pytestmark = pytest.mark.gpu
NAMES = list(gc.BY_NAME)
SPLIT = [c.name for c in gc.CASES if c.mode_b]
CHILD_LIMIT = 300       # seconds: eight hiprtc programs, some twenty split-reduction kernels, a hundred small launches


def plan_lines(model, target):
    return [ln for ln in model.launch_plan(target).splitlines() if ln.startswith("[")]


def run_table(ctx):
    """Every case on models of this process: {name: (result, second result of a split reduction or None, launch lines)}."""
    from exprgrad_amd import model as egm
    models, out = {}, {}
    for case in gc.CASES:
        key = (case.program, case.f64)
        if key not in models:
            models[key] = egm.compile(*gc.PROGRAMS[case.program](), gpu=ctx, dtype=case.dtype)
        m, inputs = models[key], case.inputs()
        first = np.array(m.call(case.target, inputs))
        again = np.array(m.call(case.target, inputs)) if case.mode_b else None
        out[case.name] = (first, again, plan_lines(m, case.target))
    for m in models.values():
        m.close()
    return out


def child_main(path):
    import exprgrad_amd as eg
    ctx = eg.newGpuContext()
    arrays, plans = {}, {}
    for name, (first, again, plan) in run_table(ctx).items():
        arrays[name] = first
        if again is not None:
            arrays[name + "__again"] = again
        plans[name] = plan
    ctx.sync()
    np.savez(path, __plans=np.array(json.dumps(plans)), **arrays)
    print("table ok")


# ---- the child runs ----------------------------------------------------------------------------------------------------------------
_CHILDREN = {}
_TROUBLE = []
CHILD_ENV = {"plain": {"EG_NO_ROWFUSE": "1", "EG_NO_INLINE": "1"},
             "wide": {"EG_NO_ROWFUSE": "1", "EG_NO_INLINE": "1", "EG_NO_NARROW_INDEX": "1"}}


def child(mode, tmp_path_factory):
    if mode in _CHILDREN:
        return _CHILDREN[mode]
    if _TROUBLE:
        pytest.fail("no further child process after: " + _TROUBLE[0])
    path = str(tmp_path_factory.mktemp("routes") / (mode + ".npz"))
    try:
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "child", path], env=dict(os.environ, **CHILD_ENV[mode]),
                              capture_output=True, text=True, timeout=CHILD_LIMIT)
    except subprocess.TimeoutExpired:
        _TROUBLE.append("the %s child did not finish within %d s" % (mode, CHILD_LIMIT))
        pytest.fail(_TROUBLE[0])
    if done.returncode != 0 or "table ok" not in done.stdout:
        _TROUBLE.append("the %s child ended with %d\n%s\n%s" % (mode, done.returncode, done.stdout[-3000:], done.stderr[-3000:]))
        pytest.fail(_TROUBLE[0])
    with np.load(path) as z:
        plans = json.loads(str(z["__plans"]))
        _CHILDREN[mode] = {name: (z[name], z[name + "__again"] if name + "__again" in z.files else None, plans[name]) for name in NAMES}
    return _CHILDREN[mode]


# ---- references: computed once per case, shared by every test --------------------------------------------------------------------
_ORACLES, _REFS = {}, {}


def references(case):
    """(oracle, float64 shadow or None for a float64 case, numpy)."""
    from oracle import kd
    if case.name not in _REFS:
        key = (case.program, case.f64)
        if key not in _ORACLES:
            text = gc.program_text(case.program, case.f64)
            _ORACLES[key] = (kd.Model(text, threads=4), None if case.f64 else kd.Model(text, shadow=True))
        ref, exact = _ORACLES[key]
        inputs = case.inputs()
        _REFS[case.name] = (np.array(ref.call(case.target, inputs)), None if exact is None else np.array(exact.call(case.target, inputs)),
                            case.want())
    return _REFS[case.name]


def check_values(case, got, what):
    from parity import Trio
    ref, exact, want = references(case)
    assert got.dtype == case.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
    if case.f64:
        e_ref, e_np = gc.rel(got, ref), gc.rel(got, want)
        print("%s: %.3g from the oracle's float64 form, %.3g from numpy (limit %.0e)" % (what, e_ref, e_np, gc.TOL64))
        assert e_ref <= gc.TOL64 and e_np <= gc.TOL64, (what, e_ref, e_np)
    else:
        print("%s: %.3g from the shadow, %.3g from the oracle, %.3g from numpy" % (what, gc.rel(got, exact), gc.rel(got, ref), gc.rel(got, want)))
        Trio.check(got, ref, exact, case.rtotal or 1, "%s output" % case.target)
    gc.check_against_numpy(case, got, want, gc.TOL64 if case.f64 else TOL)
    if case.exact:
        assert np.array_equal(got, ref), (what, "differs from the oracle")


ROUTE_WORDS = ("scatter", "reduce", "vec4", "narrow", "wide")


def check_route(case, plan, words):
    """Every launch of the target is a generated one; its route words are exactly those of `words`, and the other entries of
    `words` (the kind of launch, tx=) are in the line."""
    assert plan and all("generated(" in ln for ln in plan), plan
    for ln in plan:
        m = re.search(r" \|((?: (?:%s))+)" % "|".join(ROUTE_WORDS), ln)
        assert set(m.group(1).split() if m else ()) == {w for w in words if w in ROUTE_WORDS}, (case.name, words, ln)
        for w in words:
            assert w in ROUTE_WORDS or w in ln + " ", (case.name, "expected", w, ln)


def chunking(case, line):
    """(chunks, full chunk, last chunk, ty) of a split reduction, from the launch line."""
    chunks = int(re.search(r"chunks=(\d+)", line).group(1))
    chunk = -(-case.rtotal // chunks)
    return chunks, chunk, case.rtotal - (chunks - 1) * chunk, 256 // case.tx


# ---- plain launch list ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fusion_off_route_and_values(name, tmp_path_factory):
    case = gc.BY_NAME[name]
    got, again, plan = child("plain", tmp_path_factory)[name]
    print("\n".join(plan))
    if not debug_toggles_active():
        check_route(case, plan, case.route)
        if case.mode_b:
            for ln in plan:
                chunks, chunk, last, ty = chunking(case, ln)
                print("%s: %d chunks of %d, the last %d; ty = %d" % (name, chunks, chunk, last, ty))
                assert (chunks - 1) * chunk < case.rtotal <= chunks * chunk
                if case.ragged:
                    assert chunks > 1 and last < chunk and last % ty != 0, (name, chunks, chunk, last, ty)
                if case.ragged == "all":
                    assert chunk % ty != 0, (name, chunks, chunk, ty)
    check_values(case, got, name + " (fusion off)")
    if again is not None:
        assert gc.same_bits(got, again), (name, "two runs of a split reduction differ")


@pytest.mark.parametrize("name", NAMES)
def test_wide_body_gives_the_same_bits(name, tmp_path_factory):
    case = gc.BY_NAME[name]
    narrow, _, _ = child("plain", tmp_path_factory)[name]
    wide, _, plan = child("wide", tmp_path_factory)[name]
    if not debug_toggles_active():
        check_route(case, plan, [w if w != "narrow" else "wide" for w in case.route])
    assert gc.same_bits(narrow, wide), (name, "the 32-bit and the 64-bit body differ", gc.rel(narrow, wide))
    check_values(case, wide, name + " (64-bit body)")


# ---- default settings, in this process -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def default_models(gpu_ctx):
    """program -> Trio (float32) or the backend's model alone (float64), compiled on first use."""
    from exprgrad_amd import model as egm
    from parity import Trio
    made = {}

    def get(case):
        key = (case.program, case.f64)
        if key not in made:
            made[key] = (egm.compile(*gc.PROGRAMS[case.program](), gpu=gpu_ctx, dtype=np.float64) if case.f64
                         else Trio(gpu_ctx, gc.PROGRAMS[case.program], threads=4))
        return made[key]
    yield get
    for m in made.values():
        m.close()


@pytest.mark.parametrize("name", NAMES)
def test_default_settings_values(default_models, name):
    case = gc.BY_NAME[name]
    m, inputs = default_models(case), case.inputs()
    if case.f64:
        got = np.array(m.call(case.target, inputs))
        gpu = m
    else:
        got = np.array(m.call(case.target, inputs, n=case.rtotal or 1))       # Trio.call: the project's gates
        gpu = m.gpu
    print("\n".join(plan_lines(gpu, case.target)))
    check_values(case, got, name + " (default settings)")
    if case.mode_b:
        assert gc.same_bits(got, np.array(gpu.call(case.target, inputs))), (name, "two runs differ")


if __name__ == "__main__" and sys.argv[1:2] == ["child"]:
    child_main(sys.argv[2])
