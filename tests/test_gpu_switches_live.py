"""Planning switches are read when a plan is made, not once per process (csrc/switches.hpp: reads are live).

One process, the conftest monkeypatch wrapper (setenv / delenv + eg_switches_reload), the MLP of tests/test_gpu_epilogue.py at
64 rows with EG_EPILOGUE_MIN_ELEMS=0.  Per switch - four that lowering and planning used to keep in a function-local static -
a model built with the switch set shows the effect in its launch plan, and a third model built after the switch is gone again
has the first model's plan.  Results: the same bits where the existing tests claim them (EG_NO_NARROW_INDEX:
tests/test_gpu_generated_routes.py; EG_NO_EPILOGUE: tests/test_gpu_epilogue.py, which holds the bias-gradient fold off in
both runs for it and keeps the contractions on the matrix tile - so does this test), the suite's TOL otherwise.  Plan
texts are compared only without the execution switches of tools/stress_suite.sh in the environment
(conftest.debug_toggles_active), numbers always.

EG_NO_INLINE: every elementwise kernel of this MLP rides on a contraction as its epilogue or sits in a fusion group, so
lowering finds nothing to inline and the MLP's launch list has 11 launches with the switch and without it (measured; the
parent commit's lowering gives the same 11).  The MLP case keeps its other claims (numbers within TOL, the third plan equal to
the first, a list that is no shorter), and the growth itself is asserted on the smallest model that has something to
inline: the activation chain in front of a pooling kernel of tests/test_pooling_reshape.py, one launch with inlining, more
without.
"""
import numpy as np
import pytest

from conftest import TOL, debug_toggles_active, rel_err
from exprgrad_amd import dsl, layers
from exprgrad_amd import model as egm
from test_gpu_epilogue import mlp

pytestmark = pytest.mark.gpu

BATCH = 64
FUSED = ("row-fused", "sample-fused", "small-fused", "map-fused")
SAME_BITS = ("EG_NO_NARROW_INDEX", "EG_NO_EPILOGUE")


def plan_lines(model, target):
    return [ln for ln in model.launch_plan(target).splitlines() if ln.startswith("[")]


def run(gpu_ctx):
    """A fresh model from fixed parameters: predict, one training step; (output, parameters after the step, plans)."""
    rng = np.random.default_rng(11)
    x = (rng.random((BATCH, 96), dtype=np.float32) - 0.5).astype(np.float32)
    y = rng.random((BATCH, 8), dtype=np.float32)
    m = egm.compile(*mlp(), gpu=gpu_ctx)
    for tid in sorted(m.params.ids()):
        m.params[tid] = (rng.random(m._param_shapes[tid], dtype=np.float32) * 0.6 - 0.3).astype(np.float32)
    out = np.array(m.call("predict", {"x": x}))
    m.apply("train", {"x": x, "y": y})
    params = {tid: np.array(m.params[tid]) for tid in sorted(m.params.ids())}
    plans = {t: plan_lines(m, t) for t in ("predict", "train")}
    m.close()
    return out, params, plans


@pytest.mark.parametrize("switch", ["EG_NO_EPILOGUE", "EG_NO_ROWFUSE", "EG_NO_NARROW_INDEX", "EG_NO_INLINE"])
def test_a_planning_switch_reaches_the_next_plan(switch, gpu_ctx, monkeypatch):
    toggles = debug_toggles_active()            # (before this test's own switches)
    monkeypatch.setenv("EG_EPILOGUE_MIN_ELEMS", "0")
    if switch == "EG_NO_EPILOGUE":
        # What tests/test_gpu_epilogue.py holds equal in both runs before it claims the same bits: the bias-gradient fold is
        # decided per plan (fused and unfused lists would sum the bias gradients in another order), and the plain contractions
        # must run on the matrix tile like the fused ones - at 64 rows they are small enough for the one-wave-per-element
        # kernel, whose sums run in another order (2.6e-7 of the output, measured), so that kernel is off in all three runs.
        monkeypatch.setenv("EG_NO_ONES_ROW", "1")
        monkeypatch.setenv("EG_NO_SMALL_GEMM", "1")
    base_out, base_params, base_plans = run(gpu_ctx)
    monkeypatch.setenv(switch, "1")
    out, params, plans = run(gpu_ctx)
    monkeypatch.delenv(switch)
    again_out, again_params, again_plans = run(gpu_ctx)
    for target in ("predict", "train"):
        print("\n".join(["-- %s, plain" % target] + base_plans[target] + ["-- %s, %s=1" % (target, switch)] + plans[target]))
    if not toggles:
        both = plans["predict"] + plans["train"]
        base_both = base_plans["predict"] + base_plans["train"]
        if switch == "EG_NO_EPILOGUE":
            assert any("gemm+epilogue" in ln for ln in base_both) and not any("gemm+epilogue" in ln for ln in both)
        if switch == "EG_NO_ROWFUSE":
            assert any(w in ln for ln in base_both for w in FUSED) and not any(w in ln for ln in both for w in FUSED)
        if switch == "EG_NO_NARROW_INDEX":
            generated = [ln for ln in both if "generated(" in ln or "sample-fused" in ln]
            assert generated and all(" wide" in ln + " " and " narrow" not in ln for ln in generated), generated
            assert any(" narrow" in ln for ln in base_both)
        if switch == "EG_NO_INLINE":
            assert len(plans["train"]) >= len(base_plans["train"])      # (nothing to inline here: the module's docstring)
        assert again_plans == base_plans
    for what, got, want in [("predict", out, base_out)] + [("parameter %d" % t, params[t], base_params[t]) for t in base_params]:
        if switch in SAME_BITS:
            assert np.array_equal(got, want), (switch, what, rel_err(got, want))
        else:
            assert rel_err(got, want) <= TOL, (switch, what)
    assert np.array_equal(again_out, base_out) and all(np.array_equal(again_params[t], base_params[t]) for t in base_params)


def test_no_inline_reaches_the_next_lowering(gpu_ctx, monkeypatch):
    """leakyRelu -> tanh -> maxpool2: both maps are recomputed inside the pooling kernel (lower.cpp inline_producers) unless
    EG_NO_INLINE says otherwise when the model is compiled; same operations per element either way."""
    toggles = debug_toggles_active()

    def run():
        m = egm.compile(layers.maxpool2(layers.tanh(layers.leaky_relu(dsl.input("img")))).target("out"), gpu=gpu_ctx)
        # (16 384 elements: too many for a one-block small group to take the three kernels whole)
        img = (np.random.default_rng(3).random((2, 32, 32, 8), dtype=np.float32) - 0.5).astype(np.float32)
        out, plan = np.array(m.call("out", {"img": img})), plan_lines(m, "out")
        m.close()
        return out, plan

    base_out, base_plan = run()
    monkeypatch.setenv("EG_NO_INLINE", "1")
    out, plan = run()
    monkeypatch.delenv("EG_NO_INLINE")
    again_out, again_plan = run()
    print("\n".join(["-- plain"] + base_plan + ["-- EG_NO_INLINE=1"] + plan))
    if not toggles:
        assert len(base_plan) == 1 and len(plan) > 1, (base_plan, plan)
        assert again_plan == base_plan
    assert rel_err(out, base_out) <= TOL and np.array_equal(again_out, base_out)
