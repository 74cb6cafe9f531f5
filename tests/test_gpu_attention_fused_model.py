"""The forward attention chain as a model route (csrc/host/match_attention.cpp, plan_attention.cpp): the `out` target of the
five-statement program (tests/attention_fused_programs.py) runs as ONE `eg_attn` launch — eg_attention's kernel — and the
scores, the scaled scores, the row sums and the softmax get no storage.

Every case runs three ways (tests/parity.py: backend | oracle | float64 shadow) under that module's own gates, no tolerance of
their own and no allow-list entry; tests/test_attention_fused_oracle_cpu.py holds the oracle itself to 5e-6 on the same
shapes.  The 4100 keys wide case is compared with float64 numpy only: the oracle's serial sum of 4100 terms has not been
held to that.  Statements about the plan hold in the default configuration only (conftest.debug_toggles_active)."""
import numpy as np
import pytest

import attention_fused_programs as fp
import attention_programs as ap
import refcases
from conftest import TOL, debug_toggles_active, rel_err
from exprgrad_amd import model as egm
from exprgrad_amd._lib import GpuError
from parity import Trio

pytestmark = pytest.mark.gpu
f32 = np.float32


def u(rng, *shape):
    return (rng.random(shape, dtype=f32) - f32(0.5)).astype(f32)


def launches(model, target="out"):
    return [line for line in model.launch_plan(target).splitlines() if line.startswith("[")]


def inputs(rng, B, H, I, J, K, D):
    return {"q": u(rng, B, I, H, K), "kk": u(rng, B, J, H, K), "v": u(rng, B, J, H, D)}


def exact(x, scale):
    q, kk, v = (x[n].astype(np.float64) for n in ("q", "kk", "v"))
    e = np.exp(np.einsum("bihk,bjhk->bhij", q, kk) * np.float64(f32(scale)))
    return np.einsum("bhij,bjhd->bihd", e / e.sum(-1, keepdims=True), v)


def assert_fused(model, dims, scale="0.125", names="scores, scaled, softmax.sums, softmax, context"):
    B, H, I, J, K, D = dims
    lines = launches(model)
    assert len(lines) == 1, lines
    assert f"eg_attn {B}x{H} x {I}x{J}x{K}x{D} scale={scale} ({names})" in lines[0], lines
    assert not any(w in line for line in lines for w in ("eg_bgemm2", "eg_wrows", "generated")), lines
    assert "eg_attn" in model.emit_ir()


def assert_unfused(model, target="out"):
    plan = model.launch_plan(target)
    assert "eg_attn" not in plan, plan


def tensor_id(graphs, name):
    for line in refcases.program_text(graphs()).splitlines():
        w = line.split()
        if w[:1] == ["tensor"] and w[3] == name:
            return int(w[1])
    raise KeyError(name)


# ---- 1. the chain fuses ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(2, 3, 33, 70, 16, 16), (1, 2, 65, 64, 20, 12), (1, 2, 65, 64, 40, 72)], ids=lambda d: "x".join(map(str, d)))
def test_forward_is_one_launch(gpu_ctx, dims):
    """Fails without the feature: the plan is three launches."""
    trio = Trio(gpu_ctx, fp.attention_forward())
    got = trio.call("out", inputs(np.random.default_rng(sum(dims)), *dims), n=dims[3])
    assert got.shape == (dims[0], dims[2], dims[1], dims[5])
    if not debug_toggles_active():
        assert_fused(trio.gpu, dims)
    trio.close()


def test_forward_over_4100_keys(gpu_ctx):
    """wider than a wide row group takes (4096): one launch all the same; against float64 only"""
    dims = (1, 1, 5, 4100, 8, 8)
    x = inputs(np.random.default_rng(4100), *dims)
    m = egm.compile(*fp.attention_forward()(), gpu=gpu_ctx)
    got = m.call("out", x)
    err = rel_err(got, exact(x, fp.SCALE), "attention forward over 4100 keys vs float64")
    print("4100 keys vs float64", err)
    assert err <= TOL
    if not debug_toggles_active():
        assert_fused(m, dims)
    m.close()


@pytest.mark.parametrize("graphs,scale,names", [(fp.attention_forward_unscaled, "1", "scores, softmax.sums, softmax, context"),
                                                (fp.attention_forward_scale_first, "0.125", "scores, scaled, softmax.sums, softmax, context")],
                         ids=["unscaled", "scale_first"])
def test_the_other_spellings_of_the_scale_fuse(gpu_ctx, graphs, scale, names):
    dims = (2, 3, 33, 70, 16, 16)
    trio = Trio(gpu_ctx, graphs)
    trio.call("out", inputs(np.random.default_rng(8), *dims), n=70)
    if not debug_toggles_active():
        assert_fused(trio.gpu, dims, scale, names)
    trio.close()


def test_the_training_model(gpu_ctx):
    """`out` of the training program is one eg_attn launch; its `fit` plan keeps its eg_bgemm2 products and exactly two
    collapsed eg_wrows groups (tests/test_gpu_attention_rows.py::test_training_step pins the rest of it)"""
    B, H, I, J, K, D = ap.TRAINING_SHAPE
    rng = np.random.default_rng(2)
    trio = Trio(gpu_ctx, ap.attention_training(*ap.TRAINING_SHAPE))
    trio.init_params(rng, -0.5, 0.5)
    trio.call("out", {}, n=J)
    trio.step("fit", {"labels": u(rng, B, I, H, D)}, n=B * I * H * D)
    trio.call("out", {}, n=J)
    if not debug_toggles_active():
        assert_fused(trio.gpu, ap.TRAINING_SHAPE)
        fit = launches(trio.gpu, "fit")
        assert not any("eg_attn" in l for l in fit), fit
        assert sum("eg_bgemm2" in l for l in fit) >= 5, fit
        assert len([l for l in fit if "eg_wrows" in l and "rows=" in l]) == 2, fit
    trio.close()


# ---- 2. what keeps the unfused plan ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fp.NEAR_MISSES))
def test_near_misses_run_unfused(gpu_ctx, name):
    graphs, shapes, width = fp.NEAR_MISSES[name]
    rng = np.random.default_rng(len(name))
    trio = Trio(gpu_ctx, graphs)
    trio.call("out", {k: u(rng, *shape) for k, shape in sorted(shapes.items())}, n=width)
    assert_unfused(trio.gpu)
    trio.close()


def test_a_head_dimension_of_129_keeps_the_unfused_plan(gpu_ctx):
    dims = (1, 2, 9, 70, 129, 16)
    trio = Trio(gpu_ctx, fp.attention_forward())
    trio.call("out", inputs(np.random.default_rng(129), *dims), n=129)
    assert_unfused(trio.gpu)
    if not debug_toggles_active():
        assert sum("eg_bgemm2" in l for l in launches(trio.gpu)) == 2, launches(trio.gpu)
    trio.close()


def test_a_float64_model_is_not_fused(gpu_ctx):
    dims = (2, 3, 33, 70, 16, 16)
    x = {k: v.astype(np.float64) for k, v in inputs(np.random.default_rng(64), *dims).items()}
    m = egm.compile(*fp.attention_forward()(), gpu=gpu_ctx, dtype=np.float64)
    got = m.call("out", x)
    assert rel_err(got, exact(x, fp.SCALE), "float64 attention forward") <= 1e-12
    assert_unfused(m)
    assert "eg_attn" not in m.emit_ir()
    m.close()


@pytest.mark.parametrize("switch", ["EG_NO_ROWFUSE", "EG_NO_BATCHED_GEMM"])
def test_the_switches_of_its_parts_turn_it_off(gpu_ctx, monkeypatch, switch):
    dims = (2, 3, 33, 70, 16, 16)
    monkeypatch.setenv(switch, "1")
    trio = Trio(gpu_ctx, fp.attention_forward())
    trio.call("out", inputs(np.random.default_rng(5), *dims), n=70)
    assert_unfused(trio.gpu)
    trio.close()
    monkeypatch.delenv(switch)


# ---- 3. the intermediates ---------------------------------------------------------------------------------------------------
def test_the_softmax_is_not_stored_unless_values_are_kept(gpu_ctx):
    from oracle import kd
    dims = (2, 3, 33, 70, 16, 16)
    graphs = fp.attention_forward()
    x = inputs(np.random.default_rng(9), *dims)
    tid = tensor_id(graphs, "softmax")
    m = egm.compile(*graphs(), gpu=gpu_ctx)
    first = m.call("out", x)
    if not debug_toggles_active():
        assert_fused(m, dims)
        with pytest.raises(GpuError, match="eg_model_keep_values"):
            m.read_tensor("out", tid)
    m.keep_values(True)
    kept = m.call("out", x)
    assert_unfused(m)
    ref = kd.Model(refcases.program_text(graphs()), threads=4)
    ref.call("out", x)
    assert rel_err(m.read_tensor("out", tid), ref.last[tid], "softmax read back vs oracle") <= TOL
    assert rel_err(kept, first, "unfused vs fused") <= TOL
    m.keep_values(False)
    again = m.call("out", x)
    if not debug_toggles_active():
        assert_fused(m, dims)
    assert np.array_equal(again.view(np.uint32), first.view(np.uint32))
    m.close()


# ---- 4. replay ----------------------------------------------------------------------------------------------------------------
def test_four_calls_replay_the_captured_launch(gpu_ctx):
    """new inputs on every call (the sequence is captured on the second run and replayed afterwards): every result is right,
    and a twin model gives the same bits"""
    dims = (2, 3, 33, 70, 16, 16)
    graphs = fp.attention_forward()
    models = [egm.compile(*graphs(), gpu=gpu_ctx) for _ in range(2)]
    rng = np.random.default_rng(21)
    for step in range(4):
        x = inputs(rng, *dims)
        got = [np.array(m.call("out", x)) for m in models]
        assert rel_err(got[0], exact(x, fp.SCALE), "replayed attention forward, call %d" % step) <= TOL
        assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)), step
    if not debug_toggles_active():
        assert_fused(models[0], dims)
    for m in models:
        m.close()
