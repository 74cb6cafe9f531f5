"""The forward attention chain of a compile[float64] model as ONE launch, under Model.fuse_attention_f64()
(eg_model_fuse_attention_f64, off by default): the forward programs of tests/attention_fused_programs.py and the attention
block of tests/attention_programs.py, compiled with dtype=np.float64, run beside oracle.kd.Model on the `f64` text of the
same program (the pair / compare_state pattern of tests/test_gpu_multihead_model_f64.py; bound: 1e-12 relative to the largest
element).  With the setting on, the launch list shows one `eg_attn` launch for the chain — eg_attention_f64's kernel — and no
generated kernel for its members, and the scores, the scaled scores, the sums and the softmax cannot be read.  With it off,
and with Model.batched2_f64() alone, a model shows the launches and the bits it showed before the call.  A `fit` target over
the block still trains on its generated and eg_bgemm2 kernels.  (Statements about the plan hold in the default configuration
only: under an `execution` switch such as EG_NO_BATCHED_GEMM=1 the numbers are checked alone.)"""
import numpy as np
import pytest

import attention_fused_programs as fp
import attention_programs as ap
from conftest import debug_toggles_active
from exprgrad_amd import model as egm
from exprgrad_amd._lib import GpuError
from test_gpu_attention_fused_model import tensor_id
from test_gpu_multihead_model_f64 import TOL64, compare_state, launches, rel, text64, training_steps

pytestmark = pytest.mark.gpu
DIMS = (2, 3, 33, 70, 16, 16)       # B, H, I, J, K, D
NAMES = "scores, scaled, softmax.sums, softmax, context"
bits = lambda x: np.ascontiguousarray(x, np.float64).view(np.uint64)


def inputs(rng, B, H, I, J, K, D):
    return {"q": rng.random((B, I, H, K)) - 0.5, "kk": rng.random((B, J, H, K)) - 0.5, "v": rng.random((B, J, H, D)) - 0.5}


def oracle(graphs):
    from oracle import kd
    ref = kd.Model(text64(graphs()))
    assert ref.c64
    return ref


def assert_fused(model, dims, scale="0.125", names=NAMES, target="out"):
    B, H, I, J, K, D = dims
    lines = launches(model, target)
    assert len(lines) == 1, lines
    assert f"eg_attn {B}x{H} x {I}x{J}x{K}x{D} scale={scale} ({names})" in lines[0], lines
    assert not any(w in line for line in lines for w in ("eg_bgemm2", "generated")), lines
    assert "eg_attn" in model.emit_ir()


def assert_two_products_around_generated_kernels(model, target="out"):
    lines = launches(model, target)
    assert "eg_attn" not in model.launch_plan(target) and sum("eg_bgemm2" in l for l in lines) == 2 and any("generated" in l for l in lines), lines


# ---- 1. the chain fuses -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [DIMS, (1, 2, 65, 64, 20, 12), (1, 2, 70, 130, 65, 72)], ids=lambda d: "x".join(map(str, d)))
def test_forward_is_one_launch(gpu_ctx, dims):
    """Fails without the feature.  (32, 32), and (128, 128) with its key tile of 32"""
    graphs = fp.attention_forward()
    x = inputs(np.random.default_rng(sum(dims)), *dims)
    m = egm.compile(*graphs(), gpu=gpu_ctx, dtype=np.float64)
    m.fuse_attention_f64()
    got = m.call("out", x)
    assert got.dtype == np.float64 and got.shape == (dims[0], dims[2], dims[1], dims[5])
    err = rel(got, oracle(graphs).call("out", x))
    print("fused float64 forward", dims, "vs oracle", err)
    assert err <= TOL64
    if not debug_toggles_active():
        assert_fused(m, dims)
    m.close()


@pytest.mark.parametrize("graphs,scale,names", [(fp.attention_forward_unscaled, "1", "scores, softmax.sums, softmax, context"),
                                                (fp.attention_forward_scale_first, "0.125", NAMES)], ids=["unscaled", "scale_first"])
def test_the_other_spellings_of_the_scale_fuse(gpu_ctx, graphs, scale, names):
    x = inputs(np.random.default_rng(8), *DIMS)
    m = egm.compile(*graphs(), gpu=gpu_ctx, dtype=np.float64)
    m.fuse_attention_f64()
    assert rel(m.call("out", x), oracle(graphs).call("out", x)) <= TOL64
    if not debug_toggles_active():
        assert_fused(m, DIMS, scale, names)
    m.close()


def test_the_hidden_tensors_cannot_be_read(gpu_ctx):
    graphs = fp.attention_forward()
    m = egm.compile(*graphs(), gpu=gpu_ctx, dtype=np.float64)
    m.fuse_attention_f64()
    m.call("out", inputs(np.random.default_rng(9), *DIMS))
    if not debug_toggles_active():
        assert_fused(m, DIMS)
        for name in ("scores", "scaled", "softmax.sums", "softmax"):
            with pytest.raises(GpuError, match="attention group"):
                m.read_tensor("out", tensor_id(graphs, name))
    m.close()


# ---- 2. off, and batched2_f64 alone, are the models they were ---------------------------------------------------------------
def test_off_and_batched2_alone_keep_their_launches_and_bits(gpu_ctx):
    """One model through: never set | batched2_f64 alone | both on | attention off again (batched2_f64 stays) | both off |
    the C setting alone (which forms no group).  The launch text and the output bits of a stage without fusion equal those
    captured on the same model before the call; the fused stage is within the bound of them."""
    graphs = fp.attention_forward()
    x = inputs(np.random.default_rng(10), *DIMS)
    m = egm.compile(*graphs(), gpu=gpu_ctx, dtype=np.float64)

    def stage():
        out = np.array(m.call("out", x))
        return m.launch_plan("out"), m.emit_ir(), out
    never = stage()
    assert "eg_attn" not in never[0] and "eg_attn" not in never[1] and "eg_bgemm" not in never[0]
    m.batched2_f64(True)
    plan_b, ir_b, out_b = stage()
    assert "eg_attn" not in ir_b
    if not debug_toggles_active():
        assert_two_products_around_generated_kernels(m)
    m.fuse_attention_f64(True)
    _, _, out_f = stage()
    if not debug_toggles_active():
        assert_fused(m, DIMS)
    assert rel(out_f, out_b) <= TOL64
    m.fuse_attention_f64(False)
    plan, ir, out = stage()
    assert (plan, ir) == (plan_b, ir_b) and np.array_equal(bits(out), bits(out_b))
    m.batched2_f64(False)
    plan, ir, out = stage()
    assert (plan, ir) == never[:2] and np.array_equal(bits(out), bits(never[2]))
    from exprgrad_amd._lib import call
    call("eg_model_fuse_attention_f64", m.handle, 1)        # the C setting alone: no two-index products, no group
    plan, ir, out = stage()
    assert plan == never[0] and "eg_attn" not in plan and np.array_equal(bits(out), bits(never[2]))
    m.close()


def test_a_float32_model_refuses_the_setting(gpu_ctx):
    m = egm.compile(*fp.attention_forward()(), gpu=gpu_ctx)
    with pytest.raises(Exception, match="float32"):
        m.fuse_attention_f64()
    m.close()


# ---- 3. what keeps the unfused plan -----------------------------------------------------------------------------------------
def test_a_head_dimension_of_129_keeps_the_unfused_plan(gpu_ctx):
    dims = (1, 2, 9, 70, 129, 16)
    graphs = fp.attention_forward()
    x = inputs(np.random.default_rng(129), *dims)
    m = egm.compile(*graphs(), gpu=gpu_ctx, dtype=np.float64)
    m.fuse_attention_f64()
    assert rel(m.call("out", x), oracle(graphs).call("out", x)) <= TOL64
    assert "eg_attn" not in m.launch_plan("out")
    if not debug_toggles_active():
        assert_two_products_around_generated_kernels(m)
    m.close()


@pytest.mark.parametrize("name", sorted(fp.NEAR_MISSES))
def test_near_misses_run_unfused(gpu_ctx, name):
    """a mask, bounded columns, a transposed operand, rank 3 or 5, a scale by a tensor or by division, ...: what the float32
    group refuses, this one refuses"""
    graphs, shapes, width = fp.NEAR_MISSES[name]
    rng = np.random.default_rng(len(name))
    x = {k: rng.random(shape) - 0.5 for k, shape in sorted(shapes.items())}
    m = egm.compile(*graphs(), gpu=gpu_ctx, dtype=np.float64)
    m.fuse_attention_f64()
    assert rel(m.call("out", x), oracle(graphs).call("out", x)) <= TOL64
    assert "eg_attn" not in m.launch_plan("out")
    m.close()


@pytest.mark.parametrize("how", ["keep_values", "EG_NO_BATCHED_GEMM", "EG_NO_ROWFUSE"])
def test_what_turns_the_float32_group_off_turns_this_one_off(gpu_ctx, monkeypatch, how):
    graphs = fp.attention_forward()
    x = inputs(np.random.default_rng(5), *DIMS)
    if how != "keep_values":
        monkeypatch.setenv(how, "1")
    m = egm.compile(*graphs(), gpu=gpu_ctx, dtype=np.float64)
    m.fuse_attention_f64()
    if how == "keep_values":
        m.keep_values(True)
    ref = oracle(graphs)
    assert rel(m.call("out", x), ref.call("out", x)) <= TOL64
    assert "eg_attn" not in m.launch_plan("out")
    tid = tensor_id(graphs, "softmax")
    assert rel(m.read_tensor("out", tid), ref.last[tid]) <= TOL64       # the softmax is stored again
    m.close()
    if how != "keep_values":
        monkeypatch.delenv(how)


# ---- 4. a training step over the block --------------------------------------------------------------------------------------
def test_a_fit_target_still_trains_on_its_own_kernels(gpu_ctx):
    """`out` of the training program is one eg_attn launch; `fit`, whose gradient kernels read the softmax, keeps generated and
    eg_bgemm2 kernels (the fit route is float32-only): state and gradients beside the oracle for two steps"""
    from oracle import kd
    dims = ap.TRAINING_SHAPE
    B, H, I, J, K, D = dims
    graphs = ap.attention_training(*dims)
    gpu = egm.compile(*graphs(), gpu=gpu_ctx, dtype=np.float64)
    gpu.fuse_attention_f64()
    ref = kd.Model(text64(graphs()))
    rng = np.random.default_rng(5)
    for tid in sorted(ref.params):
        v = rng.random(ref.params[tid].shape) - 0.5
        ref.params[tid][...] = v
        gpu.params[tid] = v
    assert rel(gpu.call("out", {}), ref.call("out", {})) <= TOL64
    training_steps(gpu, ref, {"labels": rng.random((B, I, H, D)) - 0.5}, steps=2)
    compare_state(gpu, ref, "after two steps")
    assert rel(gpu.call("out", {}), ref.call("out", {})) <= TOL64
    if not debug_toggles_active():
        assert_fused(gpu, dims)
        fit = launches(gpu, "fit")
        assert not any("eg_attn" in l for l in fit) and sum("eg_bgemm2" in l for l in fit) == 6, fit
        gpu.fuse_attention_fit()        # the float32 fit route: no group in a float64 model
        gpu.apply("fit", {"labels": rng.random((B, I, H, D)) - 0.5})
        assert not any("eg_attn" in l for l in launches(gpu, "fit")), launches(gpu, "fit")
    gpu.close()
