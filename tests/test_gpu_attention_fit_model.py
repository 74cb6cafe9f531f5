"""Training steps over the attention block on the fused kernels (Model.fuse_attention_fit; csrc/host/match_attention_grad.cpp,
csrc/host/plan_attention.cpp form_attention_fit_groups): with the setting on, the `fit` target of the training programs
(tests/attention_programs.py, tests/attention_fit_programs.py) runs the chain as one `eg_attn ... sums=` launch and its seven
or eight gradient kernels as one `eg_attn_grad` launch; scores, scaled scores, softmax and their gradients get no storage.
With it off (the default) nothing differs from a model that never heard of it.

Every step runs three ways (tests/parity.py: backend | oracle | float64 shadow) under that module's own gates and
conftest.TOL, with no tolerance of its own.  Statements about the plan hold in the default configuration only
(conftest.debug_toggles_active)."""
import numpy as np
import pytest

import attention_fit_programs as fit
import attention_programs as ap
import refcases
from conftest import TOL, debug_toggles_active, rel_err
from exprgrad_amd import model as egm
from exprgrad_amd._lib import GpuError
from parity import Trio

pytestmark = pytest.mark.gpu
f32 = np.float32

SHAPES = [(2, 3, 33, 70, 16, 16), (1, 2, 65, 64, 20, 12), (2, 1, 64, 64, 64, 64), (1, 1, 1, 1, 1, 1), (1, 2, 130, 129, 128, 128),
          (1, 2, 65, 64, 40, 72)]
PROJECTED = (2, 2, 70, 8, 16, 16)     # B, H, S, E, K, D
ident = lambda d: "x".join(map(str, d))


def u(rng, *shape):
    return (rng.random(shape, dtype=f32) - f32(0.5)).astype(f32)


def launches(model, target="fit"):
    return [line for line in model.launch_plan(target).splitlines() if line.startswith("[")]


def fused_lines(model, target="fit"):
    lines = launches(model, target)
    return [l for l in lines if "eg_attn " in l], [l for l in lines if "eg_attn_grad " in l]


def assert_fit_fused(model, dims, scale="0.125"):
    B, H, I, J, K, D = dims
    fwd, bwd = fused_lines(model)
    extents = f"{B}x{H} x {I}x{J}x{K}x{D} scale={scale} ("
    assert len(fwd) == 1 and "eg_attn " + extents in fwd[0] and " sums=softmax.sums" in fwd[0], launches(model)
    assert len(bwd) == 1 and "eg_attn_grad " + extents in bwd[0], launches(model)


def assert_fit_unfused(model):
    assert "eg_attn" not in model.launch_plan("fit"), model.launch_plan("fit")


def tensor_id(text, name):
    return fit._tensor_id(text, name)


def trained(trio, labels_shape, seed, steps=3, n=None, more=None):
    rng = np.random.default_rng(seed)
    trio.init_params(rng, -0.5, 0.5)
    for _ in range(steps):
        inputs = dict({"labels": u(rng, *labels_shape)}, **(more or {}))
        trio.step("fit", inputs, n=n or int(np.prod(labels_shape)))


# ---- 1. the step is right -------------------------------------------------------------------------------------------------------
def step_against_the_shadow(trio, inputs, zero):
    """Trio.step's two links with rel_err (conftest) against the float64 shadow alone, for the one case where dq and dk (the
    gradients of the parameters `zero`) are exactly zero — one key: the softmax is 1 whatever the scores are.  There the
    ORACLE's own float32 value of the cancelling difference is -2.2e-12 and the shadow's some 1e-18, and Trio's gates on the
    oracle (relative to max|exact|, floored at 1e-30) refuse the oracle, whatever the backend gives.  Those two gradients
    are held to the zero they are, which rel_err does in absolute terms: the backend has to be within TOL of 0."""
    trio.sync_from_gpu()
    trio.exact.run_backward("fit", inputs)
    trio.gpu.apply("fit", inputs)
    pairs = trio.ref.param_grads("fit")
    for ptid, gtid in pairs:
        got = trio.gpu.read_tensor("fit", gtid)
        want = trio.exact.last[gtid] if ptid not in zero else np.zeros(got.shape)      # (the shadow's own value there: some 1e-18)
        err = rel_err(got, want, "gradient of parameter %d vs float64" % ptid)
        print("gradient of parameter", ptid, "vs float64:", err)
        assert err <= TOL, (ptid, err)
        trio.exact.last[gtid][...] = got
    trio.exact.run_update("fit")
    for tid in sorted(trio.exact.params):
        err = rel_err(trio.gpu.params[tid], trio.exact.params[tid], "parameter %d after the step vs float64" % tid)
        assert err <= TOL, (tid, err)
    return {ptid: trio.gpu.read_tensor("fit", gtid) for ptid, gtid in pairs}


@pytest.mark.parametrize("dims", SHAPES, ids=ident)
def test_the_step_is_right(gpu_ctx, dims):
    """one call of `out` and three steps, every gradient and every updated parameter against oracle and float64 shadow from
    identical state; at (1,1,1,1,1,1) the softmax is 1, dq and dk are exactly zero and held so in absolute terms"""
    B, H, I, J, K, D = dims
    text = refcases.program_text(ap.attention_training(*dims)())
    trio = Trio(gpu_ctx, ap.attention_training(*dims))
    trio.gpu.fuse_attention_fit(True)
    rng = np.random.default_rng(sum(dims))
    trio.init_params(rng, -0.5, 0.5)
    trio.call("out", {}, n=J)
    for _ in range(3):
        inputs = {"labels": u(rng, B, I, H, D)}
        if I * J == 1:
            grads = step_against_the_shadow(trio, inputs, zero={tensor_id(text, "q"), tensor_id(text, "kk")})
            assert not grads[tensor_id(text, "q")].any() and not grads[tensor_id(text, "kk")].any(), grads
        else:
            trio.step("fit", inputs, n=B * I * H * D)
    if not debug_toggles_active():
        assert_fit_fused(trio.gpu, dims)
    trio.close()


def test_the_projected_step_is_right(gpu_ctx):
    B, H, S, E, K, D = PROJECTED
    trio = Trio(gpu_ctx, fit.projected(*PROJECTED))
    trio.gpu.fuse_attention_fit(True)
    rng = np.random.default_rng(70)
    trio.init_params(rng, -0.5, 0.5)
    x = u(rng, B, S, E)
    trio.call("out", {"x": x}, n=S)
    for _ in range(3):
        trio.step("fit", {"x": x, "labels": u(rng, B, S, H, D)}, n=B * S * H * D)
    if not debug_toggles_active():
        assert_fit_fused(trio.gpu, (B, H, S, S, K, D))
    trio.close()


@pytest.mark.parametrize("kwargs,scale", [({"scale_first": True}, "0.125"), ({"scale": None}, "1")], ids=["scale_first", "unscaled"])
def test_the_other_spellings_of_the_scale(gpu_ctx, kwargs, scale):
    dims = SHAPES[0]
    B, H, I, J, K, D = dims
    trio = Trio(gpu_ctx, fit.training(*dims, **kwargs))
    trio.gpu.fuse_attention_fit(True)
    trained(trio, (B, I, H, D), 5, steps=2)
    if not debug_toggles_active():
        assert_fit_fused(trio.gpu, dims, scale)
    trio.close()


# ---- 2. the plan ----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(debug_toggles_active(), reason="statements about the default plan")
def test_the_plan(gpu_ctx):
    """Fails without the feature.  One eg_attn launch with the sums, one eg_attn_grad launch, no product and no collapsed row
    group left in the training program's step; the softmax and the scores' gradient are not stored."""
    dims = SHAPES[0]
    B, H, I, J, K, D = dims
    graphs = ap.attention_training(*dims)
    text = refcases.program_text(graphs())
    m = egm.compile(*graphs(), gpu=gpu_ctx)
    m.fuse_attention_fit(True)
    labels = u(np.random.default_rng(1), B, I, H, D)
    m.apply("fit", {"labels": labels})
    assert_fit_fused(m, dims)
    lines = launches(m)
    fwd, bwd = fused_lines(m)
    assert "(scores, scaled, softmax.sums, softmax, context)" in fwd[0] and "accumulate" not in fwd[0] and "accumulate" not in bwd[0], lines
    assert bwd[0].count(",") >= 7, bwd            # eight members
    assert not any("eg_bgemm2" in l for l in lines), lines
    assert not any("eg_wrows" in l and "rows=" in l for l in lines), lines
    assert lines.index(fwd[0]) < lines.index(bwd[0]), lines
    assert "eg_attn_grad" in m.emit_ir()
    with pytest.raises(GpuError, match="eg_model_keep_values"):
        m.read_tensor("fit", tensor_id(text, "softmax"))
    # every tensor the plan never stores: scores, scaled and softmax of the program's own, and the four gradients between the
    # products (the softmax's, the sums', the scaled scores' and the scores'), which the library allocates behind them
    own = sum(1 for line in text.splitlines() if line.startswith("tensor "))
    hidden = []
    for tid in range(1, m_tensor_count(m) + 1):
        try:
            m.read_tensor("fit", tid)
        except GpuError as e:
            if "eg_model_keep_values" in str(e):
                hidden.append(tid)
    assert sorted(t for t in hidden if t <= own) == sorted(tensor_id(text, n) for n in ("scores", "scaled", "softmax")), hidden
    assert len([t for t in hidden if t > own]) == 4, hidden
    m.close()
    # the projected program: the same two launches, the projections keep theirs
    B, H, S, E, K, D = PROJECTED
    p = egm.compile(*fit.projected(*PROJECTED)(), gpu=gpu_ctx)
    p.fuse_attention_fit(True)
    rng = np.random.default_rng(2)
    p.apply("fit", {"x": u(rng, B, S, E), "labels": u(rng, B, S, H, D)})
    assert_fit_fused(p, (B, H, S, S, K, D))
    assert not any("eg_bgemm2" in l for l in launches(p)), launches(p)
    p.close()


def m_tensor_count(model):
    from exprgrad_amd import _lib
    return int(_lib.lib().eg_model_tensor_count(model.handle))


# ---- 3. off is the parent -------------------------------------------------------------------------------------------------------
def fresh(gpu_ctx, graphs, seed, on=None):
    m = egm.compile(*graphs(), gpu=gpu_ctx)
    rng = np.random.default_rng(seed)
    for tid in sorted(m.params.ids()):
        m.params[tid] = u(rng, *m.params[tid].shape)
    if on is not None:
        m.fuse_attention_fit(on)
    return m


def bits(model):
    return [model.params[tid].view(np.uint32) for tid in sorted(model.params.ids())]


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(bits(a), bits(b)))


def test_off_is_the_model_that_never_touched_it(gpu_ctx):
    dims = SHAPES[0]
    B, H, I, J, K, D = dims
    graphs = ap.attention_training(*dims)
    rng = np.random.default_rng(33)
    labels = [u(rng, B, I, H, D) for _ in range(6)]
    never = fresh(gpu_ctx, graphs, 3)
    toggled = fresh(gpu_ctx, graphs, 3, on=True)
    toggled.fuse_attention_fit(False)
    for step in range(2):
        never.apply("fit", {"labels": labels[step]})
        toggled.apply("fit", {"labels": labels[step]})
    assert never.launch_plan("fit") == toggled.launch_plan("fit")
    assert "eg_attn" not in never.launch_plan("fit") or debug_toggles_active()
    assert never.emit_ir() == toggled.emit_ir()
    assert same_bits(never, toggled)
    # on, off and on again against a model that was on throughout, from the same parameters
    always = fresh(gpu_ctx, graphs, 4, on=True)
    flipped = fresh(gpu_ctx, graphs, 4, on=True)
    for step in range(6):
        if step == 2:
            flipped.fuse_attention_fit(False)
        if step == 4:
            for tid in sorted(always.params.ids()):     # the off steps differ in rounding: start level again
                flipped.params[tid] = always.params[tid]
            flipped.fuse_attention_fit(True)
        always.apply("fit", {"labels": labels[step]})
        flipped.apply("fit", {"labels": labels[step]})
        if step in (2, 3) and not debug_toggles_active():
            assert "eg_attn" not in flipped.launch_plan("fit")
        if step >= 4 and not debug_toggles_active():
            assert_fit_fused(flipped, dims)
    assert same_bits(always, flipped)
    for m in (never, toggled, always, flipped):
        m.close()


# ---- 4. determinism and replay ----------------------------------------------------------------------------------------------------
def test_four_steps_replay_the_captured_graph(gpu_ctx):
    """new labels every step (the step's graph is captured on the second run and replayed afterwards): every step within TOL
    through Trio, and a twin model with the setting on ends with the same bits in every parameter"""
    dims = SHAPES[0]
    B, H, I, J, K, D = dims
    graphs = ap.attention_training(*dims)
    trio = Trio(gpu_ctx, graphs)
    trio.gpu.fuse_attention_fit(True)
    twin = egm.compile(*graphs(), gpu=gpu_ctx)
    twin.fuse_attention_fit(True)
    rng = np.random.default_rng(44)
    trio.init_params(rng, -0.5, 0.5)
    for tid in sorted(twin.params.ids()):
        twin.params[tid] = trio.gpu.params[tid]
    for _ in range(4):
        labels = u(rng, B, I, H, D)
        trio.step("fit", {"labels": labels}, n=B * I * H * D)
        twin.apply("fit", {"labels": labels})
    assert same_bits(trio.gpu, twin)
    if not debug_toggles_active():
        assert_fit_fused(twin, dims)
    twin.close()
    trio.close()


# ---- 5. what keeps the unfused plan -----------------------------------------------------------------------------------------------
MISSES = fit.near_misses()
RUNNABLE = sorted(name for name, miss in MISSES.items() if miss[3] is not None)


@pytest.mark.parametrize("name", RUNNABLE)
def test_near_misses_train_unfused(gpu_ctx, name):
    text, _, _, more = MISSES[name]
    B, H, I, J, K, D = fit.SHAPE
    labels_shape = fit.LABELS.get(name, (B, I, H, D))
    trio = Trio(gpu_ctx, None, text=text)
    trio.gpu.fuse_attention_fit(True)
    rng = np.random.default_rng(len(name))
    extra = {k: u(rng, *shape) for k, shape in sorted(more.items())}
    trained(trio, labels_shape, len(name) + 1, steps=2, more=extra)
    assert "eg_attn_grad" not in trio.gpu.launch_plan("fit"), trio.gpu.launch_plan("fit")
    trio.close()


def test_a_head_dimension_of_129_keeps_the_unfused_plan(gpu_ctx):
    dims = (1, 2, 9, 70, 129, 16)
    trio = Trio(gpu_ctx, ap.attention_training(*dims))
    trio.gpu.fuse_attention_fit(True)
    trained(trio, (1, 9, 2, 16), 129, steps=2)
    assert_fit_unfused(trio.gpu)
    trio.close()


def test_a_float64_model_is_not_fused(gpu_ctx):
    """against the oracle running the float64 program (its literals are doubles: the float32 program's shadow has 0.05 rounded
    to float32), at the 1e-12 that tests/test_gpu_conv64_model.py holds a float64 training step to"""
    from exprgrad_amd import dsl
    from oracle import kd
    dims = SHAPES[0]
    B, H, I, J, K, D = dims
    graphs = ap.attention_training(*dims)
    prog = dsl.to_program(*graphs())
    prog.scalar = "f64"
    m = egm.compile(*graphs(), gpu=gpu_ctx, dtype=np.float64)
    m.fuse_attention_fit(True)
    ref = kd.Model(prog.to_text())
    assert m.dtype == np.float64 and ref.c64
    rng = np.random.default_rng(64)
    for tid in sorted(ref.params):
        v = rng.uniform(-0.5, 0.5, ref.params[tid].shape)
        m.params[tid] = v
        ref.params[tid][...] = v
    labels = rng.uniform(-0.5, 0.5, (B, I, H, D))
    m.apply("fit", {"labels": labels})
    ref.apply("fit", {"labels": labels})
    for tid in sorted(ref.params):
        err = rel_err(m.params[tid], ref.params[tid], "float64 attention step, parameter %d" % tid)
        print("float64 step, parameter", tid, err)
        assert err <= 1e-12
    assert_fit_unfused(m)
    assert "eg_attn" not in m.emit_ir()
    m.close()


def test_keep_values_keeps_the_unfused_plan_and_gives_it_back(gpu_ctx):
    dims = SHAPES[0]
    B, H, I, J, K, D = dims
    graphs = ap.attention_training(*dims)
    text = refcases.program_text(graphs())
    trio = Trio(gpu_ctx, graphs)
    trio.gpu.fuse_attention_fit(True)
    trio.gpu.keep_values(True)
    trained(trio, (B, I, H, D), 6, steps=2)
    assert_fit_unfused(trio.gpu)
    softmax = trio.gpu.read_tensor("fit", tensor_id(text, "softmax"))
    assert softmax.shape == (B, H, I, J) and rel_err(softmax.sum(-1), np.ones((B, H, I)), "kept softmax rows sum to one") <= TOL
    trio.gpu.keep_values(False)
    trio.step("fit", {"labels": u(np.random.default_rng(7), B, I, H, D)}, n=B * I * H * D)
    if not debug_toggles_active():
        assert_fit_fused(trio.gpu, dims)
    trio.close()


@pytest.mark.parametrize("switch", ["EG_NO_ROWFUSE", "EG_NO_BATCHED_GEMM"])
def test_the_switches_of_its_parts_turn_it_off(gpu_ctx, monkeypatch, switch):
    dims = SHAPES[0]
    B, H, I, J, K, D = dims
    monkeypatch.setenv(switch, "1")
    trio = Trio(gpu_ctx, ap.attention_training(*dims))
    trio.gpu.fuse_attention_fit(True)
    trained(trio, (B, I, H, D), 8, steps=2)
    assert_fit_unfused(trio.gpu)
    trio.close()
    monkeypatch.delenv(switch)


# ---- 6. `out` and `loss` are unchanged ----------------------------------------------------------------------------------------------
def test_out_and_loss_keep_their_launch_and_their_bits(gpu_ctx):
    dims = SHAPES[0]
    B, H, I, J, K, D = dims
    graphs = ap.attention_training(*dims)
    labels = u(np.random.default_rng(12), B, I, H, D)
    off, on = fresh(gpu_ctx, graphs, 9), fresh(gpu_ctx, graphs, 9, on=True)
    for target, args in (("out", {}), ("loss", {"labels": labels})):
        a, b = np.array(off.call(target, args)), np.array(on.call(target, args))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), target
        assert off.launch_plan(target) == on.launch_plan(target), target
        if not debug_toggles_active():
            attn = [l for l in launches(on, target) if "eg_attn" in l]
            assert len(attn) == 1 and "eg_attn_grad" not in attn[0] and "sums=" not in attn[0], launches(on, target)
    off.close()
    on.close()
