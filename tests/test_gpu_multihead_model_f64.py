"""Model route of the products with two batch indices in a compile[float64] model, under Model.batched2_f64()
(eg_model_batched2_f64, off by default): the programs of tests/multihead_programs.py and the attention block
(tests/attention_fused_programs.py, tests/attention_programs.py), compiled with dtype=np.float64, run beside oracle.kd.Model
on the `f64` text of the same program (the step_pair / compare_state pattern of tests/test_gpu_f64.py; bound: that file's
1e-12 relative), and the plan text shows what ran them: `eg_bgemm2` launches (eg_dgemm_batched2's internal entry) and no
generated kernel for a product.  With the setting off the same models show the text they always had.  (The statements about
the plan hold in the default configuration only: under an `execution` switch such as EG_NO_BATCHED_GEMM=1 the numbers are
checked alone.)"""
import numpy as np
import pytest

import attention_fused_programs as fp
import attention_programs as ap
import multihead_programs as mh
from conftest import debug_toggles_active
from exprgrad_amd import dsl
from exprgrad_amd import model as egm

pytestmark = pytest.mark.gpu
TOL64 = 1e-12
B, H, I, J, K = 2, 3, 33, 20, 16


def rel(got, want):
    want = np.asarray(want, np.float64)
    scale = max(float(np.max(np.abs(want))) if want.size else 0.0, 1e-300)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want))) / scale if want.size else 0.0


def text64(graphs):
    prog = dsl.to_program(*graphs)
    prog.scalar = "f64"
    return prog.to_text()


def pair(gpu_ctx, graphs_fn, seed, on=True):
    """The model under test and the oracle on the float64 text, from identical parameters."""
    from oracle import kd
    gpu = egm.compile(*graphs_fn(), gpu=gpu_ctx, dtype=np.float64)
    if on is not None:
        gpu.batched2_f64(on)
    ref = kd.Model(text64(graphs_fn()))
    assert gpu.dtype == np.float64 and ref.c64
    rng = np.random.default_rng(seed)
    for tid in sorted(ref.params):
        v = rng.random(ref.params[tid].shape) - 0.5
        ref.params[tid][...] = v
        gpu.params[tid] = v
    return gpu, ref, rng


def compare_state(gpu, ref, what=""):
    for tid in sorted(ref.params):
        assert rel(gpu.params[tid], ref.params[tid]) <= TOL64, (what, "param", tid, rel(gpu.params[tid], ref.params[tid]))


def training_steps(gpu, ref, inputs, steps):
    """`steps` steps from identical state: the loss, every parameter gradient and the updated parameters."""
    for step in range(steps):
        assert rel(gpu.call("loss", inputs), ref.call("loss", inputs)) <= TOL64, ("loss", step)
        gpu.apply("fit", inputs)
        ref.apply("fit", inputs)
        grads = ref.prog.param_grads["fit"]
        assert grads
        for _, gt in grads:
            assert rel(gpu.read_tensor("fit", gt), ref.last[gt]) <= TOL64, ("gradient", gt, step)
        compare_state(gpu, ref, f"step {step}")


def launches(model, target):
    return [line for line in model.launch_plan(target).splitlines() if line.startswith("[")]


def batched(model, target):
    """{layout: "b0xb1 x MxNxK"} of the target's eg_bgemm2 launches, and their count"""
    lines = [l for l in launches(model, target) if "eg_bgemm2" in l]
    return {l.split()[2]: " ".join(l.split()[3:6]) for l in lines}, len(lines)


def lowering(model, target):
    """The lines of the lowering text of one target that name a product route or a generated kernel."""
    return [l for l in model.emit_ir().split("target " + target)[1].split("target ")[0].splitlines() if "eg_bgemm" in l or "generic" in l]


def generated_products(model, target):
    """Launch lines of generated kernels whose kernel the lowering text names eg_bgemm2: products that ran generated."""
    ir = model.emit_ir().split("target " + target)[1].split("target ")[0].splitlines()
    products = {l.split("]")[0].strip().lstrip("[") for l in ir if "] eg_bgemm2" in l}
    return [l for l in launches(model, target) if "generated" in l and l.split(" kernel ")[1].split()[0] in products]


# ---- 1. each program against the oracle, and what ran it ---------------------------------------------------------------------------
def test_scores_forward(gpu_ctx):
    gpu, ref, rng = pair(gpu_ctx, mh.scores_forward, 1)
    x = {"q": rng.random((B, I, H, K)) - 0.5, "kk": rng.random((B, J, H, K)) - 0.5}
    got = gpu.call("out", x)
    assert got.dtype == np.float64 and got.shape == (B, H, I, J)
    assert rel(got, ref.call("out", x)) <= TOL64 and rel(got, np.einsum("bihk,bjhk->bhij", x["q"], x["kk"])) <= TOL64
    if not debug_toggles_active():
        lines = launches(gpu, "out")
        assert len(lines) == 1 and "eg_bgemm2 NT 2x3 x 33x20x16" in lines[0], lines
        assert "generic" not in gpu.emit_ir() and "eg_bgemm2 NT" in gpu.emit_ir()
    gpu.close()


def test_context_forward(gpu_ctx):
    """o[b,i,h,d] ++= p[b,h,i,j] * v[b,j,h,d]: the items of the output interleave (ldc = H * D, head stride D)."""
    D = 16
    gpu, ref, rng = pair(gpu_ctx, mh.context_forward, 3)
    x = {"p": rng.random((B, H, I, J)) - 0.5, "v": rng.random((B, J, H, D)) - 0.5}
    got = gpu.call("out", x)
    assert got.shape == (B, I, H, D)
    assert rel(got, ref.call("out", x)) <= TOL64 and rel(got, np.einsum("bhij,bjhd->bihd", x["p"], x["v"])) <= TOL64
    if not debug_toggles_active():
        lines = launches(gpu, "out")
        assert len(lines) == 1 and "eg_bgemm2 NN 2x3 x 33x16x20" in lines[0], lines
        assert "generic" not in gpu.emit_ir()
    gpu.close()


def test_scores_training_two_steps(gpu_ctx):
    """The backward pass holds both derived gradients: gs * kk (NN) for q and gs^T * q (TN) for kk."""
    gpu, ref, rng = pair(gpu_ctx, mh.scores_training(B, H, I, J, K), 2)
    training_steps(gpu, ref, {"labels": rng.random((B, H, I, J)) - 0.5}, steps=2)
    if not debug_toggles_active():
        shapes, n = batched(gpu, "fit")
        assert n == 3 and shapes == {"NT": "2x3 x 33x20x16", "NN": "2x3 x 33x16x20", "TN": "2x3 x 20x16x33"}, launches(gpu, "fit")
        assert sum("eg_bgemm2" in l for l in lowering(gpu, "fit")) == 3, lowering(gpu, "fit")
        assert generated_products(gpu, "fit") == []
    assert rel(gpu.call("out", {}), ref.call("out", {})) <= TOL64
    gpu.close()


def test_attention_forward_chain(gpu_ctx):
    """scores -> scale -> softmax -> context at (2, 3, 33, 70, 16, 16): the two products are eg_bgemm2 launches, the chain
    between them stays generated `double` code (no eg_attn, no row group)."""
    B_, H_, I_, J_, K_, D_ = ap.TRAINING_SHAPE
    gpu, ref, rng = pair(gpu_ctx, fp.attention_forward(), 4)
    x = {"q": rng.random((B_, I_, H_, K_)) - 0.5, "kk": rng.random((B_, J_, H_, K_)) - 0.5, "v": rng.random((B_, J_, H_, D_)) - 0.5}
    got = gpu.call("out", x)
    e = np.exp(np.einsum("bihk,bjhk->bhij", x["q"], x["kk"]) * fp.SCALE)
    assert rel(got, ref.call("out", x)) <= TOL64 and rel(got, np.einsum("bhij,bjhd->bihd", e / e.sum(-1, keepdims=True), x["v"])) <= TOL64
    if not debug_toggles_active():
        shapes, n = batched(gpu, "out")
        assert n == 2 and shapes == {"NT": "2x3 x 33x70x16", "NN": "2x3 x 33x16x70"}, launches(gpu, "out")
        assert "eg_attn" not in gpu.launch_plan("out") and any("generated" in l for l in launches(gpu, "out"))
    gpu.close()


def test_attention_training_step(gpu_ctx):
    """One step of the whole block: six products — scores NT and context NN, the softmax's gradient NT, dv TN, dq NN, dk TN —
    as six eg_bgemm2 launches; every gradient and every updated parameter against the oracle."""
    dims = ap.TRAINING_SHAPE
    B_, H_, I_, J_, K_, D_ = dims
    gpu, ref, rng = pair(gpu_ctx, ap.attention_training(*dims), 5)
    training_steps(gpu, ref, {"labels": rng.random((B_, I_, H_, D_)) - 0.5}, steps=1)
    if not debug_toggles_active():
        lines = [l for l in launches(gpu, "fit") if "eg_bgemm2" in l]
        assert sorted(l.split()[2] for l in lines) == ["NN", "NN", "NT", "NT", "TN", "TN"], launches(gpu, "fit")
        assert sum("eg_bgemm2" in l for l in lowering(gpu, "fit")) == 6, lowering(gpu, "fit")
        assert "eg_attn" not in gpu.launch_plan("fit") and generated_products(gpu, "fit") == []
    gpu.close()


# ---- 2. off is today's model -----------------------------------------------------------------------------------------------------------
def test_off_is_the_text_of_a_model_that_never_heard_of_it(gpu_ctx):
    """Never set, set to off, and on -> off: one lowering text and one launch text, all products generated."""
    graphs = mh.scores_training(B, H, I, J, K)
    labels = {"labels": np.random.default_rng(6).random((B, H, I, J)) - 0.5}
    texts = []
    for on in (None, False, "toggle"):
        gpu, ref, _ = pair(gpu_ctx, graphs, 6, on=None if on == "toggle" else on)
        if on == "toggle":
            gpu.batched2_f64(True)
            assert "eg_bgemm2" in gpu.emit_ir()
            gpu.batched2_f64(False)
        training_steps(gpu, ref, labels, steps=1)
        assert "eg_bgemm" not in gpu.emit_ir() and "eg_bgemm" not in gpu.launch_plan("fit")
        texts.append((gpu.emit_ir(), gpu.launch_plan("fit")))
        gpu.close()
    assert texts[0] == texts[1] == texts[2]


def test_off_on_off_with_a_captured_fit_in_between(gpu_ctx):
    """One model through off -> on -> off, three steps of fit() at every stage (the launch sequence is captured on its second
    run and replayed on the third): the oracle's parameters after every stage, and the plan of the stage."""
    graphs = mh.scores_training(B, H, I, J, K)
    gpu, ref, rng = pair(gpu_ctx, graphs, 7, on=None)
    for stage, on in enumerate((False, True, False)):
        gpu.batched2_f64(on)
        labels = rng.random((3 * B, H, I, J)) - 0.5
        gpu.fit("fit", {"labels": labels}, batch_size=B)
        for s in range(3):
            ref.apply("fit", {"labels": labels[s * B:(s + 1) * B]})
        compare_state(gpu, ref, f"stage {stage}")
        if not debug_toggles_active():
            assert gpu.launch_plan("fit").count("eg_bgemm2") == (3 if on else 0), (stage, gpu.launch_plan("fit"))
            assert ("eg_bgemm2" in gpu.emit_ir()) == on
    gpu.close()


# ---- 3. what the route declines ------------------------------------------------------------------------------------------------------
def test_batch_register_last_stays_generated(gpu_ctx):
    gpu, ref, rng = pair(gpu_ctx, mh.batch_register_last, 8)
    x = {"q": rng.random((B, I, K, H)) - 0.5, "kk": rng.random((B, J, H, K)) - 0.5}
    assert rel(gpu.call("out", x), ref.call("out", x)) <= TOL64
    lines = launches(gpu, "out")
    assert len(lines) == 1 and "generated" in lines[0] and "eg_bgemm" not in gpu.emit_ir(), lines
    gpu.close()


@pytest.mark.parametrize("empty", ["I", "K"])
def test_an_empty_extent_runs_the_generated_kernel_of_that_plan(gpu_ctx, empty):
    """plan_batched2 declines an empty sequence or an empty contraction: that plan runs the generated kernel, built when
    first needed; the same model then runs the full shape as one eg_bgemm2 launch."""
    rng = np.random.default_rng(9)
    m = egm.compile(*mh.scores_forward(), gpu=gpu_ctx, dtype=np.float64)
    m.batched2_f64()
    i0, k0 = (0, K) if empty == "I" else (I, 0)
    got = m.call("out", {"q": rng.random((B, i0, H, k0)), "kk": rng.random((B, J, H, k0))})
    assert got.shape == (B, H, i0, J) and not np.any(got)
    lines = launches(m, "out")
    assert len(lines) == 1 and "generated" in lines[0], lines
    q, kk = rng.random((B, I, H, K)) - 0.5, rng.random((B, J, H, K)) - 0.5
    assert rel(m.call("out", {"q": q, "kk": kk}), np.einsum("bihk,bjhk->bhij", q, kk)) <= TOL64
    assert debug_toggles_active() or "eg_bgemm2 NT 2x3 x 33x20x16" in launches(m, "out")[0]
    m.close()


def test_the_switch_of_the_batched_products_turns_it_off(gpu_ctx, monkeypatch):
    monkeypatch.setenv("EG_NO_BATCHED_GEMM", "1")
    gpu, ref, rng = pair(gpu_ctx, mh.scores_training(B, H, I, J, K), 10)
    training_steps(gpu, ref, {"labels": rng.random((B, H, I, J)) - 0.5}, steps=1)
    assert "eg_bgemm" not in gpu.launch_plan("fit") and "eg_bgemm" not in gpu.emit_ir()
    gpu.close()
    monkeypatch.delenv("EG_NO_BATCHED_GEMM")


def test_a_float32_model_refuses_the_setting(gpu_ctx):
    m = egm.compile(*mh.scores_forward(), gpu=gpu_ctx)
    with pytest.raises(Exception, match="float32"):
        m.batched2_f64()
    m.close()


# ---- 4. capture ---------------------------------------------------------------------------------------------------------------------------
def test_fit_under_graph_capture_is_reproducible(gpu_ctx):
    """Three steps of eg_model_fit (the launch sequence is captured on its second run and replayed on the third): a second
    model that starts from the same parameters ends with the same bits."""
    graphs = mh.scores_training(B, H, I, J, K)
    labels = np.random.default_rng(11).random((3 * B, H, I, J)) - 0.5
    results = []
    for _ in range(2):
        m = egm.compile(*graphs(), gpu=gpu_ctx, dtype=np.float64)
        m.batched2_f64()
        init = np.random.default_rng(12)
        start = {}
        for tid in sorted(m.params.ids()):
            start[tid] = init.random(m.params[tid].shape) - 0.5
            m.params[tid] = start[tid]
        m.fit("fit", {"labels": labels}, batch_size=B)
        assert debug_toggles_active() or m.launch_plan("fit").count("eg_bgemm2") == 3
        results.append({tid: m.params[tid].copy() for tid in sorted(m.params.ids())})
        assert any(not np.array_equal(results[-1][tid], start[tid]) for tid in start)       # the steps did run
        m.close()
    for tid in results[0]:
        assert np.all(np.isfinite(results[0][tid]))
        assert np.array_equal(results[0][tid].view(np.uint64), results[1][tid].view(np.uint64)), tid
