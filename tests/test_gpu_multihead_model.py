"""Model route of the products with two batch indices (csrc/host/match.cpp match_batched2_gemm): the multi-head programs of
tests/multihead_programs.py run three ways (tests/parity.py: backend | oracle | float64 shadow), and the plan text shows what
ran them: `eg_bgemm2` launches (eg_sgemm_batched2's internal entry) and no generated kernel.  An operand that ends in a batch
register and a compile[float64] model keep their generated kernels.  (The statements about the plan hold in the default
configuration only: under an `execution` switch such as EG_NO_BATCHED_GEMM=1 the numbers are checked alone.)"""
import numpy as np
import pytest

import multihead_programs as mh
from conftest import TOL, debug_toggles_active
from exprgrad_amd import dsl
from exprgrad_amd import model as egm
from parity import Trio

pytestmark = pytest.mark.gpu

B, H, I, J, K = 2, 3, 33, 20, 16


def u(rng, *shape):
    return (rng.random(shape, dtype=np.float32) - np.float32(0.5)).astype(np.float32)


def launches(model, target):
    return [line for line in model.launch_plan(target).splitlines() if line.startswith("[")]


def test_scores_forward(gpu_ctx):
    rng = np.random.default_rng(1)
    trio = Trio(gpu_ctx, mh.scores_forward)
    q, kk = u(rng, B, I, H, K), u(rng, B, J, H, K)
    got = trio.call("out", {"q": q, "kk": kk}, n=K)
    assert got.shape == (B, H, I, J)
    if not debug_toggles_active():
        lines = launches(trio.gpu, "out")
        assert len(lines) == 1 and "eg_bgemm2 NT 2x3 x 33x20x16" in lines[0], lines
        assert "generic" not in trio.gpu.emit_ir() and "eg_bgemm2 NT" in trio.gpu.emit_ir()
    trio.close()


def test_scores_training_step(gpu_ctx):
    """The backward pass holds both derived gradients: gs * kk (NN) for q and gs^T * q (TN) for kk, as
    tests/test_batched2_cpu.py finds them."""
    rng = np.random.default_rng(2)
    trio = Trio(gpu_ctx, mh.scores_training(B, H, I, J, K))
    trio.init_params(rng, -0.5, 0.5)
    labels = u(rng, B, H, I, J)
    for _ in range(2):
        trio.step("fit", {"labels": labels}, n=B * H * I * J)
    if not debug_toggles_active():
        lines = launches(trio.gpu, "fit")
        batched = [l for l in lines if "eg_bgemm2" in l]
        assert len(batched) == 3 and sorted(l.split()[2] for l in batched) == ["NN", "NT", "TN"], lines
        shapes = {l.split()[2]: " ".join(l.split()[3:6]) for l in batched}
        assert shapes == {"NT": "2x3 x 33x20x16", "NN": "2x3 x 33x16x20", "TN": "2x3 x 20x16x33"}, lines
        ir = [l for l in trio.gpu.emit_ir().split("target fit")[1].split("target ")[0].splitlines() if "eg_bgemm" in l or "generic" in l]
        # every kernel has ONE line in the lowering text: the three products are eg_bgemm2 there, so none of them is generated
        assert sum("eg_bgemm2" in l for l in ir) == 3, ir
    trio.call("out", {}, n=K)
    trio.close()


def test_context_forward(gpu_ctx):
    """o[b,i,h,d] ++= p[b,h,i,j] * v[b,j,h,d]: the items of the output interleave (ldc = H * D, head stride D)."""
    D = 16
    rng = np.random.default_rng(3)
    trio = Trio(gpu_ctx, mh.context_forward)
    got = trio.call("out", {"p": u(rng, B, H, I, J), "v": u(rng, B, J, H, D)}, n=J)
    assert got.shape == (B, I, H, D)
    if not debug_toggles_active():
        lines = launches(trio.gpu, "out")
        assert len(lines) == 1 and "eg_bgemm2 NN 2x3 x 33x16x20" in lines[0], lines
        assert "generic" not in trio.gpu.emit_ir()
    trio.close()


def test_batch_register_last_stays_generated(gpu_ctx):
    rng = np.random.default_rng(4)
    trio = Trio(gpu_ctx, mh.batch_register_last)
    trio.call("out", {"q": u(rng, B, I, K, H), "kk": u(rng, B, J, H, K)}, n=K)
    lines = launches(trio.gpu, "out")
    assert len(lines) == 1 and "generated" in lines[0] and "eg_bgemm" not in trio.gpu.emit_ir(), lines
    trio.close()


@pytest.mark.parametrize("empty", ["I", "K"])
def test_an_empty_extent_runs_the_generated_kernel_of_that_plan(gpu_ctx, empty):
    """The route is decided plan by plan (plan_batched2): with an empty sequence or an empty contraction the shapes do not
    suit the launch and the plan runs the generated kernel, built when first needed — an empty output, or zeros; the same
    model then runs the full shape as one eg_bgemm2 launch."""
    rng = np.random.default_rng(7)
    m = egm.compile(*mh.scores_forward(), gpu=gpu_ctx)
    i0, k0 = (0, K) if empty == "I" else (I, 0)
    got = m.call("out", {"q": u(rng, B, i0, H, k0), "kk": u(rng, B, J, H, k0)})
    assert got.shape == (B, H, i0, J) and not np.any(got)
    lines = launches(m, "out")
    assert len(lines) == 1 and "generated" in lines[0], lines
    q, kk = u(rng, B, I, H, K), u(rng, B, J, H, K)
    got = m.call("out", {"q": q, "kk": kk})
    exact = np.einsum("bihk,bjhk->bhij", q.astype(np.float64), kk.astype(np.float64))
    assert float(np.max(np.abs(got - exact)) / np.max(np.abs(exact))) <= TOL
    assert debug_toggles_active() or "eg_bgemm2 NT 2x3 x 33x20x16" in launches(m, "out")[0]
    m.close()


def test_scores_forward_f64_stays_generated(gpu_ctx):
    """A compile[float64] model has no library entry for this form yet: the generated kernel, against the oracle's float64
    form of the same program at the 1e-12 of tests/test_gpu_f64.py."""
    from oracle import kd
    prog = dsl.to_program(*mh.scores_forward())
    prog.scalar = "f64"
    gpu = egm.compile(*mh.scores_forward(), gpu=gpu_ctx, dtype=np.float64)
    ref = kd.Model(prog.to_text())
    assert gpu.dtype == np.float64 and ref.c64
    rng = np.random.default_rng(5)
    q, kk = rng.random((B, I, H, K)) - 0.5, rng.random((B, J, H, K)) - 0.5
    got, want = gpu.call("out", {"q": q, "kk": kk}), ref.call("out", {"q": q, "kk": kk})
    rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    assert got.dtype == np.float64 and got.shape == (B, H, I, J)
    assert rel(got, want) <= 1e-12 and rel(got, np.einsum("bihk,bjhk->bhij", q, kk)) <= 1e-12
    lines = launches(gpu, "out")
    assert len(lines) == 1 and "generated" in lines[0] and "eg_bgemm" not in gpu.emit_ir(), lines
    gpu.close()


def test_fit_under_graph_capture_is_reproducible(gpu_ctx):
    """Three steps of eg_model_fit (the launch sequence is captured on its second run and replayed on the third): a second
    model that starts from the same parameters ends with the same bits."""
    graphs = mh.scores_training(B, H, I, J, K)
    labels = u(np.random.default_rng(5), 3 * B, H, I, J)
    results = []
    for _ in range(2):
        m = egm.compile(*graphs(), gpu=gpu_ctx)
        init = np.random.default_rng(6)
        start = {}
        for tid in sorted(m.params.ids()):
            start[tid] = u(init, *m.params[tid].shape)
            m.params[tid] = start[tid]
        m.fit("fit", {"labels": labels}, batch_size=B)
        assert debug_toggles_active() or m.launch_plan("fit").count("eg_bgemm2") == 3
        results.append({tid: m.params[tid].copy() for tid in sorted(m.params.ids())})
        assert any(not np.array_equal(results[-1][tid], start[tid]) for tid in start)       # the steps did run
        m.close()
    for tid in results[0]:
        assert np.all(np.isfinite(results[0][tid]))
        assert np.array_equal(results[0][tid].view(np.uint32), results[1][tid].view(np.uint32)), tid
