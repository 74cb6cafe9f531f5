"""Model route of the products with a leading batch index in a compile[float64] model: the programs of
tests/batched_programs.py, compiled with dtype=np.float64, run beside oracle.kd.Model on the `f64` text of the same
program (the step_pair / compare_state pattern of tests/test_gpu_f64.py; bound: that file's 1e-12 relative), and the plan
text shows what ran them: `eg_bgemm` launches (eg_dgemm_batched) for the batched form, plain `gemm` launches (eg_dgemm)
over the collapsed extents for the shared-weight forms, and no generated kernel for either.  (The statements about the plan
hold in the default configuration only: under an `execution` switch such as EG_NO_BATCHED_GEMM=1 the numbers are checked
alone.)"""
import numpy as np
import pytest

import batched_programs as bp
from conftest import debug_toggles_active
from exprgrad_amd import dsl
from exprgrad_amd import model as egm

pytestmark = pytest.mark.gpu
TOL64 = 1e-12


def rel(got, want):
    want = np.asarray(want, np.float64)
    scale = max(float(np.max(np.abs(want))) if want.size else 0.0, 1e-300)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want))) / scale if want.size else 0.0


def text64(graphs):
    prog = dsl.to_program(*graphs)
    prog.scalar = "f64"
    return prog.to_text()


def step_pair(gpu_ctx, graphs_fn, seed, lo=-0.5, hi=0.5):
    from oracle import kd
    gpu = egm.compile(*graphs_fn(), gpu=gpu_ctx, dtype=np.float64)
    ref = kd.Model(text64(graphs_fn()))
    assert gpu.dtype == np.float64 and ref.c64
    rng = np.random.default_rng(seed)
    for tid in sorted(ref.params):
        v = lo + (hi - lo) * rng.random(ref.params[tid].shape)
        ref.params[tid][...] = v
        gpu.params[tid] = v
    return gpu, ref, rng


def compare_state(gpu, ref, tol=TOL64, what=""):
    for tid in sorted(ref.params):
        assert rel(gpu.params[tid], ref.params[tid]) <= tol, (what, "param", tid, rel(gpu.params[tid], ref.params[tid]))
    for tid in sorted(ref.caches):
        assert rel(gpu.caches[tid], ref.caches[tid]) <= tol, (what, "cache", tid)


def launches(model, target):
    return [line for line in model.launch_plan(target).splitlines() if line.startswith("[")]


def training_steps(gpu, ref, inputs, steps=2):
    """`steps` steps from identical state: the loss, every parameter gradient and the updated parameters."""
    for step in range(steps):
        assert rel(gpu.call("loss", inputs), ref.call("loss", inputs)) <= TOL64, ("loss", step)
        gpu.apply("fit", inputs)
        ref.apply("fit", inputs)
        grads = ref.prog.param_grads["fit"]
        assert grads
        for _, gt in grads:
            assert rel(gpu.read_tensor("fit", gt), ref.last[gt]) <= TOL64, ("gradient", gt, step)
        compare_state(gpu, ref, TOL64, f"step {step}")


def test_batched_forward_f64(gpu_ctx):
    G, I, J, K = 5, 33, 20, 17
    gpu, ref, rng = step_pair(gpu_ctx, bp.batched_forward, 1)
    a, b = rng.random((G, I, K)) - 0.5, rng.random((G, K, J)) - 0.5
    got, want = gpu.call("out", {"a": a, "b": b}), ref.call("out", {"a": a, "b": b})
    assert got.dtype == np.float64 and got.shape == (G, I, J)
    assert rel(got, want) <= TOL64 and rel(got, np.einsum("gik,gkj->gij", a, b)) <= TOL64
    if not debug_toggles_active():
        lines = launches(gpu, "out")
        assert len(lines) == 1 and "eg_bgemm NN 5 x 33x20x17" in lines[0], lines
        assert "generic" not in gpu.emit_ir()
    gpu.close()


def test_batched_training_step_f64(gpu_ctx):
    """The backward pass holds both derived gradients: gout * b^T (NT) and a^T * gout (TN)."""
    G, I, J, K = 5, 33, 20, 17
    gpu, ref, rng = step_pair(gpu_ctx, bp.batched_training(G, I, J, K), 2)
    training_steps(gpu, ref, {"labels": rng.random((G, I, J)) - 0.5})
    if not debug_toggles_active():
        lines = launches(gpu, "fit")
        batched = [l for l in lines if "eg_bgemm" in l]
        assert len(batched) == 3 and sorted(l.split()[2] for l in batched) == ["NN", "NT", "TN"], lines
        ir = [l for l in gpu.emit_ir().split("target fit")[1].split("target ")[0].splitlines() if "eg_bgemm" in l or "generic" in l]
        # every kernel has ONE line in the lowering text: the three products are eg_bgemm there, so none of them is generated
        assert sum("eg_bgemm" in l for l in ir) == 3, ir
    assert rel(gpu.call("out", {}), ref.call("out", {})) <= TOL64
    gpu.close()


def test_shared_weight_training_step_f64(gpu_ctx):
    G, I, K, J, H = 4, 19, 10, 24, 8
    gpu, ref, rng = step_pair(gpu_ctx, bp.shared_training(K, J, H), 3)
    x, labels = rng.random((G, I, K)) - 0.5, rng.random((G, I, H)) - 0.5
    training_steps(gpu, ref, {"x": x, "labels": labels})
    if not debug_toggles_active():
        lines = launches(gpu, "fit")
        collapsed = [l for l in lines if "(batch rows collapsed)" in l]
        # two forwards and the input gradient with M = G * I = 76, two weight gradients with K = G * I
        assert len(collapsed) == 5 and all(l.split()[1] == "gemm" for l in collapsed), lines
        assert sorted(l.split()[2] for l in collapsed) == ["NN", "NN", "NT", "TN", "TN"], lines
        assert sum(" 76x" in l for l in collapsed) == 3 and sum(l.split()[3].endswith("x76") for l in collapsed) == 2, lines
        assert not [l for l in lines if "eg_bgemm" in l]
        fit_ir = gpu.emit_ir().split("target fit")[1].split("target ")[0]
        assert fit_ir.count("gemm(batch rows collapsed") == 5 and "generic(map|split-reduce)" not in fit_ir, fit_ir
    assert rel(gpu.call("out", {"x": x}), ref.call("out", {"x": x})) <= TOL64
    gpu.close()


def test_batch_index_in_the_middle_stays_generated_f64(gpu_ctx):
    G, I, J, K = 5, 33, 20, 17
    gpu, ref, rng = step_pair(gpu_ctx, bp.batch_in_the_middle, 4)
    a, b = rng.random((I, G, K)) - 0.5, rng.random((G, K, J)) - 0.5
    got = gpu.call("out", {"a": a, "b": b})
    assert rel(got, ref.call("out", {"a": a, "b": b})) <= TOL64 and rel(got, np.einsum("igk,gkj->igj", a, b)) <= TOL64
    lines = launches(gpu, "out")
    assert len(lines) == 1 and "generated" in lines[0] and "eg_bgemm" not in gpu.emit_ir(), lines
    gpu.close()


def test_fit_under_graph_capture_is_reproducible_f64(gpu_ctx):
    """Three steps of eg_model_fit (the launch sequence is captured on its second run and replayed on the third): a second
    model that starts from the same parameters ends with the same bits."""
    G, I, J, K = 5, 33, 20, 17
    graphs = bp.batched_training(G, I, J, K)
    labels = np.random.default_rng(5).random((3 * G, I, J)) - 0.5
    results = []
    for _ in range(2):
        m = egm.compile(*graphs(), gpu=gpu_ctx, dtype=np.float64)
        init = np.random.default_rng(6)
        start = {}
        for tid in sorted(m.params.ids()):
            start[tid] = init.random(m.params[tid].shape) - 0.5
            m.params[tid] = start[tid]
        m.fit("fit", {"labels": labels}, batch_size=G)
        assert debug_toggles_active() or m.launch_plan("fit").count("eg_bgemm") == 3
        results.append({tid: m.params[tid].copy() for tid in sorted(m.params.ids())})
        assert all(r.dtype == np.float64 for r in results[-1].values())
        assert any(not np.array_equal(results[-1][tid], start[tid]) for tid in start)       # the steps did run
        m.close()
    for tid in results[0]:
        assert np.all(np.isfinite(results[0][tid]))
        assert np.array_equal(results[0][tid].view(np.uint64), results[1][tid].view(np.uint64)), tid
