"""Model route of the products with a leading batch index (csrc/host/match.cpp match_batched_gemm): programs written with
exprgrad_amd.dsl (tests/batched_programs.py) run three ways (tests/parity.py: backend | oracle | float64 shadow), and the
plan text shows what ran them: `eg_bgemm` launches for the batched form, plain `gemm` launches over the collapsed extents
for the shared-weight forms, and no generated kernel for either.  (The statements about the plan hold in the default
configuration only: under an `execution` switch such as EG_NO_BATCHED_GEMM=1 the numbers are checked alone.)"""
import numpy as np
import pytest

import batched_programs as bp
from conftest import debug_toggles_active
from exprgrad_amd import model as egm
from parity import Trio

pytestmark = pytest.mark.gpu


def u(rng, *shape):
    return (rng.random(shape, dtype=np.float32) - np.float32(0.5)).astype(np.float32)


def launches(trio, target):
    return [line for line in trio.gpu.launch_plan(target).splitlines() if line.startswith("[")]


def test_batched_forward(gpu_ctx):
    G, I, J, K = 5, 33, 20, 17
    rng = np.random.default_rng(1)
    trio = Trio(gpu_ctx, bp.batched_forward)
    trio.call("out", {"a": u(rng, G, I, K), "b": u(rng, G, K, J)}, n=K)
    if not debug_toggles_active():
        lines = launches(trio, "out")
        assert len(lines) == 1 and "eg_bgemm NN 5 x 33x20x17" in lines[0], lines
        assert "generic" not in trio.gpu.emit_ir()
    trio.close()


def test_batched_training_step(gpu_ctx):
    """The backward pass holds both derived gradients: gout * b^T (NT) and a^T * gout (TN)."""
    G, I, J, K = 5, 33, 20, 17
    rng = np.random.default_rng(2)
    trio = Trio(gpu_ctx, bp.batched_training(G, I, J, K))
    trio.init_params(rng, -0.5, 0.5)
    labels = u(rng, G, I, J)
    for _ in range(2):
        trio.step("fit", {"labels": labels}, n=G * I * J)
    if not debug_toggles_active():
        lines = launches(trio, "fit")
        batched = [l for l in lines if "eg_bgemm" in l]
        assert len(batched) == 3 and sorted(l.split()[2] for l in batched) == ["NN", "NT", "TN"], lines
        ir = [l for l in trio.gpu.emit_ir().split("target fit")[1].split("target ")[0].splitlines() if "eg_bgemm" in l or "generic" in l]
        assert sum("eg_bgemm" in l for l in ir) == 3, ir
        # (every kernel has ONE line in the lowering text: the three products are eg_bgemm there, so none of them is generated)
    trio.call("out", {}, n=K)
    trio.close()


def test_shared_weight_training_step(gpu_ctx):
    G, I, K, J, H = 4, 19, 10, 24, 8
    rng = np.random.default_rng(3)
    trio = Trio(gpu_ctx, bp.shared_training(K, J, H))
    trio.init_params(rng, -0.5, 0.5)
    x, labels = u(rng, G, I, K), u(rng, G, I, H)
    for _ in range(2):
        trio.step("fit", {"x": x, "labels": labels}, n=G * I)
    if not debug_toggles_active():
        lines = launches(trio, "fit")
        collapsed = [l for l in lines if "(batch rows collapsed)" in l]
        # two forwards and the input gradient with M = G * I = 76, two weight gradients with K = G * I
        assert len(collapsed) == 5 and all(l.split()[1] == "gemm" for l in collapsed), lines
        assert sorted(l.split()[2] for l in collapsed) == ["NN", "NN", "NT", "TN", "TN"], lines
        assert sum(" 76x" in l for l in collapsed) == 3 and sum(l.split()[3].endswith("x76") for l in collapsed) == 2, lines
        assert not [l for l in lines if "eg_bgemm" in l]
        fit_ir = trio.gpu.emit_ir().split("target fit")[1].split("target ")[0]
        assert fit_ir.count("gemm(batch rows collapsed") == 5 and "generic(map|split-reduce)" not in fit_ir, fit_ir
    trio.call("out", {"x": x}, n=J)
    trio.close()


def test_batch_index_in_the_middle_stays_generated(gpu_ctx):
    G, I, J, K = 5, 33, 20, 17
    rng = np.random.default_rng(4)
    trio = Trio(gpu_ctx, bp.batch_in_the_middle)
    trio.call("out", {"a": u(rng, I, G, K), "b": u(rng, G, K, J)}, n=K)
    lines = launches(trio, "out")
    assert len(lines) == 1 and "generated" in lines[0] and "eg_bgemm" not in trio.gpu.emit_ir(), lines
    trio.close()


def test_fit_under_graph_capture_is_reproducible(gpu_ctx):
    """Three steps of eg_model_fit (the launch sequence is captured on its second run and replayed on the third): a second
    model that starts from the same parameters ends with the same bits."""
    G, I, J, K = 5, 33, 20, 17
    graphs = bp.batched_training(G, I, J, K)
    rng = np.random.default_rng(5)
    labels = u(rng, 3 * G, I, J)
    results = []
    for _ in range(2):
        m = egm.compile(*graphs(), gpu=gpu_ctx)
        init = np.random.default_rng(6)
        for tid in sorted(m.params.ids()):
            m.params[tid] = u(init, *m.params[tid].shape)
        m.fit("fit", {"labels": labels}, batch_size=G)
        assert debug_toggles_active() or m.launch_plan("fit").count("eg_bgemm") == 3
        results.append({tid: m.params[tid].copy() for tid in sorted(m.params.ids())})
        m.close()
    for tid in results[0]:
        assert np.all(np.isfinite(results[0][tid]))
        assert np.array_equal(results[0][tid].view(np.uint32), results[1][tid].view(np.uint32)), tid
