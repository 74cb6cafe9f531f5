"""Wide row groups over collapsed leading axes (csrc/host/rowfuse.hpp, "Collapsed leading axes"): the scale and the softmax
between the two multi-head products — tests/attention_programs.py — run as one generated kernel `eg_wrows<i>` in which a
wave owns a row of the scores [B, H, I, J] taken as [B * H * I, J].

Every case runs three ways (tests/parity.py: backend | oracle | float64 shadow) under that module's own gates — no tolerance
of their own and no allow-list entry; tests/test_attention_oracle_cpu.py holds the oracle itself to 5e-6 on the same shapes.
The plan text shows what ran: one `eg_wrows` line with `rows=` that holds the softmax kernels, no `generated` line for them.
(The statements about the plan hold in the default configuration only: under an `execution` switch such as EG_NO_ROWFUSE=1
the numbers are checked alone.)"""
import numpy as np
import pytest

import attention_programs as ap
import refcases
from conftest import debug_toggles_active
from exprgrad_amd import model as egm
from parity import Trio
from test_gpu_special_values import same_special

pytestmark = pytest.mark.gpu
f32 = np.float32


def u(rng, *shape):
    return (rng.random(shape, dtype=f32) - f32(0.5)).astype(f32)


def launches(model, target):
    return [line for line in model.launch_plan(target).splitlines() if line.startswith("[")]


def collapsed(lines):
    return [line for line in lines if "eg_wrows" in line and "rows=" in line]


def assert_forward_plan(model, rows, width):
    lines = launches(model, "out")
    wide = collapsed(lines)
    assert len(wide) == 1, lines
    assert f" W={width} rows={'x'.join(str(d) for d in rows)} 3 kernels (scaled:map, softmax.sums:rowsum, softmax:map)" in wide[0], lines
    assert f"grid {-(-int(np.prod(rows)) // 256)} x 256" in wide[0], lines
    assert not any("generated" in line for line in lines), lines
    assert len(lines) < model.kernel_count("out"), lines


# ---- 1. forward: parity and plan ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ap.FORWARD_SHAPES)
def test_forward_parity_and_plan(gpu_ctx, shape):
    """Fails without the feature: no launch of the plan is an eg_wrows group with rows=."""
    rng = np.random.default_rng(sum(shape))
    trio = Trio(gpu_ctx, ap.softmax_forward)
    got = trio.call("out", {"s": u(rng, *shape)}, n=shape[-1])
    assert got.shape == shape
    if not debug_toggles_active():
        assert_forward_plan(trio.gpu, shape[:-1], shape[-1])
    trio.close()


def test_rank3_forward_parity_and_plan(gpu_ctx):
    shape = ap.RANK3_SHAPE
    trio = Trio(gpu_ctx, ap.softmax_forward_rank3)
    got = trio.call("out", {"s": u(np.random.default_rng(3), *shape)}, n=shape[-1])
    assert got.shape == shape
    if not debug_toggles_active():
        assert_forward_plan(trio.gpu, shape[:-1], shape[-1])
    trio.close()


# ---- 2. the attention block's training step -------------------------------------------------------------------------------
def test_training_step(gpu_ctx, monkeypatch):
    """scores -> scale -> softmax -> context -> mse -> gradient descent on q, kk, v.  The products stay the eg_bgemm2
    launches they are without row fusion; the softmax's forward kernels and its gradient kernels (two maps and a row sum
    from the softmax, one map from the scale) sit in eg_wrows groups."""
    B, H, I, J, K, D = ap.TRAINING_SHAPE
    rng = np.random.default_rng(2)
    trio = Trio(gpu_ctx, ap.attention_training(*ap.TRAINING_SHAPE))
    trio.init_params(rng, -0.5, 0.5)
    labels = u(rng, B, I, H, D)
    for _ in range(2):
        trio.step("fit", {"labels": labels}, n=B * I * H * D)
    trio.call("out", {}, n=J)
    if not debug_toggles_active():
        lines = launches(trio.gpu, "fit")
        monkeypatch.setenv("EG_NO_ROWFUSE", "1")
        plain = egm.compile(*ap.attention_training(*ap.TRAINING_SHAPE)(), gpu=gpu_ctx)
        plain.apply("fit", {"labels": labels})
        plain_lines = launches(plain, "fit")
        plain.close()
        monkeypatch.delenv("EG_NO_ROWFUSE")
        products = lambda ls: sorted(" ".join(l.split()[1:6]) for l in ls if "eg_bgemm2" in l)
        assert not any("eg_wrows" in l for l in plain_lines), plain_lines
        assert len(products(lines)) == len(products(plain_lines)) >= 5 and products(lines) == products(plain_lines), (lines, plain_lines)
        wide = collapsed(lines)
        assert len(wide) == 2 and all(f" W={J} rows={B}x{H}x{I} " in l for l in wide), lines
        assert "3 kernels (scaled:map, softmax.sums:rowsum, softmax:map)" in wide[0], lines
        assert "4 kernels (" in wide[1] and wide[1].count(":rowsum") == 1 and wide[1].count(":map") == 3, lines
        assert not any("sample-fused" in l for l in lines), lines     # (which took the gradient chain, one block per b, before)
        assert len(lines) < trio.gpu.kernel_count("fit")
    trio.close()


def test_one_step_twice_gives_the_same_bits(gpu_ctx):
    B, H, I, J, K, D = ap.TRAINING_SHAPE
    labels = u(np.random.default_rng(11), B, I, H, D)
    results = []
    for _ in range(2):
        m = egm.compile(*ap.attention_training(*ap.TRAINING_SHAPE)(), gpu=gpu_ctx)
        rng = np.random.default_rng(3)
        for tid in sorted(m.params.ids()):
            m.params[tid] = u(rng, *m.params[tid].shape)
        m.apply("fit", {"labels": labels})
        m.apply("fit", {"labels": labels})
        results.append({tid: np.array(m.params[tid]) for tid in sorted(m.params.ids())})
        m.close()
    for tid in results[0]:
        assert np.array_equal(results[0][tid].view(np.uint32), results[1][tid].view(np.uint32)), tid


def test_fit_under_graph_capture_is_reproducible(gpu_ctx):
    """Three steps of eg_model_fit (the launch sequence is captured on its second run and replayed on the third): a second
    model that starts from the same parameters ends with the same bits."""
    B, H, I, J, K, D = ap.TRAINING_SHAPE
    graphs = ap.attention_training(*ap.TRAINING_SHAPE)
    labels = u(np.random.default_rng(5), 3 * B, I, H, D)
    results = []
    for _ in range(2):
        m = egm.compile(*graphs(), gpu=gpu_ctx)
        init = np.random.default_rng(6)
        start = {}
        for tid in sorted(m.params.ids()):
            start[tid] = u(init, *m.params[tid].shape)
            m.params[tid] = start[tid]
        m.fit("fit", {"labels": labels}, batch_size=B)
        assert debug_toggles_active() or len(collapsed(launches(m, "fit"))) == 2
        results.append({tid: m.params[tid].copy() for tid in sorted(m.params.ids())})
        assert any(not np.array_equal(results[-1][tid], start[tid]) for tid in start)       # the steps did run
        m.close()
    for tid in results[0]:
        assert np.all(np.isfinite(results[0][tid]))
        assert np.array_equal(results[0][tid].view(np.uint32), results[1][tid].view(np.uint32)), tid


# ---- 3. near misses -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ap.NEAR_MISSES))
def test_near_misses_run_and_form_no_collapsed_group(gpu_ctx, name):
    graphs, shapes = ap.NEAR_MISSES[name]
    rng = np.random.default_rng(len(name))
    trio = Trio(gpu_ctx, graphs)
    trio.call("out", {k: u(rng, *shape) for k, shape in sorted(shapes.items())}, n=shapes["s"][-1])
    assert "rows=" not in trio.gpu.launch_plan("out"), trio.gpu.launch_plan("out")
    trio.close()


# ---- 4. edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1, 65), (1, 1, 257, 65)])
def test_device_inputs_that_end_at_the_allocation(gpu_ctx, shape):
    """The scores are exactly R * 65 floats of device memory followed by NaN.  Lanes beyond a row's end read column `lane`
    of their own row; with one row that column lies one float before the edge."""
    import torch
    s = u(np.random.default_rng(65), *shape)

    def run(inputs):
        m = egm.compile(*ap.softmax_forward(), gpu=gpu_ctx)
        out = np.array(m.call("out", inputs))
        if not debug_toggles_active():
            assert collapsed(launches(m, "out")), m.launch_plan("out")
        m.close()
        return out

    buf = torch.full((s.size + 4096,), float("nan"), dtype=torch.float32, device="cuda")
    buf[:s.size] = torch.from_numpy(s.ravel()).cuda()
    want = run({"s": s})
    got = run({"s": buf[:s.size].view(shape)})
    assert np.all(np.isfinite(got)) and np.array_equal(got, want)
    rows = got.reshape(-1, shape[-1]).astype(np.float64).sum(axis=1)
    assert np.max(np.abs(rows - 1.0)) <= 1e-5


def test_rows_of_special_values_match_the_oracle(gpu_ctx):
    """softmax is exp(e) / sum(exp(e)) as written, without the row maximum: a row holding +Inf gives Inf / Inf = NaN there
    and zeros elsewhere, a NaN poisons its row, a row of -1e30 is 0 / 0."""
    from oracle import kd
    shape = (2, 3, 5, 70)
    gpu = egm.compile(*ap.softmax_forward(), gpu=gpu_ctx)
    ref = kd.Model(refcases.program_text(ap.softmax_forward()))
    s = u(np.random.default_rng(0), *shape)
    s[0, 1, 2, 69] = np.inf
    s[0, 2, 0, 3] = np.nan
    s[1, 0, 4, :] = -1e30
    s[1, 2, 1, 64] = 88.0 / ap.SCALE
    s[1, 2, 4, 0] = -np.inf
    with np.errstate(all="ignore"):
        want = ref.call("out", {"s": s})
    same_special(gpu.call("out", {"s": s}), want, "softmax over special rows")
    if not debug_toggles_active():
        assert collapsed(launches(gpu, "out")), gpu.launch_plan("out")
    gpu.close()
