"""Wide row groups (rowfuse.hpp, "one wave per sample"): per-sample chains over rows of 65 .. 4096 floats run as one
generated kernel `eg_wrows<i>` in which a wave owns a sample (lane l holds the columns l + 64 j).

The chain of a classification head — softmax.sums, softmax, the loss gradient, softmax's three gradient kernels and the
bias gradient of `dense -> softmax -> crossEntropy` — and a chain of raw `{it}` maps with a column reduction (bias add ->
tanh -> leakyRelu -> mse and its gradients over [B, 300]) are held to the oracle and the float64 shadow with the gates of
tests/parity.py (no tolerance of their own), at widths that are and are not multiples of 64, at the bounds (64: the
thread-per-sample group stays; 4097: no group), on inputs that end exactly where the allocation ends, twice for the same
bits, and on rows holding Inf / NaN / -1e30.

Model.kernel_count(target) is the length of the unfused kernel list; the launches of a plan are the lines of
Model.launch_plan(target).  Up to a batch of 1280 a sample group (one block per sample, formed first) may take the same
chain, as it did before wide groups existed: the plan is asserted at batch 1 and above that limit, parity at every batch."""
import numpy as np
import pytest

import refcases
from conftest import debug_toggles_active
from exprgrad_amd import dsl, layers
from exprgrad_amd import model as egm
from exprgrad_amd.dsl import Fun, iters, param
from parity import Trio
from test_gpu_special_values import same_special

pytestmark = pytest.mark.gpu
f32 = np.float32

N_IN, N_HIDDEN = 24, 16
WIDTHS = [65, 100, 257, 1000, 4096]
BATCHES = [1, 7, 300, 4096]
WIDE_BATCHES = (1, 4096)        # batches at which no sample group is formed (plan_groups.cpp form_sample_group)


def softmax_net(n_out):
    return lambda: refcases.dense_softmax_net(N_IN, N_HIDDEN, n_out)


def mse_net(width=300, rate=0.01):
    """[B, width] input + [width] bias -> tanh -> leakyRelu -> mse: a row-local map with a [W] operand, raw `{it}` maps,
    a reduction over everything (the loss) and, in the gradient, a reduction over the batch per column (the bias)."""
    def build():
        y, x = iters("y x")
        inp = dsl.input("x")
        bias = param([width], name="bias")
        biased = Fun()
        biased.name = "biased"
        biased[y, x] += inp[y, x] + bias[x]
        net = layers.leaky_relu(layers.tanh(biased)).target("predict")
        loss = layers.mse(net, dsl.input("t")).target("loss")
        return [loss.backprop(layers.gradient_descent(rate)).target("train")]
    return build


def softmax_data(batch, n_out, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((batch, N_IN), dtype=f32)
    y = np.zeros((batch, n_out), f32)
    y[np.arange(batch), rng.integers(0, n_out, batch)] = 1.0
    return {"x": x, "y": y}


def launches(plan_text):
    return [line for line in plan_text.splitlines() if line.startswith("[")]


def wide_launches(plan_text):
    return [line for line in launches(plan_text) if "eg_wrows" in line]


# ---- 1. fused -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_out", WIDTHS)
def test_the_softmax_chain_is_one_wide_row_group(gpu_ctx, n_out):
    """Fails without the feature: no launch of the plan is an eg_wrows group."""
    m = egm.compile(*softmax_net(n_out)(), gpu=gpu_ctx)
    m.apply("train", softmax_data(2048, n_out, 1))
    plan = m.launch_plan("train")
    if not debug_toggles_active():
        wide = wide_launches(plan)
        assert wide, plan
        assert any("softmax.sums" in line and f"W={n_out} " in line for line in wide), plan
        assert len(launches(plan)) < m.kernel_count("train"), plan
    m.close()


# ---- 2. parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("n_out", WIDTHS)
def test_softmax_chain_parity(gpu_ctx, n_out, batch):
    trio = Trio(gpu_ctx, softmax_net(n_out))
    trio.init_params(np.random.default_rng(n_out + batch))
    data = softmax_data(batch, n_out, n_out * 7 + batch)
    trio.call("predict", {"x": data["x"]}, n=n_out)
    trio.call("loss", data, n=batch * n_out)
    for _ in range(3):
        trio.step("train", data, n=max(batch, n_out))
    if batch in WIDE_BATCHES and not debug_toggles_active():
        assert wide_launches(trio.gpu.launch_plan("train")), trio.gpu.launch_plan("train")
    trio.close()


@pytest.mark.parametrize("batch", BATCHES)
def test_mse_chain_parity(gpu_ctx, batch):
    trio = Trio(gpu_ctx, mse_net())
    trio.init_params(np.random.default_rng(batch))
    rng = np.random.default_rng(1000 + batch)
    data = {"x": (rng.random((batch, 300), dtype=f32) * 4 - 2).astype(f32), "t": rng.random((batch, 300), dtype=f32)}
    pred = trio.call("predict", {"x": data["x"]}, n=1)
    # The oracle adds the loss's batch * 300 terms one after the other in float32: like-signed terms, so its own distance
    # from the exact sum grows with their number (up to n * 2^-25; 6.6e-4 measured at 4096 x 300 dense terms) and the
    # direct gate of 1e-5 cannot be met by the oracle itself.  Beyond 100 000 terms the loss is called on targets that
    # equal the prediction except in 2000 places: the same kernel over the same extent, 2000 non-zero terms.
    loss_data = data
    if batch * 300 > 100000:
        t = np.array(pred, dtype=f32).reshape(batch, 300)
        where = rng.choice(t.size, 2000, replace=False)
        t.flat[where] += rng.random(2000, dtype=f32)
        loss_data = {"x": data["x"], "t": t}
    trio.call("loss", loss_data, n=batch * 300)
    for _ in range(3):
        trio.step("train", data, n=batch)
    if batch in WIDE_BATCHES and not debug_toggles_active():
        plan = trio.gpu.launch_plan("train")
        assert any("W=300 " in line for line in wide_launches(plan)), plan
    trio.close()


# ---- 3. edges -------------------------------------------------------------------------------------------------------------
def test_width_64_keeps_the_thread_per_sample_group(gpu_ctx):
    trio = Trio(gpu_ctx, softmax_net(64))
    trio.init_params(np.random.default_rng(64))
    data = softmax_data(2048, 64, 64)
    trio.step("train", data, n=2048)
    plan = trio.gpu.launch_plan("train")
    if not debug_toggles_active():
        assert not wide_launches(plan), plan
        assert any("row-fused" in line and "wide" not in line for line in launches(plan)), plan
    trio.close()


def test_width_4097_forms_no_wide_group(gpu_ctx):
    trio = Trio(gpu_ctx, softmax_net(4097))
    trio.init_params(np.random.default_rng(4097))
    data = softmax_data(7, 4097, 4097)
    trio.call("predict", {"x": data["x"]}, n=4097)
    trio.step("train", data, n=4097)
    assert not wide_launches(trio.gpu.launch_plan("train")), trio.gpu.launch_plan("train")
    trio.close()


@pytest.mark.parametrize("width", [65, 127])
def test_device_inputs_that_end_at_the_allocation(gpu_ctx, width):
    """The [B, W] input is exactly B * W floats of device memory followed by NaN: lanes beyond the row's end load nothing."""
    import torch
    batch = 1500
    rng = np.random.default_rng(width)
    x = (rng.random((batch, width), dtype=f32) * 4 - 2).astype(f32)
    t = rng.random((batch, width), dtype=f32)

    def run(inputs):
        m = egm.compile(*mse_net(width)(), gpu=gpu_ctx)
        m.params[m.params.ids()[0]] = np.linspace(-0.2, 0.2, width, dtype=f32)
        loss = np.array(m.call("loss", inputs))
        m.apply("train", inputs)
        if not debug_toggles_active():
            assert wide_launches(m.launch_plan("train")), m.launch_plan("train")
        out = (loss, np.array(m.params[m.params.ids()[0]]))
        m.close()
        return out

    held = []

    def on_device(a):
        buf = torch.full((a.size + 4096,), float("nan"), dtype=torch.float32, device="cuda")
        buf[:a.size] = torch.from_numpy(a.ravel()).cuda()
        held.append(buf)
        return buf[:a.size].view(a.shape)

    want_loss, want_bias = run({"x": x, "t": t})
    got_loss, got_bias = run({"x": on_device(x), "t": on_device(t)})
    assert np.all(np.isfinite(got_loss)) and np.all(np.isfinite(got_bias))
    assert np.array_equal(got_loss, want_loss) and np.array_equal(got_bias, want_bias)


# ---- 4. same bits twice ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_out,batch", [(1000, 2048), (257, 4096)])
def test_one_step_twice_gives_the_same_bits(gpu_ctx, n_out, batch):
    data = softmax_data(batch, n_out, 11)
    results = []
    for _ in range(2):
        m = egm.compile(*softmax_net(n_out)(), gpu=gpu_ctx)
        rng = np.random.default_rng(3)
        for tid in m.params.ids():
            m.params[tid] = (rng.random(m.params[tid].shape, dtype=f32) * 0.4 - 0.2).astype(f32)
        m.apply("train", data)
        results.append({tid: np.array(m.params[tid]) for tid in m.params.ids()})
        m.close()
    for tid in results[0]:
        assert np.array_equal(results[0][tid], results[1][tid]), tid


# ---- 5. special values ----------------------------------------------------------------------------------------------------
def test_rows_of_special_values_match_the_oracle(gpu_ctx):
    """softmax is exp(x) / sum(exp(x)) as written (dnn.nim): a row holding +Inf gives Inf / Inf = NaN there and zeros
    elsewhere, a NaN poisons its row, a row of -1e30 is 0 / 0."""
    from oracle import kd
    width = 100

    def graphs():
        net = layers.softmax(dsl.input("x")).target("predict")
        return [layers.cross_entropy(net, dsl.input("y")).target("loss")]

    gpu = egm.compile(*graphs(), gpu=gpu_ctx)
    ref = kd.Model(refcases.program_text(graphs()))
    rng = np.random.default_rng(0)
    x = (rng.random((6, width), dtype=f32) - 0.5).astype(f32)
    x[1, 70] = np.inf
    x[2, 3] = np.nan
    x[3, :] = -1e30
    x[4, 99] = 88.0
    y = np.zeros((6, width), f32)
    y[np.arange(6), [0, 70, 5, 9, 99, 64]] = 1.0
    with np.errstate(all="ignore"):
        want = ref.call("predict", {"x": x})
        want_loss = ref.call("loss", {"x": x, "y": y})
    same_special(gpu.call("predict", {"x": x}), want, "softmax over special rows")
    same_special(gpu.call("loss", {"x": x, "y": y}), want_loss, "cross entropy over special rows")
    if not debug_toggles_active():
        assert wide_launches(gpu.launch_plan("loss")), gpu.launch_plan("loss")
    gpu.close()
