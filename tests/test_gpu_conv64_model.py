"""The float64 model route of convolutions that the band and direct kernels decline: conv2 (24 -> 20 channels, 3 x 3) -> relu
-> conv2 (20 -> 18, 3 x 3) -> mse -> gradientDescent on 12 x 12 images, batch 3 and the unbatched rank-3 form, against the
oracle's interpreter over double; the launch list names the implicit-GEMM kernels (csrc/kernels/conv2_f64_mfma.hip); the
same step with EG_CONV_NO_MFMA64=1 (the generated kernels) in a child process; and fit and apply steps through captured
graphs against the same steps issued launch by launch, bit for bit (the filter gradient's slabs and the image gradient's flipped bank live in the
context's scratch, sized by the eager run in front of the capture)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from exprgrad_amd import dsl, layers
from exprgrad_amd import model as egm
from exprgrad_amd.dsl import Fun, iters, param

pytestmark = pytest.mark.gpu
TOL64 = 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("eg_conv64_mfma_fwd", "eg_conv64_mfma_gimg", "eg_conv64_mfma_gflt")


def rel(got, want):
    want = np.asarray(want, np.float64)
    scale = max(float(np.max(np.abs(want))) if want.size else 0.0, 1e-300)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want))) / scale if want.size else 0.0


def conv3(image, chans, w, h, nfilters):
    """conv2 without a batch index (benchmarks/conv2/conv2.nim:128-132) with its filter bank as a parameter."""
    y, x, f, c, dy, dx = iters("y x filter chan dy dx")
    filters = param([nfilters, h, w, chans], name="filters")
    r = Fun()
    r[y, x, f] += image[y + dy, x + dx, c] * filters[f, dy, dx, c]
    return r


def net(batched, rate=0.05):
    conv = layers.conv2 if batched else conv3
    hidden = layers.relu(conv(dsl.input("x"), 24, 3, 3, 20))
    out = conv(hidden, 20, 3, 3, 18).target("predict")
    return [layers.mse(out, dsl.input("y")).target("loss").backprop(layers.gradient_descent(rate)).target("train")]


def text64(graphs):
    prog = dsl.to_program(*graphs)
    prog.scalar = "f64"
    return prog.to_text()


def data(batched, seed=5):
    rng = np.random.default_rng(seed)
    lead = (3,) if batched else ()
    return rng, rng.uniform(-1, 1, lead + (12, 12, 24)), rng.uniform(-1, 1, lead + (8, 8, 18))


def step_against_the_oracle(gpu_ctx, batched):
    from oracle import kd
    gpu = egm.compile(*net(batched), gpu=gpu_ctx, dtype=np.float64)
    ref = kd.Model(text64(net(batched)))
    rng, x, y = data(batched)
    for tid in sorted(ref.params):
        v = rng.uniform(-0.3, 0.3, ref.params[tid].shape)
        ref.params[tid][...] = v
        gpu.params[tid] = v
    worst = rel(gpu.call("loss", {"x": x, "y": y}), ref.call("loss", {"x": x, "y": y}))
    gpu.apply("train", {"x": x, "y": y})
    ref.apply("train", {"x": x, "y": y})
    for tid in sorted(ref.params):
        worst = max(worst, rel(gpu.params[tid], ref.params[tid]))
    plan = gpu.launch_plan("train")
    gpu.close()
    return worst, plan


@pytest.mark.parametrize("batched", [True, False], ids=["batch-3", "rank-3"])
def test_training_step_against_the_oracle_names_the_kernels(gpu_ctx, batched):
    worst, plan = step_against_the_oracle(gpu_ctx, batched)
    print("worst relative error", worst)
    assert worst <= TOL64
    for name in KERNELS:
        assert name in plan, (name, plan)


CHILD = """
import sys
import numpy as np
sys.path.insert(0, {tests!r})
import exprgrad_amd as eg
import test_gpu_conv64_model as t
ctx = eg.newGpuContext(0)
for batched in (True, False):
    worst, plan = t.step_against_the_oracle(ctx, batched)
    assert not any(k in plan for k in t.KERNELS), plan
    print("worst", batched, worst)
    assert worst <= t.TOL64, worst
print("CHILD-OK")
"""


def test_the_same_step_on_the_generated_kernels():
    """EG_CONV_NO_MFMA64=1 is the parent route; the step runs in a fresh process that starts with the switch set."""
    env = dict(os.environ, EG_CONV_NO_MFMA64="1")
    out = subprocess.run([sys.executable, "-c", CHILD.format(tests=os.path.join(ROOT, "tests"))], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "CHILD-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def fit_sequence(gpu_ctx):
    """Two fit calls of two batches each, then three apply calls on one batch (an eager run, the capture, a replay): the
    parameters afterwards."""
    rng = np.random.default_rng(12)
    x, y = rng.uniform(-1, 1, (6, 12, 12, 24)), rng.uniform(-1, 1, (6, 8, 8, 18))
    m = egm.compile(*net(True, rate=1e-4), gpu=gpu_ctx, dtype=np.float64)   # (mse divides by the batch alone: a small rate keeps 7 steps bounded)
    for tid in sorted(m.params):
        m.params[tid] = rng.uniform(-0.3, 0.3, m.params[tid].shape)
    for _ in range(2):
        m.fit("train", {"x": x, "y": y}, batch_size=3)
    for _ in range(3):
        m.apply("train", {"x": x[:3], "y": y[:3]})
    plan = m.launch_plan("train")
    params = [np.array(m.params[tid]) for tid in sorted(m.params)]
    m.close()
    return params, plan


EAGER_CHILD = """
import sys
import numpy as np
sys.path.insert(0, {tests!r})
import exprgrad_amd as eg
import test_gpu_conv64_model as t
params, plan = t.fit_sequence(eg.newGpuContext(0))
assert all(k in plan for k in t.KERNELS), plan
np.savez({out!r}, *params)
print("CHILD-OK")
"""


def test_steps_through_captured_graphs_equal_eager_steps(gpu_ctx, tmp_path):
    """The same sequence of fit and apply calls here, where launch sequences are captured after one eager run and replayed,
    and in a child process under EG_NO_GRAPH=1, where every launch is issued one by one: the same bits."""
    params, plan = fit_sequence(gpu_ctx)
    for name in KERNELS:
        assert name in plan
    out = str(tmp_path / "eager.npz")
    env = dict(os.environ, EG_NO_GRAPH="1")
    child = subprocess.run([sys.executable, "-c", EAGER_CHILD.format(tests=os.path.join(ROOT, "tests"), out=out)], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=600)
    assert child.returncode == 0 and "CHILD-OK" in child.stdout, child.stdout[-2000:] + child.stderr[-4000:]
    eager = np.load(out)
    assert len(eager.files) == len(params)
    for i, p in enumerate(params):
        assert np.all(np.isfinite(p)), i
        assert np.array_equal(p, eager["arr_%d" % i]), i
