"""Scenarios for tests/test_gpu_replay_changes.py: a small model, a list of steps (call, change, call, ...), and what is read
after every call.  Nothing here needs a GPU to be imported: a scenario is a function of a *session*, and there are two kinds,

    GpuSession      models of exprgrad_amd on a context; every call records the parameters, the caches, the gradient bucket
                    and the random tensors it leaves behind (bit patterns), every `mark` closes a phase (the test counts the graph
                    captures the library reported during it);
    OracleSession   the same steps on the oracle (oracle/kd.py) in float32 and on its float64 shadow, or on the oracle's
                    compile[float64] form for a float64 model; only the final state is compared.

Run as a program (`python tests/replay_cases.py OUT.npz`, in a process started with EG_NO_GRAPH=1) it is the eager twin: every
scenario twice on fresh models, run-to-run bit equality asserted, the first run's records written to OUT.npz.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from exprgrad_amd import dsl, examples, layers  # noqa: E402
from exprgrad_amd.dsl import Fun, iters  # noqa: E402

F32, F64 = np.float32, np.float64
SENTINEL = -12345.5          # what an unbound bucket is filled with (exact in float32 and float64)


# ---- the colliding pair --------------------------------------------------------------------------------------------------
def colliding_pair(start=0.1234567):
    """Two float32 scales that differ as floats and print alike with six significant digits (`%g`, ostream's default): the
    float nearest `start` and the first float above it whose text is still the same, at least four ulps away so that a
    gradient scaled by one differs from a gradient scaled by the other in most of its elements."""
    a = np.float32(start)
    b = a
    for _ in range(4):
        b = np.nextafter(b, np.float32(np.inf), dtype=np.float32)
    assert "%g" % float(a) == "%g" % float(b) and a != b, (a, b)
    return float(a), float(b)


# ---- models --------------------------------------------------------------------------------------------------------------
def softmax_net(optim="sgd", n_in=24, n_hidden=32, n_out=8):
    """refcases.dense_softmax_net at 24 -> 32 -> 8; with adam, the same layers under layers.adam."""
    if optim == "sgd":
        return examples.dense_softmax_net(n_in, n_hidden, n_out, rate=0.05)
    net = layers.relu(layers.dense(dsl.input("x"), n_in, n_hidden))
    net = layers.softmax(layers.dense(net, n_hidden, n_out)).target("predict")
    net = layers.cross_entropy(net, dsl.input("y")).target("loss")
    return [net.backprop(layers.adam(0.01)).target("train")]


def mlp():
    from test_gpu_epilogue import mlp as epilogue_mlp
    return epilogue_mlp(act="relu")


def dropout_mlp(dims=(96, 80, 72, 8)):
    """The dropout net of tests/test_dropout.py is one launch, which is never captured: the same layer (layers.dropout, a
    random tensor redrawn per call) behind the first activation of the MLP of tests/test_gpu_epilogue.py."""
    net = layers.dropout(layers.relu(layers.dense(dsl.input("x"), dims[0], dims[1])), 0.25)
    net = layers.relu(layers.dense(net, dims[1], dims[2]))
    net = layers.dense(net, dims[2], dims[3]).target("predict")
    net = layers.mse(net, dsl.input("y")).target("loss")
    return [net.backprop(layers.gradient_descent(0.05)).target("train")]


def epoch_slab_net(n=24, h=32, k=8):
    """`r[b, i] ++= x[epoch() mod shape, b, i]`: the epoch picks one slab of the input — a host value, fixed when a plan is made
    (kd::Program::epoch_in_setup: plans are keyed by the epoch, those of other epochs are released) — in front of a dense
    net, so that the range has several launches."""
    x = dsl.input("x")
    b, i = iters("b i")
    r = Fun()
    r[b, i] += x[dsl.epoch() % x.shape[0], b, i]
    r.with_shape(x.shape[1], x.shape[2])
    net = layers.sigmoid(layers.dense(layers.tanh(layers.dense(r, n, h)), h, k)).target("predict")
    return [layers.mse(net, dsl.input("y")).target("loss").backprop(layers.gradient_descent(0.05)).target("train")]


def onehot(rng, rows, classes, dtype):
    return np.eye(classes, dtype=dtype)[rng.integers(0, classes, rows)]


def _dense_data(n_in, n_out):
    def make(rng, rows, dtype):
        return {"x": rng.random((rows, n_in)).astype(dtype), "y": onehot(rng, rows, n_out, dtype)}
    return make


def _mlp_data(rng, rows, dtype):
    return {"x": (rng.random((rows, 96)) - 0.5).astype(dtype), "y": rng.random((rows, 8)).astype(dtype)}


def _pool_data(rng, rows, dtype):
    return {"x": rng.random((rows, 36)).astype(dtype), "y": rng.random((rows, 2, 2, 2)).astype(dtype)}


def _fashion_data(rng, rows, dtype):
    return {"x": rng.random((rows, 144)).astype(dtype), "y": onehot(rng, rows, 10, dtype)}


def _slab_data(rng, rows, dtype):
    return {"x": rng.random((3, rows, 24)).astype(dtype), "y": rng.random((rows, 8)).astype(dtype)}


# key -> (graphs, scalar type, data maker, training target)
MODELS = {
    "softmax_sgd": (lambda: softmax_net("sgd"), F32, _dense_data(24, 8), "train"),
    "softmax_adam": (lambda: softmax_net("adam"), F32, _dense_data(24, 8), "train"),
    "softmax_sgd64": (lambda: softmax_net("sgd"), F64, _dense_data(24, 8), "train"),
    "softmax_wide": (lambda: softmax_net("sgd", 48, 64, 8), F32, _dense_data(48, 8), "train"),
    "mlp": (mlp, F32, _mlp_data, "train"),
    "dropout_mlp": (dropout_mlp, F32, _mlp_data, "train"),
    "pool_adam": (lambda: examples.pool_chain_adam(), F32, _pool_data, "fit"),
    "fashion": (lambda: examples.fashion_mnist_net(size=12, f1=4, f2=8, eta=0.02), F32, _fashion_data, "fit"),
    "epoch_slab": (epoch_slab_net, F32, _slab_data, "train"),
}


def program_text(key):
    graphs, dtype = MODELS[key][0], MODELS[key][1]
    prog = dsl.to_program(*graphs())
    if dtype == F64:
        prog.scalar = "f64"
    return prog.to_text()


def data(key, rows, seed=1):
    return MODELS[key][2](np.random.default_rng(seed), rows, MODELS[key][1])


def start_values(shapes, dtype, seed):
    """The parameters every side starts from: uniform in (-0.3, 0.3), drawn in tensor-id order."""
    rng = np.random.default_rng(1000 + seed)
    return {tid: ((rng.random(tuple(shapes[tid])) * 0.6) - 0.3).astype(dtype) for tid in sorted(shapes)}


# ---- scenario 6: shapes chosen with the planner ---------------------------------------------------------------------------
WS_BATCH = 497           # the smallest batch at which the first layer's weight gradient of softmax_sgd runs in k-slices
WS_MODEL_FLOATS = 3200   # ... and the workspace its slices need; tests/test_replay_cases_cpu.py holds both to the planner


def weight_gradient_case(batch, n_in=24, n_hidden=32):
    """The first dense layer's weight gradient with the bias gradient as its row of ones (run.cpp: sgemm_ones_row), as a line
    for tests/gemm_plan_driver.cpp: x^T [n_in, batch] times the hidden gradient [batch, n_hidden]."""
    return dict(mode="ones", M=n_in, N=n_hidden, K=batch, ta=1, tb=0, lda=n_in, ldb=n_hidden, ldc=n_hidden, a=1, b=1, c=1, bias=0, vec=0,
                switches="-")


def stranger_case():
    """A k-sliced eg_sgemm from tests/golden/gemm_routes.json whose workspace is far beyond the model's: the smallest such
    problem of the table (no switches, no bias; `b` == 2: its B operand is not 16-byte aligned)."""
    with open(os.path.join(ROOT, "tests", "golden", "gemm_routes.json")) as f:
        cases = json.load(f)["cases"]
    ok = [c for c in cases if c["mode"] == "exact" and c["switches"] == "-" and c["bias"] == 0 and int(c["expect"].get("splits", 1)) > 1 and
          int(c["expect"].get("workspace_floats", 0)) >= 16 * WS_MODEL_FLOATS and (c["a"], c["c"]) == (1, 1)]
    return min(ok, key=lambda c: (c["M"] * c["K"] + c["K"] * c["N"] + c["M"] * c["N"], c["M"], c["N"]))


# ---- device-resident inputs ----------------------------------------------------------------------------------------------
class Resident:
    """An input that lives on the device (anything with data_ptr() and shape is borrowed by Model._bind); the oracle reads
    the host copy."""

    def __init__(self, arr, ctx=None):
        self.host = np.array(arr)
        self.shape = tuple(self.host.shape)
        self.dtype = self.host.dtype.name
        self.buf = None
        if ctx is not None:
            self.buf = ctx.allocBuffer(self.host.nbytes)
            self.buf.write(self.host)

    def data_ptr(self):
        return self.buf.ptr

    def write(self, arr):       # contents changed in place (blocking, on the context's stream)
        self.host[...] = arr
        if self.buf is not None:
            self.buf.write(self.host)


def _host(inputs):
    return {k: (v.host if isinstance(v, Resident) else v) for k, v in inputs.items()}


# ---- GPU side ------------------------------------------------------------------------------------------------------------
class GpuModel:
    def __init__(self, session, index, key, seed, ctx):
        from exprgrad_amd import model as egm
        self.s, self.index, self.key, self.ctx = session, index, key, ctx
        graphs, self.dtype, _, self.target = MODELS[key]
        self.m = egm.compile(*graphs(), gpu=ctx, dtype=self.dtype)
        self.calls = 0
        self.set_params(seed)
        self.m.epoch = 1            # (adam divides by 1 - beta^epoch)
        self.random_ids = [i for i, t in enumerate(self.m.program.tensors, 1) if t["kind"] == "random"]

    # -- what a call leaves behind
    def _record(self, masks=None):
        tag = "%d.%02d." % (self.index, self.calls)
        self.calls += 1
        out = self.s.out
        for tid in self.m.params.ids():
            out[tag + "p%d" % tid] = np.array(self.m.params[tid])
        for tid in self.m.caches.ids():
            out[tag + "c%d" % tid] = np.array(self.m.caches[tid])
        b = self.bucket()
        if b is not None:
            out[tag + "bucket"] = b
        for rid in masks or ():
            out[tag + "mask%d" % rid] = np.array(self.m.read_tensor(self.target, rid))

    def bucket(self):
        """The gradient bucket wherever it lives now, read through the context's stream."""
        from exprgrad_amd.runtime import GpuBuffer
        ptr, count = self.m.grad_bucket(self.target)
        if not ptr or count <= 0:
            return None
        buf = GpuBuffer(self.ctx, count * np.dtype(self.dtype).itemsize, wrap_ptr=ptr)
        got = buf.read(self.dtype)
        buf.dealloc()           # (a wrapped block is not freed)
        return got

    # -- calls
    def apply(self, inputs, target=None):
        self.m.apply(target or self.target, inputs)
        self._record(masks=self.random_ids)

    def backward(self, inputs):
        self.m.run_backward(self.target, inputs)
        self._record()

    def update(self):
        self.m.run_update(self.target)
        self._record()

    def fit(self, inputs, batch):
        self.m.fit(self.target, inputs, batch_size=batch)
        self._record()

    # -- changes
    def scale(self, s):
        self.m.set_grad_scale(s)

    def epoch(self, e):
        self.m.epoch = e

    def set_params(self, seed):
        for tid, v in start_values(self.m._param_shapes, self.dtype, seed).items():
            self.m.params[tid] = v

    def save(self):
        return self.m.state_bytes()

    def load(self, state):
        self.m.load_state(state)

    def keep_values(self, on):
        self.m.keep_values(on)

    def seed(self, s):
        self.m.set_seed(s)

    def dev(self, arr):
        r = Resident(arr, self.ctx)
        self.s.keep.append(r)       # user-owned buffers live until the scenario ends
        return r

    def bind_bucket(self):
        """A torch tensor filled with the sentinel becomes the gradient bucket."""
        import torch
        _, count = self.m.grad_bucket(self.target)
        t = torch.full((count,), SENTINEL, dtype=torch.float64 if self.dtype == F64 else torch.float32, device="cuda")
        torch.cuda.synchronize()
        self.s.keep.append(t)
        self.m.bind_grad_bucket(self.target, t)
        return t

    def refill(self, bucket):
        """The bucket that was just unbound gets the sentinel again: nothing may write to it from here on."""
        import torch
        self.ctx.sync()
        bucket.fill_(SENTINEL)
        torch.cuda.synchronize()

    def bucket_is(self, bucket):
        """The gradients of the last backward live in `bucket` (the bound torch tensor), bit for bit."""
        import torch
        self.ctx.sync()
        torch.cuda.synchronize()
        assert same_bits(bucket.cpu().numpy(), self.bucket()), "the bound bucket does not hold the gradients"

    def untouched(self, bucket):
        import torch
        self.ctx.sync()
        torch.cuda.synchronize()
        assert bool((bucket == SENTINEL).all().item()), "an unbound bucket was written to"

    def expect_plan(self, *words):
        if self.s.check_plans:
            plan = self.m.launch_plan(self.target)
            for w in words:
                assert w in plan, (w, plan)

    def final(self):
        st = {"p%d" % tid: np.array(self.m.params[tid]) for tid in self.m.params.ids()}
        st.update({"c%d" % tid: np.array(self.m.caches[tid]) for tid in self.m.caches.ids()})
        return st

    def close(self):
        self.m.close()


class GpuSession:
    def __init__(self, ctx, mark=None, twin=False):
        self.ctx, self.out, self.keep, self.models, self.contexts = ctx, {}, [], [], []
        self._mark = mark
        self.phases = []
        self.check_plans = not twin     # (the words a test looks for in a launch plan are the graph run's)

    def model(self, key, seed=0, ctx=None):
        m = GpuModel(self, len(self.models), key, seed, ctx or self.ctx)
        self.models.append(m)
        return m

    def context(self):
        """A context of its own (its scratch blocks start empty)."""
        import exprgrad_amd as eg
        c = eg.newGpuContext(self.ctx.device)
        self.contexts.append(c)
        return c

    def stranger(self, ctx):
        """A library call on the same context that needs a larger workspace than any model step here."""
        from exprgrad_amd import ops
        c = stranger_case()
        M, N, K = c["M"], c["N"], c["K"]
        rng = np.random.default_rng(3)
        skew = 1 if c["b"] == 2 else 0      # (floats in front of B)
        a, b, out = ctx.allocTensor((M * K,)), ctx.allocTensor((K * N + skew,)), ctx.allocTensor((M * N,))
        a.write(rng.random((M * K,), dtype=F32))
        b.write(rng.random((K * N + skew,), dtype=F32))
        self.keep += [a, b, out]
        ops.sgemm(ctx, M, N, K, a, c["lda"], b.ptr + 4 * skew, c["ldb"], out, c["ldc"], trans_a=bool(c["ta"]), trans_b=bool(c["tb"]))
        ctx.sync()

    def mark(self, label, expect=None):
        """Ends a phase.  expect: "capture" (the phase must have captured a graph), "none" (it must not), None."""
        n = self._mark() if self._mark else (0, 0)
        self.phases.append((label, expect, n[0], n[1]))

    def close(self):
        for m in self.models:
            m.close()
        for c in self.contexts:
            c.close()
        self.keep = []


# ---- oracle side ---------------------------------------------------------------------------------------------------------
class OracleModel:
    def __init__(self, key, seed, index=0, masks=None):
        from oracle import kd
        self.key, self.index, self.calls, self.masks = key, index, 0, masks or {}
        _, self.dtype, _, self.target = MODELS[key]
        text = program_text(key)
        self.ref = kd.Model(text, threads=4)
        self.sides = [self.ref] if self.dtype == F64 else [self.ref, kd.Model(text, shadow=True)]
        self.s_now = 1.0
        self.set_params(seed)
        self.epoch(1)

    def _next_call(self):
        """The random tensors of this call are the ones the GPU drew for it (the reference draws from Nim's global generator:
        nothing to pin bit for bit)."""
        tag = "%d.%02d.mask" % (self.index, self.calls)
        self.calls += 1
        for k, v in self.masks.items():
            if k.startswith(tag):
                for m in self.sides:
                    m.random_override[int(k[len(tag):])] = v

    def apply(self, inputs, target=None):
        self._next_call()
        for m in self.sides:
            m.run_backward(target or self.target, _host(inputs), grad_scale=self.s_now)
            m.run_update(target or self.target)

    def backward(self, inputs):
        self._next_call()
        for m in self.sides:
            m.run_backward(self.target, _host(inputs), grad_scale=self.s_now)

    def update(self):
        self._next_call()
        for m in self.sides:
            m.run_update(self.target)

    def fit(self, inputs, batch):
        self._next_call()
        inputs = _host(inputs)
        rows = next(iter(inputs.values())).shape[0]
        for m in self.sides:
            m.epoch += 1
            for b in range(rows // batch):
                m.run_backward(self.target, {k: v[b * batch:(b + 1) * batch] for k, v in inputs.items()}, grad_scale=self.s_now)
                m.run_update(self.target)

    def scale(self, s):
        self.s_now = float(np.float32(s))

    def epoch(self, e):
        for m in self.sides:
            m.epoch = e

    def set_params(self, seed):
        shapes = {tid: p.shape for tid, p in self.ref.params.items()}
        for tid, v in start_values(shapes, F64 if self.dtype == F64 else F32, seed).items():
            for m in self.sides:
                m.params[tid][...] = v

    def save(self):
        return [({t: p.copy() for t, p in m.params.items()}, {t: c.copy() for t, c in m.caches.items()}) for m in self.sides]

    def load(self, state):
        for m, (params, caches) in zip(self.sides, state):
            for t, p in params.items():
                m.params[t][...] = p
            for t, c in caches.items():
                m.caches[t][...] = c

    def dev(self, arr):
        return Resident(arr)

    def keep_values(self, on):
        pass

    def seed(self, s):
        pass

    def bind_bucket(self):
        return None

    def refill(self, bucket):
        pass

    def bucket_is(self, bucket):
        pass

    def untouched(self, bucket):
        pass

    def expect_plan(self, *words):
        pass

    def final(self):
        """[(name, oracle value, exact value or None)]"""
        exact = self.sides[1] if len(self.sides) > 1 else None
        st = [("p%d" % t, np.asarray(p), np.asarray(exact.params[t]) if exact else None) for t, p in sorted(self.ref.params.items())]
        st += [("c%d" % t, np.asarray(c), np.asarray(exact.caches[t]) if exact else None) for t, c in sorted(self.ref.caches.items())]
        return st


class OracleSession:
    gpu = False

    def __init__(self, masks=None):
        self.models, self.masks = [], masks

    def model(self, key, seed=0, ctx=None):
        self.models.append(OracleModel(key, seed, len(self.models), self.masks))
        return self.models[-1]

    def context(self):
        return None

    def stranger(self, ctx):
        pass

    def mark(self, label, expect=None):
        pass


# ---- the scenarios -------------------------------------------------------------------------------------------------------
# Every scenario: name -> (steps, environment, how the oracle is asked).  `steps(S)` is the whole sequence.
def _times(n, fn, *a):
    for _ in range(n):
        fn(*a)


def _scale_steps(key, how, pair):
    """1.0 -> 0.25 -> 1.0, or the colliding pair p0 -> p1 -> p0: three calls, three calls, two calls."""
    def steps(S):
        d = S.model(key)
        inputs = data(key, 64)
        p0, p1 = colliding_pair()
        seq = [(p0, 3), (p1, 3), (p0, 2)] if pair else [(1.0, 3), (0.25, 3), (1.0, 2)]
        if how == "fit":
            inputs = data(key, 8 * 12)      # two single batches, two groups of five (EG_FIT_GROUP=5)
            seq = [(s, 2) for s, _ in seq]
        for s, n in seq:
            d.scale(s)
            for _ in range(n):
                if how == "apply":
                    d.apply(inputs)
                elif how == "split":
                    d.backward(inputs)
                    d.update()
                else:
                    d.epoch(0)              # (fit bumps the epoch, which is part of every graph's key: hold it still)
                    d.fit(inputs, 8)
            S.mark("scale %r" % s, "capture")
        if pair:
            # the precondition on the reference: from one state, one step with p0 and one with p1 differ in bits
            for s in (p0, p1):
                probe = S.model(key)
                probe.scale(s)
                probe.backward(data(key, 64))
    return steps


def epoch_kernel_argument(S):
    d = S.model("softmax_adam")
    inputs = data("softmax_adam", 64)
    for e, n in ((1, 3), (2, 3), (1, 2)):
        d.epoch(e)
        _times(n, d.apply, inputs)
        S.mark("epoch %d" % e, "capture")


def epoch_kernel_argument_pool(S):
    """pool_chain_adam.kd: epoch() next to computed indices (y div 2 of the pooling gradient)."""
    d = S.model("pool_adam")
    inputs = data("pool_adam", 8)
    for e, n in ((1, 3), (2, 3), (1, 2)):
        d.epoch(e)
        _times(n, d.apply, inputs)
        S.mark("epoch %d" % e, "capture")


def epoch_host_value(S):
    d = S.model("epoch_slab")
    inputs = data("epoch_slab", 64)
    for e, n in ((1, 3), (2, 3), (1, 2)):
        d.epoch(e)
        _times(n, d.apply, inputs)
        S.mark("epoch %d" % e, "capture")   # a plan of its own per epoch; the one of epoch 1 was released and is rebuilt


def pointer_device(S):
    d = S.model("softmax_sgd")
    one, two = data("softmax_sgd", 64, seed=1), data("softmax_sgd", 64, seed=2)
    a = {k: d.dev(v) for k, v in one.items()}
    b = {k: d.dev(v) for k, v in two.items()}
    for name, bound, n in (("a", a, 3), ("b", b, 3), ("a again", a, 2)):
        _times(n, d.apply, bound)
        S.mark(name, "capture")
    for step in range(3):                   # the contents of a change in place between replays
        fresh = data("softmax_sgd", 64, seed=10 + step)
        for k in a:
            a[k].write(fresh[k])
        d.apply(a)
    S.mark("a rewritten in place", "none")


def pointer_host(S):
    d = S.model("softmax_sgd")
    _times(3, d.apply, data("softmax_sgd", 64, seed=1))
    S.mark("host arrays", "capture")
    for step in range(3):                   # new values on every call; the staging buffers stay where they are
        d.apply(data("softmax_sgd", 64, seed=20 + step))
    S.mark("new values", "none")


def _shape_steps(key, device):
    def steps(S):
        d = S.model(key)
        small, large = data(key, 64, seed=1), data(key, 200, seed=2)
        if device:
            small = {k: d.dev(v) for k, v in small.items()}
            large = {k: d.dev(v) for k, v in large.items()}
        _times(3, d.apply, small)
        S.mark("batch 64", "capture")
        _times(3, d.apply, large)
        S.mark("batch 200", "capture")
        _times(2, d.apply, small)
        # host arrays: the staging buffers were regrown for 200 rows, the first plan's graph names freed memory and must be
        # captured again; device tensors: the first plan's graph still names live tensors and is right as it stands
        S.mark("batch 64 again", "none" if device else "capture")
    return steps


def scratch_grown_by_a_stranger(S):
    ctx = S.context()
    d = S.model("softmax_sgd", ctx=ctx)
    inputs = data("softmax_sgd", WS_BATCH)
    _times(3, d.apply, inputs)
    d.expect_plan("gemm TN 24x32x%d" % WS_BATCH)
    S.mark("the model's own workspace", "capture")
    S.stranger(ctx)
    _times(3, d.apply, inputs)
    S.mark("after the stranger grew it", "capture")


def scratch_two_models(S):
    ctx = S.context()
    small, large = S.model("softmax_sgd", ctx=ctx), S.model("softmax_wide", seed=1, ctx=ctx)
    xs, xl = data("softmax_sgd", WS_BATCH), data("softmax_wide", 4 * WS_BATCH)
    _times(3, small.apply, xs)
    S.mark("small alone", "capture")
    _times(3, large.apply, xl)
    S.mark("large grows the workspace", "capture")
    _times(3, small.apply, xs)
    S.mark("small again", "capture")
    for _ in range(2):
        large.apply(xl)
        small.apply(xs)
    S.mark("alternating", "none")


def gradient_bucket(S):
    d = S.model("softmax_sgd")
    inputs = data("softmax_sgd", 64)

    def rounds(n):
        for _ in range(n):
            d.backward(inputs)
            d.update()
    rounds(3)
    S.mark("the library's bucket", "capture")
    first = d.bind_bucket()
    rounds(3)
    d.bucket_is(first)
    S.mark("a torch bucket", "capture")
    second = d.bind_bucket()
    d.refill(first)
    rounds(3)
    d.bucket_is(second)
    d.untouched(first)
    S.mark("another torch bucket", "capture")


def _keep_values_steps(toggle):
    def steps(S):
        d = S.model("mlp")
        inputs = data("mlp", 200)
        # a plan of its own while the values are kept; back off, the first plan and its graph serve again
        for on, expect in ((False, "capture"), (True, "capture"), (False, "none")):
            if toggle:
                d.keep_values(on)
            _times(3, d.apply, inputs)
            S.mark("keep_values %s" % on, expect if toggle else None)
    return steps


def params_rewritten(S):
    d = S.model("softmax_sgd")
    inputs = data("softmax_sgd", 64)
    _times(3, d.apply, inputs)
    S.mark("first parameters", "capture")
    d.set_params(7)
    _times(3, d.apply, inputs)
    S.mark("params[tid] = ...", "none")


def state_reloaded(S):
    d = S.model("softmax_adam")
    inputs = data("softmax_adam", 64)
    d.epoch(1)
    _times(3, d.apply, inputs)
    state = d.save()
    S.mark("calls 0 to 2", "capture")
    _times(3, d.apply, inputs)
    d.load(state)
    _times(3, d.apply, inputs)              # calls 6 to 8 repeat calls 3 to 5
    S.mark("calls 3 to 8 around load_state", "none")


def seed_between_replays(S):
    d = S.model("dropout_mlp")
    inputs = data("dropout_mlp", 64)
    d.seed(5)
    _times(3, d.apply, inputs)
    S.mark("seed 5", "capture")
    d.seed(99)
    d.set_params(0)                         # (back to the start, so that the calls can be held to a fresh model's)
    _times(3, d.apply, inputs)
    S.mark("seed 99", "none")
    fresh = S.model("dropout_mlp")
    fresh.seed(99)
    _times(3, fresh.apply, inputs)
    S.mark("a fresh model with seed 99", "capture")


def _fit_apply_steps(key):
    def steps(S):
        d = S.model(key)
        d.epoch(0)
        d.fit(data(key, 8 * 12, seed=1), 8)       # two single batches, two groups of five
        S.mark("fit, 96 rows", "capture")
        one = data(key, 8, seed=2)
        _times(3, d.apply, one)
        S.mark("three applies", None)
        d.fit(data(key, 8 * 17, seed=3), 8)       # another row count: the data set's device copy is regrown
        S.mark("fit, 136 rows", "capture")
        d.apply(one)
        S.mark("apply", None)
    return steps


FIT_ENV = {"EG_FIT_GROUP": "5"}
MLP_ENV = {"EG_EPILOGUE_MIN_ELEMS": "0"}

# name -> (steps, environment, oracle: "state" = final parameters and caches; None = the twin alone)
SCENARIOS = {
    "scale_apply": (_scale_steps("softmax_sgd", "apply", False), {}, "state"),
    "scale_apply_adam": (_scale_steps("softmax_adam", "apply", False), {}, "state"),
    "scale_split": (_scale_steps("softmax_sgd", "split", False), {}, "state"),
    "scale_f64": (_scale_steps("softmax_sgd64", "apply", False), {}, "state"),
    "scale_fit": (_scale_steps("softmax_sgd", "fit", False), FIT_ENV, "state"),
    "scale_mlp": (_scale_steps("mlp", "apply", False), MLP_ENV, "state"),
    "scale_pair_apply": (_scale_steps("softmax_sgd", "apply", True), {}, "state"),
    "scale_pair_split": (_scale_steps("softmax_sgd", "split", True), {}, "state"),
    "scale_pair_f64": (_scale_steps("softmax_sgd64", "apply", True), {}, "state"),
    "scale_pair_fit": (_scale_steps("softmax_sgd", "fit", True), FIT_ENV, "state"),
    "epoch_kernel_argument": (epoch_kernel_argument, {}, "state"),
    "epoch_kernel_argument_pool": (epoch_kernel_argument_pool, {}, "state"),
    "epoch_host_value": (epoch_host_value, {}, "state"),
    "pointer_device": (pointer_device, {}, "state"),
    "pointer_host": (pointer_host, {}, "state"),
    "shape_host": (_shape_steps("softmax_sgd", False), {}, "state"),
    "shape_device": (_shape_steps("softmax_sgd", True), {}, "state"),
    "shape_adam": (_shape_steps("softmax_adam", False), {}, "state"),
    "shape_f64": (_shape_steps("softmax_sgd64", False), {}, "state"),
    "scratch_stranger": (scratch_grown_by_a_stranger, {}, "state"),
    "scratch_two_models": (scratch_two_models, {}, "state"),
    "gradient_bucket": (gradient_bucket, {}, "state"),
    "keep_values": (_keep_values_steps(True), MLP_ENV, "state"),
    "keep_values_never": (_keep_values_steps(False), MLP_ENV, None),
    "params_rewritten": (params_rewritten, {}, "state"),
    "state_reloaded": (state_reloaded, {}, "state"),
    "seed_between_replays": (seed_between_replays, {}, "state"),
    "fit_apply_fashion": (_fit_apply_steps("fashion"), FIT_ENV, "state"),
    "fit_apply_dense": (_fit_apply_steps("softmax_sgd"), FIT_ENV, "state"),
}
PAIRS = [n for n in SCENARIOS if n.startswith("scale_pair_")]


def run_on_gpu(name, ctx, mark=None, twin=False):
    """One scenario on fresh models: the session (records in .out, phases in .phases), closed."""
    S = GpuSession(ctx, mark, twin)
    try:
        SCENARIOS[name][0](S)
        S.finals = [m.final() for m in S.models]
    finally:
        S.close()
    return S


def run_on_oracle(name, masks=None):
    """masks: the records of the GPU run (the random tensors it drew, call by call)."""
    S = OracleSession(masks)
    SCENARIOS[name][0](S)
    return S


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def probes_differ(out):
    """The two one-step probes of a pair scenario (models 1 and 2) left different gradient bits."""
    return not same_bits(out["1.00.bucket"], out["2.00.bucket"])


# ---- the eager twin ------------------------------------------------------------------------------------------------------
def main(path):
    import time
    import exprgrad_amd as eg
    from exprgrad_amd import _lib
    assert os.environ.get("EG_NO_GRAPH") == "1", "the twin issues every launch by itself"
    ctx = eg.newGpuContext(0)
    records, unstable = {}, []
    for name, (_, env, _) in SCENARIOS.items():
        t0 = time.time()
        for k, v in env.items():
            os.environ[k] = v
        _lib.reload_switches()
        try:
            first = run_on_gpu(name, ctx, twin=True).out
            again = run_on_gpu(name, ctx, twin=True).out
        finally:
            for k in env:
                del os.environ[k]
            _lib.reload_switches()
        assert sorted(first) == sorted(again), name
        differ = [k for k in first if not same_bits(first[k], again[k])]
        if differ:
            unstable.append(name)
            print("NOT-REPRODUCIBLE", name, differ[:8], flush=True)
        if name in PAIRS:
            assert probes_differ(first), (name, "the reference does not tell the two scales apart")
        for k, v in first.items():
            records[name + "|" + k] = v
        print("twin %-28s %5.2f s  %d records" % (name, time.time() - t0, len(first)), flush=True)
    records["unstable"] = np.array(unstable, dtype="U64")
    np.savez(path, **records)
    print("TWIN-OK")


if __name__ == "__main__":
    main(sys.argv[1])
