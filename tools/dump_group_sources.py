#!/usr/bin/env python
"""Digests of the generated fusion-group sources, case by case: what a refactor of the kernel generators (csrc/host/rowfuse_*.cpp)
must leave unchanged to the byte.  Identical text is an identical hiprtc input, the same disk-cache key and the same code object.

    tools/dump_group_sources.py [--out DIR] [--only SUBSTRING]          (GPU box; EG_LIB_PATH selects another build)

Every case runs in a fresh child process (each under its own `timeout`; the run stops at the first child that fails): the
child builds ONE model with EG_DUMP_CODE pointing at a fresh directory and EG_NO_KERNEL_CACHE=1 and runs ONE target once,
because every plan is dumped under the same label.  Per case and dumped file one line

    case-name  file  sha256  bytes  kernels=<names found in it>  mfma=<n> gather4=<n>

(mfma: matrix-core instructions in the text; gather4: 4-wide gathers of the convolution members), so that a case that forms
no group of the kind it is listed for is visible.  Two runs of two builds are compared with `diff`."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
FILES = ("eg_plan_kernels.hip", "eg_model_kernels.hip")

SWITCHES = [{"EG_SAMPLE_NO_MFMA": "1"}, {"EG_SAMPLE_NO_STAGE": "1"}, {"EG_SAMPLE_KEEP_BARRIERS": "1"}, {"EG_NO_NARROW_INDEX": "1"},
            {"EG_NO_ROW_DIRECT": "1"}, {"EG_NO_ROW_TAIL": "1"}, {"EG_SAMPLE_STOP": "3", "EG_TUNING": "1"}, {"EG_SAMPLE_TRACE": "1"},
            {"EG_SAMPLE_TRACE": "101"}, {"EG_ROW_TRACE": "1"}]


def cases():
    """(name, net, arguments of the net, batch, environment)"""
    out = []
    for b in (64, 256, 4096):          # single_block, in_kernel_finalize, a row tail with grid_blocks
        out.append(("xor_b%d" % b, "xor", (), b, {}))
        out.append(("dense_b%d" % b, "dense", (784, 512, 10), b, {}))
    # the sample group: forward with and without patches, by-rows filter gradient, T > 1, blocking; behind it a map group (adam)
    for b in (5, 32, 64):              # that folds the sample group's slab
        out.append(("fashion_fit_b%d" % b, "fashion", (28, 8, 16), b, {}))
    for w in (100, 1000, 2500, 4096):  # wide rows (one wave per sample); the widest split their chain over several groups
        out.append(("softmax_w%d_b2048" % w, "dense", (24, 16, w), 2048, {}))
    out.append(("mse_w300_b2048", "mse_wide", (300,), 2048, {}))
    out.append(("small_chain", "small_chain", (), 4, {}))                # a small group (kernels over parameters that are no maps)
    out.append(("xor_adam_b64", "xor_adam", (), 64, {}))                 # a row group and a map group (adam's chains)
    out.append(("pool_chain_adam_fit_b8", "pool_adam", (), 8, {}))       # the same through Model.fit, with a convolution
    # convolutions in the form of tests/test_gpu_fuzz.py build_cnn that take the one-value gathers: channels and filters no
    # multiple of 4; an odd output width; and the fashion_mnist network with 3 and 5 filters
    out.append(("cnn_c3_s12_f2_3x3_b9", "cnn", (3, 12, 2, 3, 3, 5), 9, {}))
    out.append(("cnn_c3_s9_f2_3x3_b9", "cnn", (3, 9, 2, 3, 3, 5), 9, {}))
    out.append(("cnn_c4_s12_f8_2x3_b9", "cnn", (4, 12, 8, 2, 3, 10), 9, {}))
    out.append(("fashion_s14_f3_f5_fit_b8", "fashion", (14, 3, 5), 8, {}))
    for env in SWITCHES:
        tag = "_".join("%s=%s" % kv for kv in sorted(env.items()) if kv[0] != "EG_TUNING")
        out.append(("fashion_fit_b32[%s]" % tag, "fashion", (28, 8, 16), 32, env))
        out.append(("xor_b4096[%s]" % tag, "xor", (), 4096, env))
        out.append(("xor_b64[%s]" % tag, "xor", (), 64, env))
    return out


def child(name):
    sys.path.insert(0, ROOT)
    import numpy as np
    import exprgrad_amd as eg
    from exprgrad_amd import dsl, examples, layers
    from exprgrad_amd import model as egm
    from exprgrad_amd.dsl import Fun, iters, param
    _, net, args, batch, _ = next(c for c in cases() if c[0] == name)
    rng = np.random.default_rng(0)
    f = np.float32

    def onehot(n, classes):
        return np.eye(classes, dtype=f)[rng.integers(0, classes, n)]

    ctx = eg.newGpuContext(0)
    if net == "xor":
        m = egm.compile(*examples.xor_from_scratch(), gpu=ctx)
        m.apply("train", {"x": rng.integers(0, 2, (batch, 2)).astype(f), "y": rng.random((batch, 1), dtype=f)})
    elif net == "dense":
        m = egm.compile(*examples.dense_softmax_net(*args), gpu=ctx)
        m.apply("train", {"x": rng.random((batch, args[0]), dtype=f), "y": onehot(batch, args[2])})
    elif net == "fashion":
        size, f1, f2 = args
        m = egm.compile(*examples.fashion_mnist_net(size=size, f1=f1, f2=f2), gpu=ctx)
        m.fit("fit", {"x": rng.random((2 * batch, size * size), dtype=f), "y": onehot(2 * batch, 10)}, batch_size=batch)
    elif net == "mse_wide":
        y, x = iters("y x")
        biased = Fun()
        biased.name = "biased"
        biased[y, x] += dsl.input("x")[y, x] + param([args[0]], name="bias")[x]
        loss = layers.mse(layers.leaky_relu(layers.tanh(biased)).target("predict"), dsl.input("t")).target("loss")
        m = egm.compile(loss.backprop(layers.gradient_descent(0.01)).target("train"), gpu=ctx)
        m.apply("train", {"x": rng.random((batch, args[0]), dtype=f), "t": rng.random((batch, args[0]), dtype=f)})
    elif net == "small_chain":
        i, k = iters("i k")
        w, v = param([8, 6], name="w"), param([8], name="v")
        sq, scaled = Fun(), Fun()
        sq.name, scaled.name = "sq", "scaled"
        sq[i] += w[i, k] * w[i, k]
        scaled[i] += sq[i] * v[i]
        y = iters("y")
        out = Fun()
        out.name = "out"
        out[y, i] += dsl.input("x")[y, i] * scaled[i]      # (groups form only in plans that have a batch)
        m = egm.compile(out.target("out"), gpu=ctx)
        m.apply("out", {"x": rng.random((batch, 8), dtype=f)})
    elif net == "xor_adam":
        n = layers.sigmoid(layers.dense(layers.leaky_relu(layers.dense(dsl.input("x"), 2, 4)), 4, 1)).target("predict")
        m = egm.compile(layers.mse(n, dsl.input("y")).target("loss").backprop(layers.adam(eta=0.05)).target("train"), gpu=ctx)
        m.apply("train", {"x": rng.integers(0, 2, (batch, 2)).astype(f), "y": rng.random((batch, 1), dtype=f)})
    elif net == "pool_adam":
        m = egm.compile(*examples.pool_chain_adam(), gpu=ctx)
        m.fit("fit", {"x": rng.random((2 * batch, 36), dtype=f), "y": rng.random((2 * batch, 2, 2, 2), dtype=f)}, batch_size=batch)
    elif net == "cnn":
        chans, size, flt, kh, kw, outs = args
        h, w = size - kh + 1, size - kw + 1
        n = layers.leaky_relu(layers.conv2(dsl.input("x"), dsl.param([flt, kh, kw, chans], name="filters")))
        n = layers.dense(dsl.reshape(n, [-1, h * w * flt]), h * w * flt, outs).target("predict")
        loss = layers.mse(n, dsl.input("y")).target("loss")
        m = egm.compile(loss.backprop(layers.gradient_descent(0.02)).target("train"), gpu=ctx)
        m.apply("train", {"x": rng.random((batch, size, size, chans), dtype=f), "y": rng.random((batch, outs), dtype=f)})
    else:
        raise SystemExit("unknown net " + net)
    ctx.sync()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--out", default=None, help="keep the dumped sources under this directory")
    ap.add_argument("--only", default="")
    ap.add_argument("--timeout", type=int, default=180, help="seconds per child")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    base = a.out or tempfile.mkdtemp(prefix="eg_group_sources_")
    for i, (name, _, _, _, env) in enumerate(cases()):
        if a.only not in name:
            continue
        d = os.path.join(base, "%02d" % i)
        os.makedirs(d, exist_ok=True)
        e = dict(os.environ, EG_DUMP_CODE=d, EG_NO_KERNEL_CACHE="1", **env)
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", name], env=e,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:       # nothing more is started on the GPU after a failure
            print("%s  FAILED exit %d\n%s" % (name, r.returncode, r.stdout[-4000:]), flush=True)
            return 1
        for fn in FILES:
            p = os.path.join(d, fn)
            if not os.path.exists(p):
                print("%s  %s  -" % (name, fn), flush=True)
                continue
            text = open(p, "rb").read()
            names = re.findall(rb"__global__ void (?:__launch_bounds__\([^)]*\) )?(\w+)\(", text)
            groups = sorted({n.decode() for n in names})
            print("%s  %s  %s  %d  kernels=%s  mfma=%d gather4=%d" % (name, fn, hashlib.sha256(text).hexdigest(), len(text), ",".join(groups),
                                                                     text.count(b"__builtin_amdgcn_mfma"), text.count(b"const mf4 a4")), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
