#!/usr/bin/env python
"""The attention block's backward pass on tensors stored [batch, seq, head, feat], everything resident on the device:

  sums     one eg_attention_sums call: the forward, also storing its denominators
  grad     one eg_attention_grad call: the dQ kernel and the dK/dV kernel, nothing of size I x J stored
  kernels  the two kernels of that call one by one: one more process under `rocprofv3 --kernel-trace --stats`, the mean
           duration of each kernel over its calls (device events cannot tell two launches of one call apart)
  fit      for comparison, the `fit` step of the attention block's training program through the model layer (Model.apply), which
           no launch plan routes through these entries yet: the unfused products and row groups, with the scores, the scaled
           scores, the softmax and their gradients stored.  With --against DIR it runs from the built checkout in DIR (for
           instance the parent commit), else from this one.

Time per call between two events on the stream: warm-up first, then ROUNDS rounds of INNER calls each, the median of the
rounds.  Every measurement is a fresh process; the sides run in turns, three turns each, so that a drift of the clocks hits
all alike.  The spread of a side is the min-max range of its turns.  Flops per item: 2 I J (K + D) for the forward, 2 I J (2 K + D)
for the dQ kernel (S, dP, dS K), 2 I J (2 K + 2 D) for the dK/dV kernel (S^T, dP^T, p^T dO, dS^T Q): 2 I J (4 K + 3 D) for the pair.

tools/bench_attention_grad.py [--against DIR] [BxHxIxJxK[xD] ...]     both shapes of profiles/attention_grad.txt by default
tools/bench_attention_grad.py --one DIR sums|grad|fit SHAPE            one measurement with the package of DIR, one JSON line"""
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ["8x16x512x512x64", "8x16x2048x2048x64"]
ROUNDS, INNER = 9, 10
SCALE = 0.125
MFMA_F32_TFLOPS = 157.3
FORWARD_TFLOPS = {"8x16x512x512x64": 83.8, "8x16x2048x2048x64": 93.6}      # eg_attention, profiles/attention_fused.txt


def training(dsl, layers, dims):
    B, H, I, J, K, D = dims
    b, h, i, j, k, d = dsl.iters("b h i j k d")
    q, kk, v = dsl.param([B, I, H, K], name="q"), dsl.param([B, J, H, K], name="kk"), dsl.param([B, J, H, D], name="v")
    s, e, sums, p, o = (dsl.Fun() for _ in range(5))
    s[b, h, i, j] += q[b, i, h, k] * kk[b, j, h, k]
    e[b, h, i, j] += s[b, h, i, j] * SCALE
    sums[b, h, i] += dsl.exp(e[b, h, i, j])
    p[b, h, i, j] += dsl.exp(e[b, h, i, j]) / sums[b, h, i]
    o[b, i, h, d] += p[b, h, i, j] * v[b, j, h, d]
    loss = layers.mse(o, dsl.input("labels")).target("loss")
    return [loss.backwards().optimize([q, kk, v], layers.gradient_descent(0.05)).target("fit")]


def one(root, what, spec):
    sys.path.insert(0, root)
    import time
    import numpy as np
    import torch
    import exprgrad_amd as eg
    from exprgrad_amd import dsl, layers, ops, model as egm
    dims = [int(x) for x in spec.split("x")]
    dims = dims + [dims[4]] * (6 - len(dims))
    B, H, I, J, K, D = dims
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = eg.newGpuContext(0, stream=stream.cuda_stream)
    torch.manual_seed(0)
    plan, m, err = [], None, None
    free_before = torch.cuda.mem_get_info()[0]
    if what == "fit":
        m = egm.compile(*training(dsl, layers, dims), gpu=ctx)
        rng = np.random.default_rng(0)
        for tid in sorted(m.params.ids()):
            m.params[tid] = (rng.random(m.params[tid].shape, dtype=np.float32) - np.float32(0.5)).astype(np.float32)
        args = {"labels": torch.rand((B, I, H, D), device="cuda") - 0.5}
        run = lambda: m.apply("fit", args)
    else:
        q, kk, v, d_out = (torch.rand(s, device="cuda") - 0.5 for s in ((B, I, H, K), (B, J, H, K), (B, J, H, D), (B, I, H, D)))
        out = torch.full((B, I, H, D), float("nan"), device="cuda")
        sums = torch.full((B, H, I), float("nan"), device="cuda")
        dq, dk, dv = (torch.full(tuple(x.shape), float("nan"), device="cuda") for x in (q, kk, v))
        sq, sk, sv, so = (I * H * K, K), (J * H * K, K), (J * H * D, D), (I * H * D, D)

        def forward():
            ops.attention_sums(ctx, B, H, I, J, K, D, SCALE, q, H * K, sq, kk, H * K, sk, v, H * D, sv, out, H * D, so, sums, (H * I, I))

        def backward():
            ops.attention_grad(ctx, B, H, I, J, K, D, SCALE, q, H * K, sq, kk, H * K, sk, v, H * D, sv, out, H * D, so, sums, (H * I, I), d_out, H * D, so,
                               dq, H * K, sq, dk, H * K, sk, dv, H * D, sv)
        forward()
        backward()
        torch.cuda.synchronize()
        # the last item against float64
        f = lambda x: x[B - 1, :, H - 1].double().cpu().numpy()
        e = np.exp(f(q) @ f(kk).T * SCALE)
        p = e / e.sum(axis=1, keepdims=True)
        dp = f(d_out) @ f(v).T
        ds = SCALE * p * (dp - np.sum(f(d_out) * (p @ f(v)), axis=1, keepdims=True))
        far = lambda got, ref: float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
        err = max(far(sums[B - 1, H - 1].double().cpu().numpy(), e.sum(axis=1)), far(f(dq), ds @ f(kk)), far(f(dk), ds.T @ f(q)),
                  far(f(dv), p.T @ f(d_out)))
        run = forward if what == "sums" else backward
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3:     # warm-up: lazy builds, clocks
        run()
        torch.cuda.synchronize()
    held = free_before - torch.cuda.mem_get_info()[0]      # device memory this process took for the operands and what the step stores
    rounds = []
    for _ in range(ROUNDS):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        for _ in range(INNER):
            run()
        end.record(stream)
        torch.cuda.synchronize()
        rounds.append(start.elapsed_time(end) / INNER * 1e3)
    if m is not None:
        plan = [line for line in m.launch_plan("fit").splitlines() if line.startswith("[")]
        m.close()
    return {"what": what, "shape": spec, "us": statistics.median(rounds), "min_us": min(rounds), "max_us": max(rounds), "err_vs_float64": err,
            "plan": plan, "held_mb": held / 1e6}


def child(root, what, spec, profile_dir=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--one", root, what, spec]
    if profile_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", profile_dir, "-o", "t", "--"] + cmd
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        sys.exit("measurement %s %s of %s checkout failed (exit %d):\n%s" % (what, spec, "this" if root == HERE else "the other", out.returncode, out.stderr[-3000:]))
    return json.loads([line for line in out.stdout.splitlines() if line.startswith("{")][-1])


def kernel_means(spec):
    """{"dq" / "dkv": (calls, mean us)} of one profiled process that runs eg_attention_grad"""
    with tempfile.TemporaryDirectory() as tmp:
        child(HERE, "grad", spec, profile_dir=tmp)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        found = {}
        for row in csv.DictReader(open(files[0])) if files else []:
            for key in ("dq", "dkv"):
                if "attention_%s_kernel" % key in row["Name"]:
                    found[key] = (int(row["Calls"]), float(row["TotalDurationNs"]) / int(row["Calls"]) / 1e3)
        return found


def report(name, runs):
    us = [r["us"] for r in runs]
    med = statistics.median(us)
    err = runs[-1]["err_vs_float64"]
    print(f"{name}: {med:9.1f} us per call (turns: {', '.join('%.1f' % x for x in us)}; spread {max(us) - min(us):.1f}; rounds of the last turn "
          f"{runs[-1]['min_us']:.1f} .. {runs[-1]['max_us']:.1f})" + (f", err vs float64 {err:.1e}" if err is not None else "") +
          f", device memory held {runs[-1]['held_mb']:.0f} MB")
    for line in runs[-1]["plan"]:
        print("    " + line[:200])
    sys.stdout.flush()
    return med, max(us) - min(us)


def commit_of(root):
    """' (commit abc1234)' when DIR is a git checkout, else nothing: the printed label never holds DIR itself"""
    try:
        out = subprocess.run(["git", "-C", root, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, timeout=30)
        top = subprocess.run(["git", "-C", root, "rev-parse", "--show-toplevel"], capture_output=True, text=True, timeout=30)
        if out.returncode == 0 and top.returncode == 0 and os.path.realpath(top.stdout.strip()) == os.path.realpath(root):
            return " (commit %s)" % out.stdout.strip()
    except OSError:
        pass
    return ""


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv[:1] == ["--one"]:
        print(json.dumps(one(os.path.abspath(argv[1]), argv[2], argv[3])))
        sys.exit(0)
    other = HERE
    if argv[:1] == ["--against"]:
        other, argv = os.path.abspath(argv[1]), argv[2:]
    sides = [("eg_attention_sums", HERE, "sums"), ("eg_attention_grad", HERE, "grad"),
             ("`fit` through the model, %s" % ("this checkout" if other == HERE else "the other checkout" + commit_of(other)), other, "fit")]
    for spec in argv or DEFAULT:
        dims = [int(x) for x in spec.split("x")]
        B, H, I, J, K, D = dims + [dims[4]] * (6 - len(dims))
        runs = {name: [] for name, _, _ in sides}
        for _ in range(3):
            for name, root, what in sides:
                runs[name].append(child(root, what, spec))
        print(f"attention backward, {spec} (B x H x I x J x K[x D]), device events, median of {ROUNDS} rounds of {INNER} calls")
        (fwd, _), (grad, grad_spread), (fit, fit_spread) = (report(name, runs[name]) for name, _, _ in sides)
        unit = 2.0 * B * H * I * J / 1e6      # flops per unit of head dimension, in TFLOP per us
        flops = {"sums": unit * (K + D), "dq": unit * (2 * K + D), "dkv": unit * (2 * K + 2 * D), "grad": unit * (4 * K + 3 * D)}
        tf = lambda key, us: f"{flops[key] / us:.1f} TFLOP/s = {100 * flops[key] / us / MFMA_F32_TFLOPS:.1f} % of the f32 matrix peak"
        print(f"    eg_attention_sums: {tf('sums', fwd)}" + (f" (eg_attention on record: {FORWARD_TFLOPS[spec]})" if spec in FORWARD_TFLOPS else ""))
        print(f"    eg_attention_grad: {tf('grad', grad)}")
        for key, (calls, us) in sorted(kernel_means(spec).items()):
            print(f"    attention_{key}_kernel: {us:9.1f} us mean of {calls} calls under rocprofv3 --kernel-trace; {tf(key, us)}")
        ij = 4.0 * B * H * I * J / 1e6
        print(f"    a tensor of B x H x I x J floats is {ij:.0f} MB: the unfused step stores the scores, the scaled scores, the softmax and their gradients "
              f"(device memory held, above); eg_attention_sums and eg_attention_grad store none, their process holds the nine operands")
        print(f"sums + grad {fwd + grad:.1f} us against the whole fit step {fit:.1f} us (forward, backward, loss and update): ratio {fit / (fwd + grad):.2f}x; "
              f"spreads {grad_spread:.1f} and {fit_spread:.1f} us", flush=True)
