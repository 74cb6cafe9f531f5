#!/usr/bin/env python
"""The attention block's forward pass, out[b,i,h,:] = softmax_j(scale * q[b,i,h,:] . kk[b,j,h,:]) * v[b,j,h,:] on tensors
stored [batch, seq, head, feat], everything resident on the device:

  model   the `out` target of the five-statement program through the model layer (Model.apply: no upload, no read-back).
          This checkout runs it as one eg_attn launch (kernels/attention_f32.hip: nothing of size I x J is stored); a
          checkout without the route runs two eg_bgemm2 products with the collapsed wide row group between them — three
          launches that write the scores once, rewrite them in the softmax and read them a fourth time.
  entry   one eg_attention call on the same tensors, this checkout only: the kernel without the model layer around it

Time per call between two events on the stream: warm-up first, then ROUNDS rounds of INNER calls each, the median of the
rounds.  Every measurement is a fresh process; the sides run in turns, three turns each, so that a drift of the clocks hits
all alike.  The spread of a side is the min-max range of its turns; a difference counts when it exceeds the larger of the
two spreads.  For the entry: the fraction of the f32 matrix peak (157.3 TFLOP/s) its 2 * I * J * (K + D) flops per item
reach, and the operand and result bytes per second.

tools/bench_attention_fused.py --against DIR [BxHxIxJxK[xD] ...]   this checkout against the built checkout in DIR (for instance
                                                                   the parent commit); both shapes of profiles/attention_fused.txt
                                                                   by default
tools/bench_attention_fused.py [SHAPE ...]                         this checkout against itself with eg_model_keep_values, which
                                                                   keeps the unfused plan (and stores every row of the softmax group)
tools/bench_attention_fused.py --one DIR model|kept|entry SHAPE    one measurement with the package of DIR, one JSON line"""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ["8x16x512x512x64", "8x16x2048x2048x64"]
ROUNDS, INNER = 9, 10
SCALE = 0.125
MFMA_F32_TFLOPS = 157.3


def program(dsl):
    b, h, i, j, k, d = dsl.iters("b h i j k d")
    q, kk, v = dsl.input("q"), dsl.input("kk"), dsl.input("v")
    s, e, sums, p, o = (dsl.Fun() for _ in range(5))
    s[b, h, i, j] += q[b, i, h, k] * kk[b, j, h, k]
    e[b, h, i, j] += s[b, h, i, j] * SCALE
    sums[b, h, i] += dsl.exp(e[b, h, i, j])
    p[b, h, i, j] += dsl.exp(e[b, h, i, j]) / sums[b, h, i]
    o[b, i, h, d] += p[b, h, i, j] * v[b, j, h, d]
    return [o.target("out")]


def one(root, what, spec):
    sys.path.insert(0, root)
    import time
    import numpy as np
    import torch
    import exprgrad_amd as eg
    from exprgrad_amd import dsl, ops, model as egm
    dims = [int(x) for x in spec.split("x")]
    dims = dims + [dims[4]] * (6 - len(dims))
    B, H, I, J, K, D = dims
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = eg.newGpuContext(0, stream=stream.cuda_stream)
    torch.manual_seed(0)
    q, kk, v = (torch.rand(s, device="cuda") - 0.5 for s in ((B, I, H, K), (B, J, H, K), (B, J, H, D)))
    plan, m = [], None
    if what == "entry":
        out = torch.full((B, I, H, D), float("nan"), device="cuda")

        def run():
            ops.attention(ctx, B, H, I, J, K, D, SCALE, q, H * K, (I * H * K, K), kk, H * K, (J * H * K, K), v, H * D, (J * H * D, D), out, H * D,
                          (I * H * D, D))
        run()
        torch.cuda.synchronize()
        got = out[B - 1, :, H - 1].cpu().numpy()
    else:
        m = egm.compile(*program(dsl), gpu=ctx)
        if what == "kept":
            m.keep_values(True)
        args = {"q": q, "kk": kk, "v": v}
        got = m.call("out", args)[B - 1, :, H - 1]
        run = lambda: m.apply("out", args)
    s = np.exp(q[B - 1, :, H - 1].double().cpu().numpy() @ kk[B - 1, :, H - 1].double().cpu().numpy().T * SCALE)
    ref = (s @ v[B - 1, :, H - 1].double().cpu().numpy()) / s.sum(axis=1, keepdims=True)
    err = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3:     # warm-up: lazy builds, clocks
        run()
        torch.cuda.synchronize()
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
        plan = [line for line in m.launch_plan("out").splitlines() if line.startswith("[")]
        m.close()
    return {"root": root, "what": what, "shape": spec, "us": statistics.median(rounds), "min_us": min(rounds), "max_us": max(rounds), "err_vs_float64": err,
            "plan": plan, "flops": 2.0 * B * H * I * J * (K + D), "bytes": 4.0 * B * H * (I * K + J * K + J * D + I * D),
            "scores_mb": 4.0 * B * H * I * J / 1e6}


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


def child(root, what, spec):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", root, what, spec], capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        sys.exit("measurement %s %s of %s checkout failed (exit %d):\n%s" % (what, spec, "this" if root == HERE else "the other", out.returncode, out.stderr[-3000:]))
    return json.loads(out.stdout.strip().splitlines()[-1])


def report(name, runs):
    us = [r["us"] for r in runs]
    med = statistics.median(us)
    print(f"{name}: {med:9.1f} us per call (turns: {', '.join('%.1f' % x for x in us)}; spread {max(us) - min(us):.1f}; rounds of the last turn "
          f"{runs[-1]['min_us']:.1f} .. {runs[-1]['max_us']:.1f}), err vs float64 {runs[-1]['err_vs_float64']:.1e}")
    for line in runs[-1]["plan"]:
        print("    " + line[:200])
    sys.stdout.flush()
    return med, max(us) - min(us)


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv[:1] == ["--one"]:
        print(json.dumps(one(os.path.abspath(argv[1]), argv[2], argv[3])))
        sys.exit(0)
    other = None
    if argv[:1] == ["--against"]:
        other, argv = os.path.abspath(argv[1]), argv[2:]
    sides = [("this checkout, `out` through the model", HERE, "model"),
             ("the other checkout%s, `out` through the model" % commit_of(other), other, "model") if other else ("this checkout, eg_model_keep_values", HERE, "kept"),
             ("this checkout, one eg_attention call", HERE, "entry")]
    for spec in argv or DEFAULT:
        runs = {name: [] for name, _, _ in sides}
        for _ in range(3):
            for name, root, what in sides:
                runs[name].append(child(root, what, spec))
        print(f"attention forward, {spec} (B x H x I x J x K[x D]), device events, median of {ROUNDS} rounds of {INNER} calls")
        (new, new_spread), (old, old_spread), (entry, _) = (report(name, runs[name]) for name, _, _ in sides)
        r = runs[sides[2][0]][-1]
        print(f"    eg_attention: {r['flops'] / entry / 1e6:.1f} TFLOP/s = {100 * r['flops'] / entry / 1e6 / MFMA_F32_TFLOPS:.1f} % of the f32 matrix peak; "
              f"operands and result {r['bytes'] / 1e6:.0f} MB, {r['bytes'] / entry / 1e6:.2f} TB/s; the scores it does not store: {r['scores_mb']:.0f} MB")
        spread = max(new_spread, old_spread)
        verdict = "faster by more than the spread" if old - new > spread else ("slower" if new > old else "faster, but within the spread")
        print(f"ratio: {old / new:.2f}x ({sides[1][0]} / {sides[0][0]}); difference {old - new:.1f} us against a spread of {spread:.1f} us: {verdict}",
              flush=True)
