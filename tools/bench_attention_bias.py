#!/usr/bin/env python
"""Causal attention through the model layer, out[b,i,h,:] = softmax_j(scale * q[b,i,h,:] . kk[b,j,h,:] + m[i,j]) * v[b,j,h,:] with
m[i,j] = -Inf above the diagonal, on tensors stored [batch, seq, head, feat], everything resident on the device:

  model   the `out` target of the five-statement program whose scale map adds m[i,j] (Model.apply: no upload, no read-back).
          This checkout runs it as one eg_attn launch with the bias operand (kernels/attention_f32.hip, BIAS: nothing of size
          I x J is stored, the I x J table is read once per batch item and head); a checkout without the route — or this one
          under eg_model_keep_values — runs two eg_bgemm2 products around a generated map and the collapsed wide row group.
  bias0   one eg_attention_bias call with a bias of zeros [i,j] on the same q, kk, v
  plain   one eg_attention call on the same q, kk, v: bias0 - plain is the price of the operand (sixteen loads and additions
          per lane and key tile, 32 more registers)

Time per call between two events on the stream: warm-up first, then ROUNDS rounds of INNER calls each, the median of the
rounds.  Every measurement is a fresh process; the sides run in turns, three turns each, so that a drift of the clocks hits
all alike.  The spread of a side is the min-max range of its turns; a difference counts when it exceeds the larger of the
two spreads.

tools/bench_attention_bias.py --against DIR [BxHxIxJxK ...]   this checkout against the built checkout in DIR (the parent commit);
                                                              both shapes of profiles/attention_fused.txt by default
tools/bench_attention_bias.py [SHAPE ...]                     this checkout against itself with eg_model_keep_values (the unfused plan)
tools/bench_attention_bias.py --one DIR model|kept|bias0|plain SHAPE    one measurement with the package of DIR, one JSON line"""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ["8x16x512x512x64", "8x16x2048x2048x64"]
ROUNDS, INNER = 9, 10
SCALE = 0.125


def program(dsl):
    b, h, i, j, k, d = dsl.iters("b h i j k d")
    q, kk, v, m = dsl.input("q"), dsl.input("kk"), dsl.input("v"), dsl.input("m")
    s, e, sums, p, o = (dsl.Fun() for _ in range(5))
    s[b, h, i, j] += q[b, i, h, k] * kk[b, j, h, k]
    e[b, h, i, j] += s[b, h, i, j] * SCALE + m[i, j]
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
    B, H, I, J, K = [int(x) for x in spec.split("x")]
    D = K
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = eg.newGpuContext(0, stream=stream.cuda_stream)
    torch.manual_seed(0)
    q, kk, v = (torch.rand(s, device="cuda") - 0.5 for s in ((B, I, H, K), (B, J, H, K), (B, J, H, D)))
    causal = torch.full((I, J), float("-inf"), device="cuda").triu(1)
    plan, m = [], None
    if what in ("bias0", "plain"):
        out = torch.full((B, I, H, D), float("nan"), device="cuda")
        bias = torch.zeros((I, J), device="cuda")
        x = (q, H * K, (I * H * K, K), kk, H * K, (J * H * K, K), v, H * D, (J * H * D, D), out, H * D, (I * H * D, D))
        if what == "bias0":
            run = lambda: ops.attention_bias(ctx, B, H, I, J, K, D, SCALE, *x, None, (0, 0), bias, J, (0, 0))
        else:
            run = lambda: ops.attention(ctx, B, H, I, J, K, D, SCALE, *x)
        run()
        torch.cuda.synchronize()
        got, mask = out[B - 1, :, H - 1].cpu().numpy(), bias.double().cpu().numpy()
    else:
        m = egm.compile(*program(dsl), gpu=ctx)
        if what == "kept":
            m.keep_values(True)
        args = {"q": q, "kk": kk, "v": v, "m": causal}
        got, mask = m.call("out", args)[B - 1, :, H - 1], causal.double().cpu().numpy()
        run = lambda: m.apply("out", args)
    s = np.exp(q[B - 1, :, H - 1].double().cpu().numpy() @ kk[B - 1, :, H - 1].double().cpu().numpy().T * SCALE + mask)
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
    return {"what": what, "shape": spec, "us": statistics.median(rounds), "min_us": min(rounds), "max_us": max(rounds), "err_vs_float64": err,
            "plan": plan, "flops": 2.0 * B * H * I * J * (K + D), "bias_mb": 4.0 * I * J / 1e6, "scores_mb": 4.0 * B * H * I * J / 1e6}


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


def verdict(slow, fast, spread):
    return "outside the spread" if abs(slow - fast) > spread else "within the spread"


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv[:1] == ["--one"]:
        print(json.dumps(one(os.path.abspath(argv[1]), argv[2], argv[3])))
        sys.exit(0)
    other = None
    if argv[:1] == ["--against"]:
        other, argv = os.path.abspath(argv[1]), argv[2:]
    sides = [("this checkout, causal `out` through the model", HERE, "model"),
             ("the other checkout, causal `out` through the model", other, "model") if other else ("this checkout, eg_model_keep_values", HERE, "kept"),
             ("this checkout, eg_attention_bias with a zero bias", HERE, "bias0"), ("this checkout, eg_attention", HERE, "plain")]
    for spec in argv or DEFAULT:
        runs = {name: [] for name, _, _ in sides}
        for _ in range(3):
            for name, root, what in sides:
                runs[name].append(child(root, what, spec))
        print(f"causal attention forward, {spec} (B x H x I x J x K, D = K), device events, median of {ROUNDS} rounds of {INNER} calls")
        (new, s0), (old, s1), (bias0, s2), (plain, s3) = (report(name, runs[name]) for name, _, _ in sides)
        r = runs[sides[2][0]][-1]
        print(f"    eg_attention_bias: {r['flops'] / bias0 / 1e6:.1f} TFLOP/s against eg_attention's {r['flops'] / plain / 1e6:.1f}; the bias table {r['bias_mb']:.1f} MB, "
              f"the scores neither stores {r['scores_mb']:.0f} MB")
        print(f"model: {old / new:.2f}x ({sides[1][0]} / {sides[0][0]}); difference {old - new:.1f} us against a spread of {max(s0, s1):.1f} us: "
              f"{verdict(old, new, max(s0, s1))}")
        print(f"price of the operand: {bias0 - plain:.1f} us = {100 * (bias0 - plain) / plain:.1f} % of eg_attention, against a spread of {max(s2, s3):.1f} us: "
              f"{verdict(bias0, plain, max(s2, s3))}", flush=True)
