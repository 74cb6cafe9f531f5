#!/usr/bin/env python
"""One `fit` step of the attention block's training program through the model layer (Model.apply), tensors stored
[batch, seq, head, feat], parameters q, kk, v resident on the device, three ways:

  on       Model.fuse_attention_fit(True): the chain as one eg_attn launch that stores the sums, its gradient kernels as one
           eg_attn_grad launch; nothing of size I x J is stored
  off      the setting never touched, this checkout: the unfused products and row groups, with the scores, the scaled scores,
           the softmax and their gradients stored
  parent   with --against DIR: the same step from the built checkout in DIR (for instance the parent commit), setting off —
           `off` has to be level with it within the turns' spread

Time per step between two events on the stream: warm-up first, then ROUNDS rounds of INNER steps each, the median of the
rounds.  Every measurement is a fresh process; the sides run in turns, three turns each, so that a drift of the clocks hits
all alike.  The spread of a side is the min-max range of its turns.  Every side prints the sum of the parameters' magnitudes
after its first three steps, from the same parameters and labels: on and off agree to float32 rounding, off and the other
checkout to the last digit.  Device memory held: what the process took between the
context's creation and the end of the warm-up (parameters, labels, the plan's arena).

tools/bench_attention_fit.py [--against DIR] [BxHxIxJxK[xD] ...]     both shapes of profiles/attention_fit.txt by default
tools/bench_attention_fit.py --one DIR on|off SHAPE                   one measurement with the package of DIR, one JSON line"""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ["8x16x512x512x64", "8x16x2048x2048x64"]
ROUNDS, INNER = 9, 10
SCALE = 0.125


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
    from exprgrad_amd import dsl, layers, model as egm
    dims = [int(x) for x in spec.split("x")]
    dims = dims + [dims[4]] * (6 - len(dims))
    B, H, I, J, K, D = dims
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = eg.newGpuContext(0, stream=stream.cuda_stream)
    free_before = torch.cuda.mem_get_info()[0]
    m = egm.compile(*training(dsl, layers, dims), gpu=ctx)
    if what == "on":
        m.fuse_attention_fit(True)
    rng = np.random.default_rng(0)
    for tid in sorted(m.params.ids()):
        m.params[tid] = (rng.random(m.params[tid].shape, dtype=np.float32) - np.float32(0.5)).astype(np.float32)
    torch.manual_seed(0)
    args = {"labels": torch.rand((B, I, H, D), device="cuda") - 0.5}
    run = lambda: m.apply("fit", args)
    for _ in range(3):      # the same three steps on every side: what the sides' parameters are compared after
        run()
    torch.cuda.synchronize()
    checksum = float(sum(np.abs(m.params[tid]).sum(dtype=np.float64) for tid in sorted(m.params.ids())))
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3:     # warm-up: lazy builds, the graph's capture, clocks
        run()
        torch.cuda.synchronize()
    held = free_before - torch.cuda.mem_get_info()[0]
    rounds = []
    for _ in range(ROUNDS):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        for _ in range(INNER):
            run()
        end.record(stream)
        torch.cuda.synchronize()
        rounds.append(start.elapsed_time(end) / INNER * 1e3)
    plan = [line for line in m.launch_plan("fit").splitlines() if line.startswith("[")]
    m.close()
    return {"what": what, "shape": spec, "us": statistics.median(rounds), "min_us": min(rounds), "max_us": max(rounds), "plan": plan,
            "held_mb": held / 1e6, "checksum": checksum}


def child(root, what, spec):
    cmd = [sys.executable, os.path.abspath(__file__), "--one", root, what, spec]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        sys.exit("measurement %s %s of %s checkout failed (exit %d):\n%s" % (what, spec, "this" if root == HERE else "the other", out.returncode, out.stderr[-3000:]))
    return json.loads([line for line in out.stdout.splitlines() if line.startswith("{")][-1])


def report(name, runs):
    us = [r["us"] for r in runs]
    med = statistics.median(us)
    print(f"{name}: {med:9.1f} us per step (turns: {', '.join('%.1f' % x for x in us)}; spread {max(us) - min(us):.1f}; rounds of the last turn "
          f"{runs[-1]['min_us']:.1f} .. {runs[-1]['max_us']:.1f}), device memory held {runs[-1]['held_mb']:.0f} MB, "
          f"sum of |parameters| after three steps {runs[-1]['checksum']:.9g}")
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
    other = None
    if argv[:1] == ["--against"]:
        other, argv = os.path.abspath(argv[1]), argv[2:]
    sides = [("setting on, this checkout", HERE, "on"), ("setting off, this checkout", HERE, "off")]
    if other:
        sides.append(("setting off, the other checkout" + commit_of(other), other, "off"))
    for spec in argv or DEFAULT:
        runs = {name: [] for name, _, _ in sides}
        for _ in range(3):
            for name, root, what in sides:
                runs[name].append(child(root, what, spec))
        print(f"attention fit step, {spec} (B x H x I x J x K[x D]), device events, median of {ROUNDS} rounds of {INNER} steps")
        got = [report(name, runs[name]) for name, _, _ in sides]
        (on, on_spread), (off, off_spread) = got[0], got[1]
        print(f"on {on:.1f} us against off {off:.1f} us: ratio {off / on:.2f}x; spreads {on_spread:.1f} and {off_spread:.1f} us")
        if other:
            parent, parent_spread = got[2]
            print(f"off {off:.1f} us against the other checkout {parent:.1f} us: difference {off - parent:+.1f} us; spreads {off_spread:.1f} and {parent_spread:.1f} us",
                  flush=True)
