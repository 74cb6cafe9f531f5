#!/usr/bin/env python
"""What sits between the two multi-head products: e = s * 0.125, sums = sum_j exp(e), p = exp(e) / sums over scores
[B, H, I, J], and the whole attention block (scores -> scale -> softmax -> context -> mse -> gradient descent on q, kk, v
stored [batch, seq, head, feat]) as one training step.  Everything is resident on the device (Model.apply: no upload, no
read-back).  Time per call between two events on the stream: warm-up first, then ROUNDS rounds of INNER calls each, the
median of the rounds.

tools/bench_attention_softmax.py [BxHxIxJ[xK]]                 this checkout, with its wide row groups and with EG_NO_ROWFUSE=1
tools/bench_attention_softmax.py --against DIR [BxHxIxJ[xK]]   this checkout against the checkout in DIR (built; for instance
                                                               the parent commit), in turns: every measurement is a fresh
                                                               process, this one first, three turns each
tools/bench_attention_softmax.py --one DIR forward|step SHAPE  one measurement with the package of DIR, one JSON line

The forward's first result is compared with the float64 softmax of one (batch, head) item.  Its floor is one read and one
write of the scores at the copy ceiling of the box (profiles/)."""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = "8x16x512x512x64"
ROUNDS, INNER = 9, 20
SCALE = 0.125


def programs(dsl, layers, dims):
    B, H, I, J, K = dims
    b, h, i, j, k, d = dsl.iters("b h i j k d")

    def softmax(s):
        e, sums, p = dsl.Fun(), dsl.Fun(), dsl.Fun()
        e[b, h, i, j] += s[b, h, i, j] * SCALE
        sums[b, h, i] += dsl.exp(e[b, h, i, j])
        p[b, h, i, j] += dsl.exp(e[b, h, i, j]) / sums[b, h, i]
        return p

    def forward():
        return [softmax(dsl.input("s")).target("out")]

    def step():
        q, kk, v = dsl.param([B, I, H, K], name="q"), dsl.param([B, J, H, K], name="kk"), dsl.param([B, J, H, K], name="v")
        s, o = dsl.Fun(), dsl.Fun()
        s[b, h, i, j] += q[b, i, h, k] * kk[b, j, h, k]
        o[b, i, h, d] += softmax(s)[b, h, i, j] * v[b, j, h, d]
        loss = layers.mse(o, dsl.input("labels")).target("loss")
        return [loss.backwards().optimize([q, kk, v], layers.gradient_descent(0.05)).target("fit")]

    return {"forward": forward, "step": step}


def one(root, what, spec):
    sys.path.insert(0, root)
    import time
    import numpy as np
    import torch
    import exprgrad_amd as eg
    from exprgrad_amd import dsl, layers, model as egm
    dims = [int(v) for v in spec.split("x")]
    dims = dims + [64] * (5 - len(dims))
    B, H, I, J, K = dims
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = eg.newGpuContext(0, stream=stream.cuda_stream)
    m = egm.compile(*programs(dsl, layers, dims)[what](), gpu=ctx)
    torch.manual_seed(0)
    err = None
    if what == "forward":
        target, args = "out", {"s": (torch.rand((B, H, I, J), device="cuda") - 0.5) * 8.0}
        got = m.call(target, args)
        ref = np.exp(args["s"][B - 1, H - 1].double().cpu().numpy() * SCALE)
        ref /= ref.sum(axis=1, keepdims=True)
        err = float(np.max(np.abs(got[B - 1, H - 1] - ref)) / np.max(np.abs(ref)))
    else:
        target, args = "fit", {"labels": torch.rand((B, I, H, K), device="cuda") - 0.5}
        rng = np.random.default_rng(0)
        for tid in sorted(m.params.ids()):
            m.params[tid] = (rng.random(m.params[tid].shape, dtype=np.float32) - np.float32(0.5)).astype(np.float32)
    run = lambda: m.apply(target, args)
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
    plan = [line for line in m.launch_plan(target).splitlines() if line.startswith("[")]
    m.close()
    return {"root": root, "what": what, "shape": spec, "us": statistics.median(rounds), "min_us": min(rounds), "max_us": max(rounds),
            "err_vs_float64": err, "plan": plan, "scores_mb": 4.0 * B * H * I * J / 1e6}


def child(root, what, spec, env=None):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", root, what, spec], capture_output=True, text=True,
                         env=dict(os.environ, **(env or {})), timeout=600)
    if out.returncode != 0:
        sys.exit("measurement with %s failed (exit %d):\n%s" % (root, out.returncode, out.stderr[-3000:]))
    return json.loads(out.stdout.strip().splitlines()[-1])


def report(name, runs):
    med = statistics.median(r["us"] for r in runs)
    err = runs[-1]["err_vs_float64"]
    print(f"{name}: {med:9.1f} us per call (turns: {', '.join('%.1f' % r['us'] for r in runs)}; rounds of the last turn "
          f"{runs[-1]['min_us']:.1f} .. {runs[-1]['max_us']:.1f})" + ("" if err is None else f", err vs float64 {err:.1e}"))
    for line in runs[-1]["plan"]:
        print("    " + line[:200])
    sys.stdout.flush()
    return med


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv[:1] == ["--one"]:
        print(json.dumps(one(os.path.abspath(argv[1]), argv[2], argv[3])))
        sys.exit(0)
    other = None
    if argv[:1] == ["--against"]:
        other, argv = os.path.abspath(argv[1]), argv[2:]
    spec = argv[0] if argv else DEFAULT
    sides = [("this checkout", HERE, None)]
    sides.append(("the checkout in %s" % other, other, None) if other else ("this checkout, EG_NO_ROWFUSE=1", HERE, {"EG_NO_ROWFUSE": "1"}))
    for what, title in (("forward", "scale -> softmax, one `out` call on device-resident scores"), ("step", "the attention block's training step")):
        runs = {name: [] for name, _, _ in sides}
        for _ in range(3):              # in turns, so that a drift of the clocks hits both alike
            for name, root, env in sides:
                runs[name].append(child(root, what, spec, env))
        print(f"{title}, {spec} (B x H x I x J x K), device events, median of {ROUNDS} rounds of {INNER} calls")
        new, old = (report(name, runs[name]) for name, _, _ in sides)
        if what == "forward":
            mb = runs[sides[0][0]][-1]["scores_mb"]
            print(f"    one read and one write of the scores: 2 x {mb:.0f} MB; {2 * mb / new:.2f} TB/s in this checkout")
        print(f"ratio: {old / new:.2f}x ({sides[1][0]} / {sides[0][0]})", flush=True)
