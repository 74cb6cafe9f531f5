#!/usr/bin/env python
"""The price of the running row maximum: eg_attention_stable against eg_attention (the as-written forward), and
eg_attention_stable_grad against eg_attention_grad, on the same q, kk, v stored [batch, seq, head, feat] and resident on the device;
and the model's forward chain under Model.fuse_attention_stable against the same model unfused (eg_model_keep_values: two
eg_bgemm2 products around the collapsed wide row group, the three-launch chain).

  stable / plain          one forward call each; the stable one also stores its Stats, the plain one is eg_attention
  stable_grad / grad      one backward call each over what eg_attention_stable / eg_attention_sums left
  model / kept            Model.apply of `out` with the switch on / with eg_model_keep_values

Inputs are U[-0.5, 0.5): the scores do not grow along j, so after the first key tiles most waves skip the correction — the
common case.  Time per call between two events on the stream: warm-up first, then ROUNDS rounds of at least INNER calls and ROUND_SECONDS of work each, the median
of the rounds.  Every measurement is a fresh process; the sides run in turns, three turns each, so that a drift of the clocks
hits all alike.  The spread of a side is the min-max range of its turns; a ratio counts when the difference exceeds the larger
of the two spreads.

tools/bench_attention_stable.py [BHxIxK ...]            B * H = BH heads, I = J, K = D; the four shapes of profiles/attention_stable.txt by default
tools/bench_attention_stable.py --one WHAT SHAPE        one measurement, one JSON line"""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ["128x512x64", "128x512x128", "128x2048x64", "128x2048x128"]
SIDES = [("stable", "plain"), ("stable_grad", "grad"), ("model", "kept")]
ROUNDS, INNER, ROUND_SECONDS = 9, 10, 0.05
SCALE = 0.125


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


def one(what, spec):
    sys.path.insert(0, HERE)
    import time
    import numpy as np
    import torch
    import exprgrad_amd as eg
    from exprgrad_amd import dsl, ops, model as egm
    BH, I, K = [int(x) for x in spec.split("x")]
    B, H, J, D = BH // 16, 16, I, K
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = eg.newGpuContext(0, stream=stream.cuda_stream)
    torch.manual_seed(0)
    q, kk, v, d_out = (torch.rand(s, device="cuda") - 0.5 for s in ((B, I, H, K), (B, J, H, K), (B, J, H, D), (B, I, H, D)))
    out, stats = torch.full((B, I, H, D), float("nan"), device="cuda"), torch.zeros((B, H, 2, I), device="cuda")
    rows = lambda t, n, w: (t, H * w, (n * H * w, w))
    x = rows(q, I, K) + rows(kk, J, K) + rows(v, J, D) + rows(out, I, D)
    st = (stats, I, (H * 2 * I, 2 * I))
    m = None
    if what in ("model", "kept"):
        m = egm.compile(*program(dsl), gpu=ctx)
        m.fuse_attention_stable(True) if what == "model" else m.keep_values(True)
        args = {"q": q, "kk": kk, "v": v}
        got = torch.from_numpy(np.asarray(m.call("out", args), dtype=np.float32)).cuda()
        run = lambda: m.apply("out", args)
    else:
        grads = [torch.full(t.shape, float("nan"), device="cuda") for t in (q, kk, v)]
        g = rows(d_out, I, D) + rows(grads[0], I, K) + rows(grads[1], J, K) + rows(grads[2], J, D)
        if what in ("stable", "stable_grad"):
            run = lambda: ops.attention_stable(ctx, B, H, I, J, K, D, SCALE, *x, *st)
            back = lambda: ops.attention_stable_grad(ctx, B, H, I, J, K, D, SCALE, *x, *st, *g)
        else:
            sums = (stats, (H * 2 * I, 2 * I))
            run = (lambda: ops.attention(ctx, B, H, I, J, K, D, SCALE, *x)) if what == "plain" else (
                lambda: ops.attention_sums(ctx, B, H, I, J, K, D, SCALE, *x, *sums))
            back = lambda: ops.attention_grad(ctx, B, H, I, J, K, D, SCALE, *x, *sums, *g)
        run()
        got = out
        if what.endswith("grad"):
            run = back
            run()
            got = grads[0]
    torch.cuda.synchronize()
    # float64 on the last head of the last batch item: the context, or dQ
    q1, k1, v1, g1 = (t[B - 1, :, H - 1].double() for t in (q, kk, v, d_out))
    p = torch.softmax(q1 @ k1.T * SCALE, dim=1)
    ref = p @ v1
    if what.endswith("grad"):
        ref = (SCALE * p * (g1 @ v1.T - (g1 * ref).sum(1, keepdim=True))) @ k1
    err = float((got[B - 1, :, H - 1].double() - ref).abs().max() / ref.abs().max())
    t0, calls = time.perf_counter(), 0
    while time.perf_counter() - t0 < 0.3:     # warm-up: lazy builds, clocks
        run()
        torch.cuda.synchronize()
        calls += 1
    inner = max(INNER, min(1000, int(ROUND_SECONDS * calls / 0.3)))   # a round is at least ROUND_SECONDS of work
    rounds = []
    for _ in range(ROUNDS):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        for _ in range(inner):
            run()
        end.record(stream)
        torch.cuda.synchronize()
        rounds.append(start.elapsed_time(end) / inner * 1e3)
    plan = []
    if m is not None:
        plan = [line[:160] for line in m.launch_plan("out").splitlines() if line.startswith("[")]
        m.close()
    return {"what": what, "shape": spec, "us": statistics.median(rounds), "min_us": min(rounds), "max_us": max(rounds), "err_vs_float64": err, "plan": plan}


def child(what, spec):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", what, spec], capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        sys.exit("measurement %s %s failed (exit %d):\n%s" % (what, spec, out.returncode, out.stderr[-3000:]))
    return json.loads(out.stdout.strip().splitlines()[-1])


def report(runs):
    us = [r["us"] for r in runs]
    print(f"  {runs[0]['what']:12s} {statistics.median(us):9.1f} us per call (turns: {', '.join('%.1f' % t for t in us)}; spread {max(us) - min(us):.1f}), "
          f"err vs float64 {runs[-1]['err_vs_float64']:.1e}" + (f"; {len(runs[-1]['plan'])} launch(es)" if runs[-1]['plan'] else ""))
    return statistics.median(us), max(us) - min(us)


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv[:1] == ["--one"]:
        print(json.dumps(one(argv[1], argv[2])))
        sys.exit(0)
    for spec in argv or DEFAULT:
        runs = {what: [] for pair in SIDES for what in pair}
        for _ in range(3):
            for what in runs:
                runs[what].append(child(what, spec))
        print(f"attention, B*H x I x K = {spec} (J = I, D = K), device events, median of {ROUNDS} rounds of at least {INNER} calls and {ROUND_SECONDS} s, 3 turns of fresh processes")
        for new, old in SIDES:
            (a, sa), (b, sb) = report(runs[new]), report(runs[old])
            print(f"  {new} / {old}: {a / b:.3f}x; difference {a - b:.1f} us against a spread of {max(sa, sb):.1f} us: "
                  f"{'outside' if abs(a - b) > max(sa, sb) else 'within'} the spread", flush=True)
