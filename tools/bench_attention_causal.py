#!/usr/bin/env python
"""What skipping the masked key tiles buys: eg_attention_causal and eg_attention_causal_grad (offset 0) against what a user does
without them, eg_attention_stable and eg_attention_stable_grad with an [I, J] bias table of -Inf above the diagonal, and against
the same entries without any mask, on q, kk, v stored [batch, seq, head, feat] and resident on the device.

  causal / table          the forward: the causal entry; the stable entry with the -Inf table (both store their Stats)
  causal / nobias         the stable entry without a bias: every tile computed, nothing masked
  causal / natural        the causal entry from a second build whose blocks take the row tiles in ascending order
                          (make OBJ=... OUT=DIR EXTRA_CXXFLAGS=-DEG_ATTENTION_CAUSAL_NATURAL_ORDER, given as --natural DIR/libexprgrad_hip.so);
                          left out without --natural
  *_grad                  the same four for one backward call (dQ, then dK and dV) over what the forward left

The floor of causal / nobias is the share of tile visits, T (T + 1) / 2 of T * T with T = I / 64: the diagonal tiles are computed.
Time per call between two events on the stream: warm-up first, then ROUNDS rounds of at least INNER calls and ROUND_SECONDS of
work each, the median of the rounds.  Every measurement is a fresh process; the sides run in turns, three turns each, so that a
drift of the clocks hits all alike.  The spread of a side is the min-max range of its turns; a ratio counts when the difference
exceeds the larger of the two spreads.

tools/bench_attention_causal.py [--natural LIB] [BxHxIxK ...]   J = I, D = K; the two shapes of profiles/attention_causal.txt by default
tools/bench_attention_causal.py --one WHAT SHAPE                 one measurement, one JSON line"""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ["8x16x512x64", "8x16x2048x64"]
ROUNDS, INNER, ROUND_SECONDS = 9, 10, 0.05
SCALE = 0.125


def one(what, spec):
    sys.path.insert(0, HERE)
    import time
    import torch
    import exprgrad_amd as eg
    from exprgrad_amd import ops
    B, H, I, K = [int(x) for x in spec.split("x")]
    J, D = I, K
    side = what[:-5] if what.endswith("_grad") else what
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = eg.newGpuContext(0, stream=stream.cuda_stream)
    torch.manual_seed(0)
    q, kk, v, d_out = (torch.rand(s, device="cuda") - 0.5 for s in ((B, I, H, K), (B, J, H, K), (B, J, H, D), (B, I, H, D)))
    out, stats = torch.full((B, I, H, D), float("nan"), device="cuda"), torch.zeros((B, H, 2, I), device="cuda")
    mask = torch.full((I, J), float("-inf"), device="cuda").triu(1)
    rows = lambda t, n, w: (t, H * w, (n * H * w, w))
    x = rows(q, I, K) + rows(kk, J, K) + rows(v, J, D) + rows(out, I, D)
    st = (stats, I, (H * 2 * I, 2 * I))
    grads = [torch.full(t.shape, float("nan"), device="cuda") for t in (q, kk, v)]
    g = rows(d_out, I, D) + rows(grads[0], I, K) + rows(grads[1], J, K) + rows(grads[2], J, D)
    bias = (mask, J, (0, 0)) if side == "table" else (None, 0, (0, 0))
    if side in ("causal", "natural"):
        run = lambda: ops.attention_causal(ctx, B, H, I, J, K, D, SCALE, *x, *st, offset=0)
        back = lambda: ops.attention_causal_grad(ctx, B, H, I, J, K, D, SCALE, *x, *st, *g, offset=0)
    else:
        run = lambda: ops.attention_stable(ctx, B, H, I, J, K, D, SCALE, *x, *st, *bias)
        back = lambda: ops.attention_stable_grad(ctx, B, H, I, J, K, D, SCALE, *x, *st, *g, *bias)
    run()
    got = out
    if what.endswith("_grad"):
        run = back
        run()
        got = grads[0]
    torch.cuda.synchronize()
    # float64 on the last head of the last batch item: the context, or dQ
    q1, k1, v1, g1 = (t[B - 1, :, H - 1].double() for t in (q, kk, v, d_out))
    p = torch.softmax(q1 @ k1.T * SCALE + (0.0 if side == "nobias" else mask.double()), dim=1)
    ref = p @ v1
    if what.endswith("_grad"):
        ref = (SCALE * p * (g1 @ v1.T - (g1 * ref).sum(1, keepdim=True))) @ k1
    err = float((got[B - 1, :, H - 1].double() - ref).abs().max() / ref.abs().max())
    t0, calls = time.perf_counter(), 0
    while time.perf_counter() - t0 < 0.3:     # warm-up: clocks
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
    return {"what": what, "shape": spec, "us": statistics.median(rounds), "min_us": min(rounds), "max_us": max(rounds), "err_vs_float64": err}


def child(what, spec, natural):
    env = dict(os.environ)
    if what.startswith("natural"):
        env["EG_LIB_PATH"] = natural
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", what, spec], capture_output=True, text=True, timeout=900, env=env)
    if out.returncode != 0:
        sys.exit("measurement %s %s failed (exit %d):\n%s" % (what, spec, out.returncode, out.stderr[-3000:]))
    return json.loads(out.stdout.strip().splitlines()[-1])


def report(runs):
    us = [r["us"] for r in runs]
    print(f"  {runs[0]['what']:13s} {statistics.median(us):9.1f} us per call (turns: {', '.join('%.1f' % t for t in us)}; spread {max(us) - min(us):.1f}), "
          f"err vs float64 {runs[-1]['err_vs_float64']:.1e}")
    return statistics.median(us), max(us) - min(us)


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv[:1] == ["--one"]:
        print(json.dumps(one(argv[1], argv[2])))
        sys.exit(0)
    natural = None
    if argv[:1] == ["--natural"]:
        natural, argv = os.path.abspath(argv[1]), argv[2:]
    sides = ["causal", "table", "nobias"] + (["natural"] if natural else [])
    for spec in argv or DEFAULT:
        T = int(spec.split("x")[2]) // 64
        runs = {side + tail: [] for tail in ("", "_grad") for side in sides}
        for _ in range(3):
            for what in runs:
                runs[what].append(child(what, spec, natural))
        print(f"attention, B x H x I x K = {spec} (J = I, D = K, offset 0), device events, median of {ROUNDS} rounds of at least {INNER} calls and "
              f"{ROUND_SECONDS} s, 3 turns of fresh processes; tile visits {T * (T + 1) // 2} of {T * T} = {(T + 1) / (2 * T):.3f}")
        for tail in ("", "_grad"):
            a, sa = report(runs["causal" + tail])
            for side in sides[1:]:
                b, sb = report(runs[side + tail])
                print(f"  causal{tail} / {side}{tail}: {a / b:.3f}x; difference {a - b:.1f} us against a spread of {max(sa, sb):.1f} us: "
                      f"{'outside' if abs(a - b) > max(sa, sb) else 'within'} the spread", flush=True)
