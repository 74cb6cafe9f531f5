#!/usr/bin/env python
"""Two measurements of the float64 fused attention forward (kernels/attention_f64.hip), per multi-head shape:

(a) eg_attention_f64 on device-resident [b,i,h,*] operands against its own matrix bound: the two products are 2 I J K and
    2 I J D flops per item, 2 I J (K + D) together (a multiply-add is two), at the float64 matrix peak of 78.6 TFLOP/s; the
    I J double exponentials per item are stated beside it, not folded into the bound.  (Counted as 4 I J (K + D) the entry
    would run above the peak at the larger shapes: that count has every multiply-add twice.)  Median [min .. max] of 7 rounds
    between two events on the stream.

(b) A compile[float64] model's forward chain (scores, scale, row sums of exp, softmax, context) with
    Model.fuse_attention_f64() — one eg_attn launch — against the same model on the best route it had before: Model.batched2_f64()
    alone, two eg_bgemm2 launches around three generated `double` kernels that write the I x J scores once and read and rewrite
    them twice more.  One process, both models alive, timed in turns: median of 7 rounds per side; the results are compared once.

Every shape runs in a fresh child process under a time limit of its own, one after the other; the first child that fails,
faults or runs out of time ends the run, and nothing more is started on the device.

tools/bench_attention_f64.py [--commit ID] [--shapes BxHxIxJxKxD,...] [--limit SECONDS]
tools/bench_attention_f64.py --child BxHxIxJxKxD          (one shape: the two measurements)"""
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

# B·H = 64 heads, I = J in {256, 1024}, K = D in {32, 64, 128}
SHAPES = ["4x16x%dx%dx%dx%d" % (n, n, k, k) for n in (256, 1024) for k in (32, 64, 128)]
PEAK_F64 = 78.6e12      # matrix FLOP/s of the MI355X in float64
SCALE = 0.125


def timed(torch, stream, run, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(stream)
    for _ in range(inner):
        run()
    e.record(stream)
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner * 1e3


def warm(torch, run, seconds=0.2):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        run()
        torch.cuda.synchronize()


def spread(v):
    return "%9.1f us [%.1f .. %.1f]" % (statistics.median(v), min(v), max(v))


def child(spec):
    import numpy as np
    import torch
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    import exprgrad_amd as eg
    from exprgrad_amd import dsl, model as egm, ops
    from exprgrad_amd.dsl import Fun, iters
    ctx = eg.newGpuContext(0, stream=stream.cuda_stream)
    B, H, I, J, K, D = (int(v) for v in spec.split("x"))
    torch.manual_seed(0)
    rand = lambda *shape: torch.rand(shape, device="cuda", dtype=torch.float64) - 0.5
    q, kk, v = rand(B, I, H, K), rand(B, J, H, K), rand(B, J, H, D)

    # ---- (a) the entry
    o = torch.empty((B, I, H, D), device="cuda", dtype=torch.float64)
    run = lambda: ops.attention_f64(ctx, B, H, I, J, K, D, SCALE, q, H * K, (I * H * K, K), kk, H * K, (J * H * K, K), v, H * D, (J * H * D, D), o,
                                    H * D, (I * H * D, D))
    warm(torch, run)
    inner = max(2, min(50, int(1e11 / (2.0 * B * H * I * J * (K + D)))))
    rounds = [timed(torch, stream, run, inner) for _ in range(7)]
    flops, exps = 2.0 * B * H * I * J * (K + D), float(B * H * I * J)
    bound = flops / PEAK_F64 * 1e6
    med = statistics.median(rounds)
    print(f"(a) eg_attention_f64 {spec}: {spread(rounds)}  matrix bound {bound:8.1f} us  bound / time {bound / med:5.3f}  "
          f"{flops / med / 1e6:5.1f} TFLOP/s  | {exps / 1e6:.1f} M exp, {exps / med / 1e3:.2f} G exp/s", flush=True)

    # ---- (b) the model's forward
    def graphs():
        b, h, i, j, k, d = iters("b h i j k d")
        s, e, sums, p, out = Fun(), Fun(), Fun(), Fun(), Fun()
        s[b, h, i, j] += dsl.input("q")[b, i, h, k] * dsl.input("kk")[b, j, h, k]
        e[b, h, i, j] += s[b, h, i, j] * SCALE
        sums[b, h, i] += dsl.exp(e[b, h, i, j])
        p[b, h, i, j] += dsl.exp(e[b, h, i, j]) / sums[b, h, i]
        out[b, i, h, d] += p[b, h, i, j] * dsl.input("v")[b, j, h, d]
        return [out.target("out")]

    inputs = {"q": q, "kk": kk, "v": v}
    models = {}
    for side in ("eg_bgemm2 + generated", "eg_attn"):
        m = egm.compile(*graphs(), gpu=ctx, dtype=np.float64)
        m.batched2_f64()
        if side == "eg_attn":
            m.fuse_attention_f64()
        models[side] = m
    runs = {side: (lambda m=m: m.apply("out", inputs)) for side, m in models.items()}
    for side in runs:
        warm(torch, runs[side])
    plans = {side: m.launch_plan("out") for side, m in models.items()}
    assert "eg_attn" in plans["eg_attn"] and "eg_attn" not in plans["eg_bgemm2 + generated"] and plans["eg_bgemm2 + generated"].count("eg_bgemm2") == 2, plans
    times = {side: [] for side in runs}
    calls = max(2, min(20, int(4e9 / (B * H * I * J * 8.0 * 6))))
    for _ in range(7):                # in turns, so that a drift of the clocks hits both alike
        for side in runs:
            times[side].append(timed(torch, stream, runs[side], calls))
    out = {side: m.call("out", inputs) for side, m in models.items()}
    err = float(np.max(np.abs(out["eg_attn"] - out["eg_bgemm2 + generated"])) / np.max(np.abs(out["eg_bgemm2 + generated"])))
    a, b = statistics.median(times["eg_bgemm2 + generated"]), statistics.median(times["eg_attn"])
    print(f"(b) model forward    {spec}: eg_bgemm2 + generated {spread(times['eg_bgemm2 + generated'])}  eg_attn {spread(times['eg_attn'])}  "
          f"unfused / fused {a / b:6.2f}{'  SLOWER' if b > a else ''}  max |difference| / max |value| {err:.1e}  | "
          f"{8.0 * B * H * I * J * 3 / 2 ** 20:.0f} MiB of scores, scaled scores and softmax not allocated", flush=True)
    for m in models.values():
        m.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--child"]:
        child(args[1])
        sys.exit(0)
    commit, shapes, limit = "unknown", SHAPES, 240
    while args:
        if args[0] == "--commit":
            commit, args = args[1], args[2:]
        elif args[0] == "--shapes":
            shapes, args = args[1].split(","), args[2:]
        elif args[0] == "--limit":
            limit, args = int(args[1]), args[2:]
        else:
            raise SystemExit(__doc__)
    print("Float64 fused attention forward: eg_attention_f64 against its matrix bound (2 I J (K + D) flops per item at 78.6 TFLOP/s), and a")
    print("model's forward with Model.fuse_attention_f64() against Model.batched2_f64() alone.  B x H x I x J x K x D; median [min .. max] of 7 rounds.")
    print(f"commit {commit}", flush=True)
    for spec in shapes:       # one fresh process per shape, each under its own limit; the first failure ends the run
        try:
            out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", spec], text=True,
                                 capture_output=True)
        except OSError as e:
            raise SystemExit("could not start the child for %s: %s" % (spec, e))
        sys.stdout.write(out.stdout)
        sys.stdout.flush()
        if out.returncode != 0:
            raise SystemExit("%s: the child ended with status %d; nothing more is started\n%s" % (spec, out.returncode, out.stderr[-3000:]))
