#!/usr/bin/env python
"""The float64 fused attention backward (kernels/attention_grad_f64.hip) per multi-head shape, on device-resident [b,i,h,*]
operands, two sides timed in turns in one process:

  fused     eg_attention_sums_f64 + eg_attention_grad_f64: the forward that leaves O and the row sums, then the two backward
            launches.  The pair eg_attention_grad_f64 alone is timed too, against its matrix bound: S and dP are computed in
            both kernels, so the products are 2 I J (4 K + 3 D) flops per item at the float64 matrix peak of 78.6 TFLOP/s; the
            2 I J double exponentials per item are stated beside it, not folded into the bound.
  products  the same gradients' four products alone, as eg_dgemm_batched2 calls on stored I x J matrices: dP = dO V^T,
            dV = P^T dO, dQ = dS Kk, dK = dS^T Q.  A lower bound on the unfused route, which also has the forward, the softmax
            and its gradient to run, and stores P, dP and dS as B H I J doubles each.

Every shape runs in a fresh child process under a time limit of its own, one after the other; the first child that fails,
faults or runs out of time ends the run, and nothing more is started on the device.  Median [min .. max] of 7 rounds between
two events on the stream.

tools/bench_attention_grad_f64.py [--commit ID] [--shapes BxHxIxJxKxD,...] [--limit SECONDS]
tools/bench_attention_grad_f64.py --child BxHxIxJxKxD"""
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from bench_attention_f64 import PEAK_F64, SCALE, SHAPES, spread, timed, warm      # noqa: E402 (the forward's tool, beside this one)


def child(spec):
    import torch
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    import exprgrad_amd as eg
    from exprgrad_amd import ops
    ctx = eg.newGpuContext(0, stream=stream.cuda_stream)
    B, H, I, J, K, D = (int(v) for v in spec.split("x"))
    torch.manual_seed(0)
    rand = lambda *shape: torch.rand(shape, device="cuda", dtype=torch.float64) - 0.5
    empty = lambda *shape: torch.empty(shape, device="cuda", dtype=torch.float64)
    q, kk, v, d_out = rand(B, I, H, K), rand(B, J, H, K), rand(B, J, H, D), rand(B, I, H, D)
    o, sums, dq, dk, dv = empty(B, I, H, D), empty(B, H, I), empty(B, I, H, K), empty(B, J, H, K), empty(B, J, H, D)
    row = lambda R, C: (H * C, (R * H * C, C))       # (ld, strides) of a [b, r, h, c] operand
    qv, kv, vv, ov = (q,) + row(I, K), (kk,) + row(J, K), (v,) + row(J, D), (o,) + row(I, D)
    forward = lambda: ops.attention_sums_f64(ctx, B, H, I, J, K, D, SCALE, *qv, *kv, *vv, *ov, sums, (H * I, I))
    grad = lambda: ops.attention_grad_f64(ctx, B, H, I, J, K, D, SCALE, *qv, *kv, *vv, *ov, sums, (H * I, I), d_out, *row(I, D), dq, *row(I, K), dk,
                                          *row(J, K), dv, *row(J, D))

    def fused():
        forward()
        grad()

    # the four products on stored [b, h, i, j] matrices (their values do not matter to the time)
    p, ds, dp = rand(B, H, I, J), rand(B, H, I, J), empty(B, H, I, J)
    mat = (J, (H * I * J, I * J))

    def products():
        ops.dgemm_batched2(ctx, B, H, I, J, D, d_out, *row(I, D), v, *row(J, D), dp, *mat, trans_b=True)
        ops.dgemm_batched2(ctx, B, H, J, D, I, p, *mat, d_out, *row(I, D), dv, *row(J, D), trans_a=True)
        ops.dgemm_batched2(ctx, B, H, I, K, J, ds, *mat, kk, *row(J, K), dq, *row(I, K))
        ops.dgemm_batched2(ctx, B, H, J, K, I, ds, *mat, q, *row(I, K), dk, *row(J, K), trans_a=True)

    sides = {"fused": fused, "grad": grad, "products": products}
    for run in sides.values():
        warm(torch, run)
    flops, exps = 2.0 * B * H * I * J * (4 * K + 3 * D), 2.0 * B * H * I * J
    inner = max(2, min(50, int(1e11 / flops)))
    times = {side: [] for side in sides}
    for _ in range(7):                # in turns, so that a drift of the clocks hits all alike
        for side, run in sides.items():
            times[side].append(timed(torch, stream, run, inner))
    med = {side: statistics.median(t) for side, t in times.items()}
    bound = flops / PEAK_F64 * 1e6
    print(f"{spec}: sums + grad {spread(times['fused'])}  four products {spread(times['products'])}  products / fused "
          f"{med['products'] / med['fused']:5.2f}{'  SLOWER' if med['fused'] > med['products'] else ''}", flush=True)
    print(f"{spec}: grad alone  {spread(times['grad'])}  matrix bound {bound:8.1f} us  bound / time {bound / med['grad']:5.3f}  "
          f"{flops / med['grad'] / 1e6:5.1f} TFLOP/s  | {exps / 1e6:.1f} M exp  | {8.0 * B * H * I * J * 3 / 2 ** 20:.0f} MiB of P, dP and dS not stored",
          flush=True)


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
    print("Float64 fused attention backward: eg_attention_sums_f64 + eg_attention_grad_f64 against the gradients' four eg_dgemm_batched2")
    print("products alone, and the backward pair against its matrix bound (2 I J (4 K + 3 D) flops per item at 78.6 TFLOP/s).")
    print("B x H x I x J x K x D; median [min .. max] of 7 rounds, the sides in turns.")
    print(f"commit {commit}", flush=True)
    for spec in shapes:       # one fresh process per shape, each under its own limit; the first failure ends the run
        out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", spec], text=True,
                             capture_output=True)
        sys.stdout.write(out.stdout)
        sys.stdout.flush()
        if out.returncode != 0:
            raise SystemExit("%s: the child ended with status %d; nothing more is started\n%s" % (spec, out.returncode, out.stderr[-3000:]))
