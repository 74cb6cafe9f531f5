#!/usr/bin/env python
"""eg_sgemm_batched against what a caller had before it: a host loop of eg_sgemm calls on the exact path (EG_NO_SPLIT_GEMM=1),
same process, same buffers, measured in turns.  Per shape: us per call of each between two events on the stream (median of the
rounds), the ratio loop / batched, and bit equality of the two results where both sum k in order.  Then the model route: the
step of the batched-form training program with eg_bgemm launches and with EG_NO_BATCHED_GEMM=1 (the generated kernels), as
HOST WALL TIME per step over 30 steps and a final sync: it holds the Python and launch overhead of a step, the same both ways.

tools/bench_batched.py [BxMxNxK ...]      default: the four shapes of DESIGN.md section 3 "Batched products"."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
os.environ["EG_NO_SPLIT_GEMM"] = "1"
import numpy as np
import torch
import exprgrad_amd as eg
from exprgrad_amd import dsl, layers, ops, _lib, model as egm

SHAPES = ["512x128x128x64", "64x512x512x64", "4096x32x32x32", "8x2048x2048x256"]
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
ctx = eg.newGpuContext(0, stream=stream.cuda_stream)


def timed(run, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(stream)
    for _ in range(inner):
        run()
    e.record(stream)
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner * 1e3


def bench_shape(spec):
    batch, M, N, K = (int(v) for v in spec.split("x"))
    A = torch.rand((batch, M, K), device="cuda") - 0.5
    B = torch.rand((batch, K, N), device="cuda") - 0.5
    C1, C2 = torch.empty((batch, M, N), device="cuda"), torch.empty((batch, M, N), device="cuda")
    batched = lambda: ops.sgemm_batched(ctx, batch, M, N, K, A, K, M * K, B, N, K * N, C1, N, M * N)
    pa, pb, pc = A.data_ptr(), B.data_ptr(), C2.data_ptr()

    def loop():
        for b in range(batch):
            ops.sgemm(ctx, M, N, K, pa + 4 * b * M * K, K, pb + 4 * b * K * N, N, pc + 4 * b * M * N, N)
    inner = max(1, min(20, 2000 // batch))
    for run in (batched, loop):       # warm-up: lazy builds, clocks
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.1:
            run()
            torch.cuda.synchronize()
    times = {"batched": [], "loop": []}
    for _ in range(7):                # in turns, so that a drift of the clocks hits both alike
        times["batched"].append(timed(batched, inner * 4))
        times["loop"].append(timed(loop, inner))
    med = {k: statistics.median(v) for k, v in times.items()}
    same = bool(torch.equal(C1, C2))
    ref = A[:4].double() @ B[:4].double()
    err = ((C1[:4].double() - ref).abs().max() / ref.abs().max()).item()
    print(f"{spec}: batched {med['batched']:9.1f} us  loop of eg_sgemm {med['loop']:9.1f} us  loop/batched {med['loop'] / med['batched']:6.2f}  "
          f"| {2.0 * batch * M * N * K / med['batched'] / 1e6:6.1f} TFLOP/s  "
          f"err vs float64 {err:.1e}  {'same bits as the loop' if same else 'bits differ from the loop (its route does not sum k in order)'}", flush=True)


def training_program(G, I, J, K, rate):
    """out[g,i,j] ++= a[g,i,k] * b[g,k,j] with both operands parameters: the step holds the product and both its gradients."""
    g, i, j, k = dsl.iters("g i j k")
    a, b = dsl.param([G, I, K], name="a"), dsl.param([G, K, J], name="b")
    out = dsl.Fun()
    out[g, i, j] += a[g, i, k] * b[g, k, j]
    loss = layers.mse(out, dsl.input("labels")).target("loss")
    return [out.target("out"), loss.backwards().optimize([a, b], layers.gradient_descent(rate)).target("fit")]


def bench_model(G=64, I=128, J=128, K=64, steps=30):
    labels = (np.random.default_rng(0).random((G, I, J), dtype=np.float32) - 0.5).astype(np.float32)
    out = {}
    for name, off in (("eg_bgemm launches", False), ("generated kernels (EG_NO_BATCHED_GEMM=1)", True)):
        if off:
            os.environ["EG_NO_BATCHED_GEMM"] = "1"
        else:
            os.environ.pop("EG_NO_BATCHED_GEMM", None)
        _lib.reload_switches()
        m = egm.compile(*training_program(G, I, J, K, rate=1e-3), gpu=ctx)
        for _ in range(5):
            m.apply("fit", {"labels": labels})
        ctx.sync()
        rounds = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(steps):
                m.apply("fit", {"labels": labels})
            ctx.sync()
            rounds.append((time.perf_counter() - t0) / steps * 1e6)
        out[name] = statistics.median(rounds)
        print(f"model step {G}x{I}x{J}x{K}, {name}: {out[name]:9.1f} us of host wall time per step ({m.launch_plan('fit').count('eg_bgemm')} eg_bgemm launches)", flush=True)
        m.close()
    os.environ.pop("EG_NO_BATCHED_GEMM", None)
    _lib.reload_switches()
    a, b = out.values()
    print(f"model step: generated / eg_bgemm = {b / a:.2f} (wall time)", flush=True)


if __name__ == "__main__":
    for spec in sys.argv[1:] or SHAPES:
        bench_shape(spec)
    if len(sys.argv) == 1:
        bench_model()
