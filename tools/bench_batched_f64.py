#!/usr/bin/env python
"""eg_dgemm_batched against what a float64 caller had before it: a host loop of eg_dgemm calls, same process, same buffers,
measured in turns.  Per shape: us per call of each between two events on the stream (median of 7 rounds), the ratio
loop / batched, bit equality of the two results, and the error against numpy's float64 product on four items.

The two "forced" columns put the call on one side of the loop-or-batched rule (gemm_plan.cpp, dgemm_batched_runs_as_loop)
whatever the rule says — EG_DGEMM_BATCHED_ROUTE=launch | loop under EG_TUNING=1: the one launch of 64 x 64 tiles, and the
loop of plain products inside the library (no Python between the items).  They are what the rule's threshold is set from.

Then the model route: the step of the batched-form training program in float64 with eg_bgemm launches and with
EG_NO_BATCHED_GEMM=1 (the generated kernels), as HOST WALL TIME per step over 30 steps and a final sync: it holds the
Python and launch overhead of a step, the same both ways.

tools/bench_batched_f64.py [--commit ID] [BxMxNxK ...]
    default shapes: the four of DESIGN.md section 3 "Batched products" and three around the rule's threshold, sized from
    the device's compute units (16 tile columns; one tile row less than, exactly, one more than a tile per CU)."""
import ctypes
import os
import platform
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
os.environ["EG_TUNING"] = "1"
os.environ.pop("EG_DGEMM_BATCHED_ROUTE", None)
import numpy as np
import torch
import exprgrad_amd as eg
from exprgrad_amd import dsl, layers, ops, _lib, model as egm

TABLE = ["512x128x128x64", "64x512x512x64", "4096x32x32x32", "8x2048x2048x256"]
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
ctx = eg.newGpuContext(0, stream=stream.cuda_stream)


def device():
    cu, clock, hbm = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    arch = ctypes.create_string_buffer(64)
    _lib.call("eg_device_props", 0, ctypes.byref(cu), ctypes.byref(clock), ctypes.byref(hbm), arch, 64)
    return cu.value, clock.value, arch.value.decode()


def threshold_shapes(cus):
    rows = -(-cus // 16)
    return ["8x%dx1024x64" % (64 * r) for r in (rows - 1, rows, rows + 1)]


def route(value):
    if value:
        os.environ["EG_DGEMM_BATCHED_ROUTE"] = value
    else:
        os.environ.pop("EG_DGEMM_BATCHED_ROUTE", None)
    _lib.reload_switches()


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
    A = torch.rand((batch, M, K), device="cuda", dtype=torch.float64) - 0.5
    B = torch.rand((batch, K, N), device="cuda", dtype=torch.float64) - 0.5
    C1, C2 = (torch.empty((batch, M, N), device="cuda", dtype=torch.float64) for _ in range(2))
    batched = lambda: ops.dgemm_batched(ctx, batch, M, N, K, A, K, M * K, B, N, K * N, C1, N, M * N)
    pa, pb, pc = A.data_ptr(), B.data_ptr(), C2.data_ptr()
    null = ctypes.c_void_p(0)

    def loop():
        for b in range(batch):
            _lib.call("eg_dgemm", ctx.handle, 0, 0, M, N, K, ctypes.c_void_p(pa + 8 * b * M * K), K, ctypes.c_void_p(pb + 8 * b * K * N), N,
                      ctypes.c_void_p(pc + 8 * b * M * N), N, 0, null)
    inner = max(1, min(20, 2000 // batch))
    variants = [("batched", None, batched, inner * 4), ("loop", None, loop, inner), ("launch", "launch", batched, inner * 4), ("inner", "loop", batched, inner)]
    for _, r, run, _ in variants:       # warm-up: lazy builds, clocks
        route(r)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.05:
            run()
            torch.cuda.synchronize()
    times = {name: [] for name, _, _, _ in variants}
    for _ in range(7):                # in turns, so that a drift of the clocks hits all alike
        for name, r, run, n in variants:
            route(r)
            times[name].append(timed(run, n))
    route(None)
    batched()
    loop()
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in times.items()}
    same = bool(torch.equal(C1, C2))
    ref = torch.from_numpy(A[:4].cpu().numpy() @ B[:4].cpu().numpy())
    err = ((C1[:4].cpu() - ref).abs().max() / ref.abs().max()).item()
    print(f"{spec}: batched {med['batched']:9.1f} us  loop of eg_dgemm {med['loop']:9.1f} us  loop/batched {med['loop'] / med['batched']:7.2f}  "
          f"| forced one launch {med['launch']:9.1f}  forced loop inside the library {med['inner']:9.1f}  "
          f"| {2.0 * batch * M * N * K / med['batched'] / 1e6:5.1f} TFLOP/s  err vs numpy float64 {err:.1e}  "
          f"{'same bits as the loop' if same else 'bits differ from the loop (eg_dgemm took k-slices)'}", flush=True)


def training_program(G, I, J, K, rate):
    """out[g,i,j] ++= a[g,i,k] * b[g,k,j] with both operands parameters: the step holds the product and both its gradients."""
    g, i, j, k = dsl.iters("g i j k")
    a, b = dsl.param([G, I, K], name="a"), dsl.param([G, K, J], name="b")
    out = dsl.Fun()
    out[g, i, j] += a[g, i, k] * b[g, k, j]
    loss = layers.mse(out, dsl.input("labels")).target("loss")
    return [out.target("out"), loss.backwards().optimize([a, b], layers.gradient_descent(rate)).target("fit")]


def bench_model(G=64, I=128, J=128, K=64, steps=30):
    labels = np.random.default_rng(0).random((G, I, J)) - 0.5
    out = {}
    for name, off in (("eg_bgemm launches", False), ("generated kernels (EG_NO_BATCHED_GEMM=1)", True)):
        if off:
            os.environ["EG_NO_BATCHED_GEMM"] = "1"
        else:
            os.environ.pop("EG_NO_BATCHED_GEMM", None)
        _lib.reload_switches()
        m = egm.compile(*training_program(G, I, J, K, rate=1e-3), gpu=ctx, dtype=np.float64)
        for _ in range(5):
            m.apply("fit", {"labels": labels})
        ctx.sync()
        rounds = []
        for _ in range(7):
            t0 = time.perf_counter()
            for _ in range(steps):
                m.apply("fit", {"labels": labels})
            ctx.sync()
            rounds.append((time.perf_counter() - t0) / steps * 1e6)
        out[name] = statistics.median(rounds)
        print(f"float64 model step {G}x{I}x{J}x{K}, {name}: {out[name]:9.1f} us of HOST WALL TIME per step "
              f"({m.launch_plan('fit').count('eg_bgemm')} eg_bgemm launches)", flush=True)
        m.close()
    os.environ.pop("EG_NO_BATCHED_GEMM", None)
    _lib.reload_switches()
    a, b = out.values()
    print(f"float64 model step: generated / eg_bgemm = {b / a:.2f} (host wall time)", flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    commit = "unknown"
    if args[:1] == ["--commit"]:
        commit, args = args[1], args[2:]
    cus, clock, arch = device()
    print(f"eg_dgemm_batched against a host loop of eg_dgemm, and the float64 model route against its generated kernels.")
    print(f"commit {commit}; box {platform.node()}: {torch.cuda.get_device_name(0)} ({arch}, {cus} CUs, {clock / 1e3:.0f} MHz), torch {torch.__version__}")
    print("One process, the variants measured in turns, median of 7 rounds per figure; us per call.", flush=True)
    for spec in args or TABLE + threshold_shapes(cus):
        bench_shape(spec)
    if not args:
        bench_model()
