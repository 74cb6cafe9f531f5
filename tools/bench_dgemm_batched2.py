#!/usr/bin/env python
"""Two measurements of the float64 batched products (kernels/gemm_f64_mfma.hip), each as A/B in turns on one box in one call:

(a) The model route of Model.batched2_f64() against the generated kernel it replaces.  Three programs of one product each —
    the multi-head scores product and the two gradients derive makes of it —
        forward  s[b,h,i,j]  ++= q[b,i,h,k]  * kk[b,j,h,k]      NT
        dq       dq[b,i,h,k] ++= gs[b,h,i,j] * kk[b,j,h,k]      NN
        dk       dk[b,j,h,k] ++= gs[b,h,i,j] * q[b,i,h,k]       TN
    at (B, H, I, J, K), as the `out` target of a compile[float64] model over device-resident inputs.  A is the model with the
    setting off (one generated kernel, one work-item per output element: what every float64 model ran before the setting
    existed), B the model with it on (one eg_bgemm2 launch).  One process, both models alive, timed in turns between two
    events on the stream: median of 7 rounds per side, each round `calls` calls; the results are compared once.

(b) eg_dgemm_batched of this build against another build of the library (--against LIB: the commit before the two-index entry,
    to show that the one-index entry, which shares the launcher and the planner with it, kept its time), at the shapes
    of profiles/batched_gemm.txt.  A library is chosen when a process starts (EG_LIB_PATH), so the turns are fresh child
    processes, this build and the other one alternating (which of the two goes first alternates too), three turns a side; per turn
    the median of 7 rounds.  Per shape: the
    three medians of each side and each side's spread (max - min of its turns), so that a difference can be read against what
    repeated runs of one build show.

tools/bench_dgemm_batched2.py [--commit ID] [--against LIB] [--dims B,H,I,J,K] [--skip-models]
tools/bench_dgemm_batched2.py --child              (one turn of (b): `shape us` per line)"""
import ctypes
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

SHAPES = ["512x128x128x64", "64x512x512x64", "4096x32x32x32", "8x2048x2048x256"]     # profiles/batched_gemm.txt
LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "exprgrad_amd", "lib", "libexprgrad_hip.so")
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
if "--child" not in sys.argv[1:]:     # a child binds the three entries it calls by hand: the other build lacks symbols this tree's _lib resolves
    import exprgrad_amd as eg
    from exprgrad_amd import dsl, _lib, model as egm
    from exprgrad_amd.dsl import Fun, iters
    ctx = eg.newGpuContext(0, stream=stream.cuda_stream)


def device():
    cu, clock, hbm = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    arch = ctypes.create_string_buffer(64)
    _lib.call("eg_device_props", 0, ctypes.byref(cu), ctypes.byref(clock), ctypes.byref(hbm), arch, 64)
    return cu.value, clock.value, arch.value.decode()


def timed(run, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(stream)
    for _ in range(inner):
        run()
    e.record(stream)
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner * 1e3


def warm(run, seconds=0.2):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        run()
        torch.cuda.synchronize()


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------
def forward():
    b, h, i, j, k = iters("b h i j k")
    s = Fun()
    s[b, h, i, j] += dsl.input("q")[b, i, h, k] * dsl.input("kk")[b, j, h, k]
    return [s.target("out")]


def grad_q():
    b, h, i, j, k = iters("b h i j k")
    g = Fun()
    g[b, i, h, k] += dsl.input("gs")[b, h, i, j] * dsl.input("kk")[b, j, h, k]
    return [g.target("out")]


def grad_k():
    b, h, i, j, k = iters("b h i j k")
    g = Fun()
    g[b, j, h, k] += dsl.input("gs")[b, h, i, j] * dsl.input("q")[b, i, h, k]
    return [g.target("out")]


def bench_models(B, H, I, J, K, calls=10):
    rand = lambda *shape: torch.rand(shape, device="cuda", dtype=torch.float64) - 0.5
    q, kk, gs = rand(B, I, H, K), rand(B, J, H, K), rand(B, H, I, J)
    forms = [("forward NT", forward, {"q": q, "kk": kk}), ("dq NN", grad_q, {"gs": gs, "kk": kk}), ("dk TN", grad_k, {"gs": gs, "q": q})]
    flops = 2.0 * B * H * I * J * K
    slower = []
    for name, graphs, inputs in forms:
        models = {}
        for side, on in (("generated", False), ("eg_bgemm2", True)):
            m = egm.compile(*graphs(), gpu=ctx, dtype=np.float64)
            if on:
                m.batched2_f64()
            models[side] = m
        run = {side: (lambda m=m: m.apply("out", inputs)) for side, m in models.items()}
        for side in run:
            warm(run[side])
        plans = {side: m.launch_plan("out") for side, m in models.items()}
        assert "eg_bgemm2" in plans["eg_bgemm2"] and "generated" in plans["generated"] and "eg_bgemm" not in plans["generated"], plans
        times = {side: [] for side in run}
        for _ in range(7):                # in turns, so that a drift of the clocks hits both alike
            for side in run:
                times[side].append(timed(run[side], calls))
        out = {side: m.call("out", inputs) for side, m in models.items()}
        err = float(np.max(np.abs(out["eg_bgemm2"] - out["generated"])) / np.max(np.abs(out["generated"])))
        med = {side: statistics.median(v) for side, v in times.items()}
        lo, hi = {s: min(v) for s, v in times.items()}, {s: max(v) for s, v in times.items()}
        line = plans["eg_bgemm2"].splitlines()[0]
        print(f"{name:10s} {B}x{H} x {I}x{J}x{K}: generated {med['generated']:9.1f} us [{lo['generated']:.1f} .. {hi['generated']:.1f}]  "
              f"eg_bgemm2 {med['eg_bgemm2']:9.1f} us [{lo['eg_bgemm2']:.1f} .. {hi['eg_bgemm2']:.1f}]  generated / eg_bgemm2 "
              f"{med['generated'] / med['eg_bgemm2']:6.2f}  | {flops / med['eg_bgemm2'] / 1e6:5.1f} TFLOP/s  max |difference| / max |value| {err:.1e}  | {line}",
              flush=True)
        if med["eg_bgemm2"] > med["generated"]:
            slower.append(name)
        for m in models.values():
            m.close()
    print("the route is slower than the generated kernel on: " + (", ".join(slower) if slower else "none of the three forms"), flush=True)


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------
def child():
    """One turn of (b) on the library EG_LIB_PATH names (default: this tree's), through ctypes alone."""
    lib = ctypes.CDLL(os.environ.get("EG_LIB_PATH") or LIB)
    i64, ptr = ctypes.c_int64, ctypes.c_void_p
    lib.eg_ctx_create_on_stream.argtypes = [ctypes.c_int, ptr, ctypes.POINTER(ptr)]
    lib.eg_dgemm_batched.argtypes = [ptr, ctypes.c_int, ctypes.c_int, i64, i64, i64, i64, ptr, i64, i64, ptr, i64, i64, ptr, i64, i64, ctypes.c_int, ptr]
    handle = ptr()
    if lib.eg_ctx_create_on_stream(0, ptr(stream.cuda_stream), ctypes.byref(handle)) != 0:
        raise SystemExit("eg_ctx_create_on_stream failed")

    def dgemm_batched(batch, M, N, K, A, lda, sa, B, ldb, sb, C, ldc, sc):
        if lib.eg_dgemm_batched(handle, 0, 0, batch, M, N, K, ptr(A.data_ptr()), lda, sa, ptr(B.data_ptr()), ldb, sb, ptr(C.data_ptr()), ldc, sc, 0, None) != 0:
            raise SystemExit("eg_dgemm_batched failed")
    torch.manual_seed(0)
    for spec in SHAPES:
        batch, M, N, K = (int(v) for v in spec.split("x"))
        A = torch.rand((batch, M, K), device="cuda", dtype=torch.float64) - 0.5
        Bm = torch.rand((batch, K, N), device="cuda", dtype=torch.float64) - 0.5
        C = torch.empty((batch, M, N), device="cuda", dtype=torch.float64)
        run = lambda: dgemm_batched(batch, M, N, K, A, K, M * K, Bm, N, K * N, C, N, M * N)
        warm(run)
        inner = max(4, min(80, 8000 // batch))
        rounds = [timed(run, inner) for _ in range(7)]
        print(f"{spec} {statistics.median(rounds):.2f} {float(C.sum().item())!r}", flush=True)


def bench_against(other, turns=3):
    sides = {"this build": os.environ.get("EG_LIB_PATH"), "other build": other}      # this build: the library this process runs on
    got = {side: {s: [] for s in SHAPES} for side in sides}
    sums = {side: {} for side in sides}
    for turn in range(turns):
        order = list(sides.items())
        for side, lib in (order if turn % 2 == 0 else order[::-1]):      # this, other | other, this | ...: neither side always runs first
            env = dict(os.environ)
            env.pop("EG_LIB_PATH", None)
            if lib:
                env["EG_LIB_PATH"] = lib
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit("a turn of %s failed (exit %d): %s" % (side, out.returncode, out.stderr[-2000:]))
            for line in out.stdout.splitlines():
                spec, us, total = line.split()
                got[side][spec].append(float(us))
                sums[side][spec] = total
    print(f"eg_dgemm_batched, us per call: {turns} turns a side of fresh processes in turns, per turn the median of 7 rounds; spread = max - min of a side's turns")
    for spec in SHAPES:
        a, b = got["this build"][spec], got["other build"][spec]
        fmt = lambda v: " / ".join("%.1f" % x for x in v)
        same = "same sum of C" if sums["this build"][spec] == sums["other build"][spec] else "sums of C differ"
        print(f"{spec}: this build {fmt(a)} (median {statistics.median(a):.1f}, spread {max(a) - min(a):.1f})  other build {fmt(b)} "
              f"(median {statistics.median(b):.1f}, spread {max(b) - min(b):.1f})  this - other {statistics.median(a) - statistics.median(b):+.1f} us  {same}",
              flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--child"]:
        child()
        sys.exit(0)
    commit, other, dims, models = "unknown", None, (8, 16, 512, 512, 64), True
    while args:
        if args[0] == "--commit":
            commit, args = args[1], args[2:]
        elif args[0] == "--against":
            other, args = os.path.abspath(args[1]), args[2:]
        elif args[0] == "--skip-models":
            models, args = False, args[1:]
        elif args[0] == "--dims":
            dims, args = tuple(int(v) for v in args[1].split(",")), args[2:]
        else:
            raise SystemExit(__doc__)
    cus, clock, arch = device()
    print("Float64 products with two batch indices: the model route against the generated kernel, and eg_dgemm_batched against another build.")
    print(f"commit {commit}; {torch.cuda.get_device_name(0)} ({arch}, {cus} CUs, {clock / 1e3:.0f} MHz), torch {torch.__version__}")
    if models:
        print("(a) one process, the two models in turns, median [min .. max] of 7 rounds of 10 calls between events; us per call", flush=True)
        bench_models(*dims)
    if other:
        print(f"(b) against {os.path.basename(os.path.dirname(other)) or other}", flush=True)
        bench_against(other)
