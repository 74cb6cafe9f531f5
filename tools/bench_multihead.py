#!/usr/bin/env python
"""The multi-head scores product s[b,h,i,j] ++= q[b,i,h,k] * kk[b,j,h,k] as ONE `out` call of the model route, q and kk stored
[batch, seq, head, feat] and resident on the device (Model.apply: no upload, no read-back).  Time per call between two
events on the stream: warm-up first, then ROUNDS rounds of INNER calls each, the median of the rounds.

tools/bench_multihead.py [BxHxIxJxK]                 this checkout, with eg_bgemm2 and with EG_NO_BATCHED_GEMM=1
tools/bench_multihead.py --against DIR [BxHxIxJxK]   this checkout against the checkout in DIR (built; for instance the
                                                     parent commit, whose route is the generated kernel), in turns: every
                                                     measurement is a fresh process, this one first, three turns each
tools/bench_multihead.py --one DIR SHAPE             one measurement with the package of DIR, one JSON line (what the above run)

The first call's result is compared with the float64 product on one (batch, head) item."""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = "8x16x512x512x64"
ROUNDS, INNER = 9, 20


def one(root, spec):
    sys.path.insert(0, root)
    import time
    import numpy as np
    import torch
    import exprgrad_amd as eg
    from exprgrad_amd import dsl, model as egm
    B, H, I, J, K = (int(v) for v in spec.split("x"))
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = eg.newGpuContext(0, stream=stream.cuda_stream)
    b, h, i, j, k = dsl.iters("b h i j k")
    s = dsl.Fun()
    s[b, h, i, j] += dsl.input("q")[b, i, h, k] * dsl.input("kk")[b, j, h, k]
    m = egm.compile(s.target("out"), gpu=ctx)
    torch.manual_seed(0)
    q, kk = torch.rand((B, I, H, K), device="cuda") - 0.5, torch.rand((B, J, H, K), device="cuda") - 0.5
    args = {"q": q, "kk": kk}
    got = m.call("out", args)
    ref = q[B - 1, :, H - 1, :].double().cpu().numpy() @ kk[B - 1, :, H - 1, :].double().cpu().numpy().T
    err = float(np.max(np.abs(got[B - 1, H - 1] - ref)) / np.max(np.abs(ref)))
    run = lambda: m.apply("out", args)
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
    plan = [line for line in m.launch_plan("out").splitlines() if line.startswith("[")]
    m.close()
    return {"root": root, "shape": spec, "us": statistics.median(rounds), "min_us": min(rounds), "max_us": max(rounds), "err_vs_float64": err,
            "plan": plan, "tflops": 2.0 * B * H * I * J * K / statistics.median(rounds) / 1e6}


def child(root, spec, env=None):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", root, spec], capture_output=True, text=True,
                         env=dict(os.environ, **(env or {})), timeout=600)
    if out.returncode != 0:
        sys.exit("measurement with %s failed (exit %d):\n%s" % (root, out.returncode, out.stderr[-3000:]))
    return json.loads(out.stdout.strip().splitlines()[-1])


def report(name, runs):
    med = statistics.median(r["us"] for r in runs)
    print(f"{name}: {med:9.1f} us per call (turns: {', '.join('%.1f' % r['us'] for r in runs)}; rounds of the last turn "
          f"{runs[-1]['min_us']:.1f} .. {runs[-1]['max_us']:.1f}), {runs[-1]['tflops']:.1f} TFLOP/s, err vs float64 {runs[-1]['err_vs_float64']:.1e}")
    print("    " + " | ".join(runs[-1]["plan"]), flush=True)
    return med


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv[:1] == ["--one"]:
        print(json.dumps(one(os.path.abspath(argv[1]), argv[2])))
        sys.exit(0)
    other = None
    if argv[:1] == ["--against"]:
        other, argv = os.path.abspath(argv[1]), argv[2:]
    spec = argv[0] if argv else DEFAULT
    sides = [("this checkout, eg_bgemm2", HERE, None)]
    sides.append(("the checkout in %s" % other, other, None) if other else ("this checkout, EG_NO_BATCHED_GEMM=1", HERE, {"EG_NO_BATCHED_GEMM": "1"}))
    runs = {name: [] for name, _, _ in sides}
    for _ in range(3):              # in turns, so that a drift of the clocks hits both alike
        for name, root, env in sides:
            runs[name].append(child(root, spec, env))
    print(f"scores product {spec} (B x H x I x J x K), one `out` call of the model route, device events, median of {ROUNDS} rounds of {INNER} calls")
    new, old = (report(name, runs[name]) for name, _, _ in sides)
    print(f"ratio: {old / new:.2f}x ({sides[1][0]} / {sides[0][0]})")
