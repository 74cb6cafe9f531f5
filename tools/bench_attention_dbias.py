#!/usr/bin/env python
"""eg_attention_bias_dbias beside eg_attention_bias_grad on the same tensors, everything resident on the device, operands stored
[batch, head, seq, feat], in three forms of the bias (and of its gradient):

  full      bias[b,h,i,j]: every block adds one item, the gradient is as large as the scores
  heads     bias[h,i,j]  (stride_b0 = 0): a block adds the B items of its head
  padding   bias[b,j]    (ldb = 0, stride_b1 = 0): the row fold; a block adds H items x all row tiles

  dbias     one eg_attention_bias_dbias call (kernels/attention_dbias_f32.hip: S and dP once per tile)
  grad      one eg_attention_bias_grad call  (kernels/attention_grad_f32.hip: dQ, dK and dV; S and dP in both of its kernels)

O and Sums come from one eg_attention_bias call before the clock starts.  Time per call between two events on the stream:
warm-up first, then ROUNDS rounds of INNER calls each, the median of the rounds.  Every measurement is a fresh process; the
sides run in turns, three turns each, so that a drift of the clocks hits both alike.  The spread of a side is the min-max range
of its turns.  dbias is also checked against float64 on the last item's cell.

tools/bench_attention_dbias.py [BxHxIxJxK ...]                     8x16x512x512x64 by default (D = K)
tools/bench_attention_dbias.py --one full|heads|padding dbias|grad SHAPE    one measurement, one JSON line"""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ["8x16x512x512x64"]
FORMS = ["full", "heads", "padding"]
ROUNDS, INNER = 9, 10
SCALE = 0.125


def one(form, what, spec):
    sys.path.insert(0, HERE)
    import time
    import numpy as np
    import torch
    import exprgrad_amd as eg
    from exprgrad_amd import ops
    B, H, I, J, K = [int(x) for x in spec.split("x")]
    D = K
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = eg.newGpuContext(0, stream=stream.cuda_stream)
    torch.manual_seed(0)
    q, kk, v, d_out = (torch.rand(s, device="cuda") - 0.5 for s in ((B, H, I, K), (B, H, J, K), (B, H, J, D), (B, H, I, D)))
    shape, view = {"full": ((B, H, I, J), (J, (H * I * J, I * J))), "heads": ((1, H, I, J), (J, (0, I * J))),
                   "padding": ((B, 1, 1, J), (0, (J, 0)))}[form]
    bias = torch.rand(shape, device="cuda") - 0.5
    out, sums = torch.empty((B, H, I, D), device="cuda"), torch.empty((B, H, I), device="cuda")
    dense = lambda t, rows, cols: (t, cols, (H * rows * cols, rows * cols))
    head = (ctx, B, H, I, J, K, D, SCALE, *dense(q, I, K), *dense(kk, J, K), *dense(v, J, D), *dense(out, I, D))
    ops.attention_bias(*head, sums, (H * I, I), bias, *view)
    err = 0.0
    if what == "dbias":
        db = torch.full(shape, float("nan"), device="cuda")
        run = lambda: ops.attention_bias_dbias(*head, sums, (H * I, I), *dense(d_out, I, D), bias, *view, db, *view)
        run()
        torch.cuda.synchronize()
        # float64 on the items of the last cell
        items = [(b, h) for b in (range(B) if shape[0] == 1 else [B - 1]) for h in (range(H) if shape[1] == 1 else [H - 1])]
        ref = 0.0
        for b, h in items:
            f = lambda t: t[b, h].double().cpu().numpy()
            e = np.exp(f(q) @ f(kk).T * SCALE + bias[b if shape[0] > 1 else 0, h if shape[1] > 1 else 0].double().cpu().numpy())
            p = e / e.sum(1, keepdims=True)
            g = p * (f(d_out) @ f(v).T - (f(d_out) * (p @ f(v))).sum(1, keepdims=True))
            ref = ref + (g.sum(0, keepdims=True) if shape[2] == 1 else g)
        got = db[-1, -1].cpu().numpy()
        err = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    else:
        dq, dk, dv = torch.empty_like(q), torch.empty_like(kk), torch.empty_like(v)
        run = lambda: ops.attention_bias_grad(*head, sums, (H * I, I), *dense(d_out, I, D), *dense(dq, I, K), *dense(dk, J, K), *dense(dv, J, D),
                                              bias, *view)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3:     # warm-up: code objects, clocks
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
    products = 2 if what == "dbias" else 7   # 64 x 64 tile products per tile: S, dP | S, dP, dQ and S, dP, dV, dK
    return {"what": what, "form": form, "shape": spec, "us": statistics.median(rounds), "min_us": min(rounds), "max_us": max(rounds),
            "err_vs_float64": err, "flops": 2.0 * B * H * I * J * K * products, "dbias_mb": 4.0 * bias.numel() / 1e6}


def child(form, what, spec):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", form, what, spec], capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        sys.exit("measurement %s %s %s failed (exit %d):\n%s" % (form, what, spec, out.returncode, out.stderr[-3000:]))
    return json.loads(out.stdout.strip().splitlines()[-1])


def report(name, runs):
    us = [r["us"] for r in runs]
    med = statistics.median(us)
    print(f"  {name}: {med:9.1f} us per call (turns: {', '.join('%.1f' % x for x in us)}; spread {max(us) - min(us):.1f}; rounds of the last turn "
          f"{runs[-1]['min_us']:.1f} .. {runs[-1]['max_us']:.1f}), {runs[-1]['flops'] / med / 1e6:.1f} TFLOP/s of its products")
    return med, max(us) - min(us)


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv[:1] == ["--one"]:
        print(json.dumps(one(argv[1], argv[2], argv[3])))
        sys.exit(0)
    for spec in argv or DEFAULT:
        print(f"gradient of the score bias, {spec} (B x H x I x J x K, D = K), device events, median of {ROUNDS} rounds of {INNER} calls")
        for form in FORMS:
            runs = {"dbias": [], "grad": []}
            for _ in range(3):
                for what in runs:
                    runs[what].append(child(form, what, spec))
            r = runs["dbias"][-1]
            print(f"{form}: dBias {r['dbias_mb']:.2f} MB, err vs float64 {r['err_vs_float64']:.1e}")
            (db, s0), (grad, s1) = report("eg_attention_bias_dbias", runs["dbias"]), report("eg_attention_bias_grad ", runs["grad"])
            print(f"  dbias / grad = {db / grad:.2f} (spreads {s0:.1f} and {s1:.1f} us)", flush=True)
