"""float64 convolutions that only the implicit-GEMM kernel takes (csrc/kernels/conv2_f64_mfma.hip): each role through the C
entry points, and a one-layer model (conv2 -> mse -> gradientDescent) with the kernel on and with EG_CONV_NO_MFMA64=1 (the
generated kernels: the route of the commit before the kernel).  Each of the two model runs starts with its switches set: they
are child processes of this one call, alternating, three rounds each.

Method: warm-up launches, then events around `reps` launches on the context's stream; operands rotate through enough
sets that a launch never finds its inputs in the 256 MiB Infinity Cache from the launch before (sets * bytes > 512 MiB, at
most 8 sets), values uniform in [-1, 1).  Prints one line per measurement: microseconds (median and minimum of the rounds),
TFLOP/s and the fraction of the float64 matrix peak (78.6 TFLOP/s).

    python tools/conv64_general_bench.py            # all three shapes
    python tools/conv64_general_bench.py model N H W C F FH FW   # (internal) one model run in this process"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 78.6e12
SHAPES = [("config 4 in float64", (1, 256, 256, 64, 64, 3, 3)), ("mid layer", (32, 28, 28, 32, 64, 3, 3)), ("model test layer", (3, 12, 12, 24, 20, 3, 3))]
ROLES = ("forward", "grad_filter", "grad_image")


def flops(shape):
    N, H, W, C, F, FH, FW = shape
    return 2.0 * N * (H - FH + 1) * (W - FW + 1) * F * FH * FW * C


def timed(ctx, torch, launch, reps, rounds=5, warm=3):
    stream = torch.cuda.ExternalStream(ctx.stream)
    for i in range(warm):
        launch(i)
    ctx.sync()
    us = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for i in range(reps):
            launch(i)
        e1.record(stream)
        ctx.sync()
        us.append(e0.elapsed_time(e1) * 1e3 / reps)
    return float(np.median(us)), float(min(us))


def report(what, shape, us):
    med, best = us
    tf = flops(shape) / med / 1e6
    print(f"{what:<34s} {'x'.join(map(str, shape)):<24s} {med:9.1f} us (min {best:9.1f})  {tf:6.2f} TFLOP/s  {tf * 1e12 / PEAK:5.3f} of peak", flush=True)


def entry_points(ctx, torch, shape):
    from exprgrad_amd import ops
    N, H, W, C, F, FH, FW = shape
    Ho, Wo = H - FH + 1, W - FW + 1
    per_set = 8 * (N * H * W * C + F * FH * FW * C + N * Ho * Wo * F)
    sets = int(min(8, max(2, -(-(512 << 20) // per_set))))
    reps = 20 if flops(shape) > 1e9 else 200

    def rnd(*s):
        return torch.rand(s, device="cuda", dtype=torch.float64) * 2 - 1
    img = [rnd(N, H, W, C) for _ in range(sets)]
    flt = [rnd(F, FH, FW, C) for _ in range(sets)]
    out = [rnd(N, Ho, Wo, F) for _ in range(sets)]
    gflt, gimg = torch.empty_like(flt[0]), torch.empty_like(img[0])
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()
    calls = {
        "forward": lambda i: ops.conv2_nhwc_f64(ctx, *shape, p(img[i % sets]), p(flt[i % sets]), p(out[i % sets])),
        "grad_filter": lambda i: ops.conv2_nhwc_grad_filter_f64(ctx, *shape, p(img[i % sets]), p(out[i % sets]), p(gflt)),
        "grad_image": lambda i: ops.conv2_nhwc_grad_image_f64(ctx, *shape, p(flt[i % sets]), p(out[i % sets]), p(gimg)),
    }
    for role in ROLES:
        report(f"entry point {role} ({sets} sets)", shape, timed(ctx, torch, calls[role], reps))


def model_run(shape):
    """One process: the one-layer model's predict and train steps; prints a JSON line."""
    import torch
    import exprgrad_amd as eg
    from exprgrad_amd import dsl, layers
    from exprgrad_amd import model as egm
    N, H, W, C, F, FH, FW = shape
    ctx = eg.newGpuContext()
    out = layers.conv2(dsl.input("x"), C, FW, FH, F).target("predict")
    graphs = [layers.mse(out, dsl.input("y")).target("loss").backprop(layers.gradient_descent(0.01)).target("train")]
    m = egm.compile(*graphs, gpu=ctx, dtype=np.float64)
    x = torch.rand((N, H, W, C), device="cuda", dtype=torch.float64) * 2 - 1
    y = torch.rand((N, H - FH + 1, W - FW + 1, F), device="cuda", dtype=torch.float64) * 2 - 1
    reps = 10 if flops(shape) > 1e9 else 100
    res = {"predict": timed(ctx, torch, lambda i: m.apply("predict", {"x": x}), reps, rounds=3),
           "train": timed(ctx, torch, lambda i: m.apply("train", {"x": x, "y": y}), reps, rounds=3)}
    plan = m.launch_plan("train")
    res["mfma"] = "eg_conv64_mfma" in plan
    print("RESULT " + json.dumps(res), flush=True)


def model_pair(shape):
    rows = {"on": [], "off": []}
    for rnd in range(3):
        for mode in ("on", "off"):
            env = dict(os.environ)
            env.pop("EG_CONV_NO_MFMA64", None)
            if mode == "off":
                env["EG_CONV_NO_MFMA64"] = "1"
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "model", *map(str, shape)], env=env, capture_output=True, text=True,
                                 timeout=240)
            line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
            if out.returncode != 0 or not line:
                print("model run failed:", out.stdout[-500:], out.stderr[-1500:], flush=True)
                sys.exit(1)             # nothing more is started on the GPU after a failed child
            r = json.loads(line[0][7:])
            assert r["mfma"] == (mode == "on"), (mode, r)
            rows[mode].append(r)
    for target, factor in (("predict", 1.0), ("train", 3.0)):
        for mode in ("on", "off"):
            meds = [r[target][0] for r in rows[mode]]
            what = f"model {target}, kernel {mode}"
            med = float(np.median(meds))
            tf = factor * flops(shape) / med / 1e6
            print(f"{what:<34s} {'x'.join(map(str, shape)):<24s} {med:9.1f} us (runs {' '.join('%.1f' % v for v in meds)})  {tf:6.2f} TFLOP/s "
                  f"{tf * 1e12 / PEAK:5.3f} of peak", flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "model":
        return model_run(tuple(int(v) for v in sys.argv[2:9]))
    import torch
    import exprgrad_amd as eg
    print(torch.cuda.get_device_name(0), flush=True)
    ctx = eg.newGpuContext()
    for name, shape in SHAPES:
        print(f"-- {name}", flush=True)
        entry_points(ctx, torch, shape)
    ctx.sync()
    del ctx
    for name, shape in SHAPES:
        print(f"-- {name}: one-layer model, implicit-GEMM kernel on / off (EG_CONV_NO_MFMA64=1)", flush=True)
        model_pair(shape)


if __name__ == "__main__":
    main()
