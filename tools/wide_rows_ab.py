"""A/B of a wide classification head between two builds of the library (profiles/wide_rows_ab.txt).

    python tools/wide_rows_ab.py --parent PATH/libexprgrad_hip.so [--out profiles/wide_rows_ab.txt]

Workload: dense(784 -> 512) -> relu -> dense(512 -> W) -> softmax -> crossEntropy -> gradientDescent, one training step on
device-resident inputs, B x W in 65536 x {100, 1000} and 4096 x {1000, 4096}.  Side A is the build at --parent (loaded
through EG_LIB_PATH), side B the in-tree build.  Every run is a fresh process: 5 warm-up steps, 20 timed ones between two
device synchronisations; the sides alternate A B A B A B.  One more run per side goes under `rocprofv3 --kernel-trace
--stats` (graphs off, so that every kernel is a row of the trace) for the summed time of the launches that are not
contractions.

Bytes of the chain (the [B, W] tensors its kernels stream; [B] and [W] operands are noise next to them), in passes of
B * W * 4 bytes, from the kernel list of Model.emit_ir() and the launches of Model.launch_plan():
  floor            3   logits and labels read once, the logits' gradient written once
  launch per kernel 15 sums r1 | softmax r1 w1 | loss gradient r2 w1 | gradient r2 w1 | sums' gradient r2 | gradient r1 rw2 | bias gradient r1
  one wide group   3   (W <= 2048: three row tensors and the bias gradient's accumulators fit 128 floats per lane)
  two wide groups  6   (2048 < W <= 4096: the loss gradient goes through memory between them)
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(65536, 100), (65536, 1000), (4096, 1000), (4096, 4096)]
HBM_BYTES_PER_S = 8e12


def child(batch, width, steps, warmup):
    sys.path.insert(0, ROOT)
    import numpy as np
    import exprgrad_amd as eg
    from exprgrad_amd import examples, model as egm
    ctx = eg.newGpuContext(0)
    m = egm.compile(*examples.dense_softmax_net(784, 512, width), gpu=ctx)
    rng = np.random.default_rng(0)
    for tid in m.params.ids():
        m.params[tid] = (rng.random(m.params[tid].shape, dtype=np.float32) * 0.2 - 0.1).astype(np.float32)
    x = rng.random((batch, 784), dtype=np.float32)
    y = np.zeros((batch, width), np.float32)
    y[np.arange(batch), rng.integers(0, width, batch)] = 1.0
    import torch
    args = {"x": torch.from_numpy(x).cuda(), "y": torch.from_numpy(y).cuda()}
    for _ in range(warmup):
        m.apply("train", args)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        m.apply("train", args)
    ctx.sync()
    step_us = (time.perf_counter() - t0) / steps * 1e6
    digest = float(np.sum(np.abs(np.asarray(m.params[m.params.ids()[-1]], np.float64))))
    print("RESULT " + json.dumps({"step_us": step_us, "plan": m.launch_plan("train"), "digest": digest}))


def run_child(lib, batch, width, steps, warmup, profile_dir=None):
    env = dict(os.environ)
    if lib:
        env["EG_LIB_PATH"] = lib
    else:
        env.pop("EG_LIB_PATH", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(batch), str(width), "--steps", str(steps), "--warmup", str(warmup)]
    if profile_dir:
        env["EG_NO_GRAPH"] = "1"
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", profile_dir, "-o", "t", "--"] + cmd
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit("run failed (%d): %s\n%s" % (out.returncode, " ".join(cmd), out.stderr[-2000:]))
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def kernel_stats(profile_dir):
    """name -> (calls, total us) from rocprofv3's kernel stats."""
    files = glob.glob(os.path.join(profile_dir, "**", "*kernel_stats.csv"), recursive=True)
    stats = {}
    for row in csv.DictReader(open(files[0])) if files else []:
        stats[row["Name"]] = (int(row["Calls"]), float(row["TotalDurationNs"]) / 1e3)
    return stats


def is_contraction(name):
    return "gemm" in name.lower() or "mfma" in name.lower()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2, type=int)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent", help="the parent build's libexprgrad_hip.so")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_rows_ab.txt"))
    ap.add_argument("--shapes", default="", help="BxW,BxW (default: the four of the module docstring)")
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.steps, a.warmup)
    if not a.parent or not os.path.exists(a.parent):
        raise SystemExit("--parent: the parent build's library is needed")
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")] if a.shapes else SHAPES
    lines = ["wide rows A/B: A = parent build, B = this build; step = dense(784->512)->relu->dense(512->W)->softmax->crossEntropy->GD",
             "%d timed steps after %d warm-up per run, fresh process per run, order A B A B A B" % (a.steps, a.warmup), ""]
    for batch, width in shapes:
        runs = {"A": [], "B": []}
        plans = {}
        for _ in range(3):
            for side, lib in (("A", a.parent), ("B", None)):
                r = run_child(lib, batch, width, a.steps, a.warmup)
                runs[side].append(r["step_us"])
                plans[side] = r
        prof = {}
        for side, lib in (("A", a.parent), ("B", None)):
            with tempfile.TemporaryDirectory() as d:
                run_child(lib, batch, width, a.steps, a.warmup, profile_dir=d)
                prof[side] = kernel_stats(d)
        per_step = float(a.steps + a.warmup)
        lines.append("== B = %d, W = %d" % (batch, width))
        for side in "AB":
            other = sum(us for name, (_, us) in prof[side].items() if not is_contraction(name)) / per_step
            lines.append("  %s step us: %s  (spread %.1f)   non-contraction launches, summed: %.1f us per step" % (
                side, "  ".join("%.1f" % v for v in runs[side]), max(runs[side]) - min(runs[side]), other))
        pass_bytes = batch * width * 4
        wide = {name: us / calls for name, (calls, us) in prof["B"].items() if "eg_wrows" in name}
        groups = len(wide)
        lines.append("  chain bytes: floor %.1f MB (3 passes), A %.1f MB (15 passes), B %.1f MB (%d passes in %d wide group(s))" % (
            3 * pass_bytes / 1e6, 15 * pass_bytes / 1e6, 3 * groups * pass_bytes / 1e6, 3 * groups, groups))
        for name, us in sorted(wide.items()):
            lines.append("  %s: %.1f us per launch = %.1f%% of 8 TB/s for its 3 passes (%.1f us at the floor rate)" % (
                name, us, 100.0 * 3 * pass_bytes / HBM_BYTES_PER_S / (us * 1e-6), 3 * pass_bytes / HBM_BYTES_PER_S * 1e6))
        lines.append("  parameter digest A %.9g  B %.9g" % (plans["A"]["digest"], plans["B"]["digest"]))
        lines.append("  plan A:")
        lines += ["    " + ln for ln in plans["A"]["plan"].splitlines()]
        lines.append("  plan B:")
        lines += ["    " + ln for ln in plans["B"]["plan"].splitlines()]
        lines.append("  A kernels (us per step): " + ", ".join("%s %.1f" % (n[:40], us / per_step) for n, (_, us) in sorted(prof["A"].items(), key=lambda kv: -kv[1][1])[:12]))
        lines.append("  B kernels (us per step): " + ", ".join("%s %.1f" % (n[:40], us / per_step) for n, (_, us) in sorted(prof["B"].items(), key=lambda kv: -kv[1][1])[:12]))
        lines.append("")
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines[-12:]), flush=True)


if __name__ == "__main__":
    main()
