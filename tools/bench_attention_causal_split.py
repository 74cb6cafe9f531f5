#!/usr/bin/env python
"""eg_attention_causal_split at chunk = 1, 2, 4, ... up to the longest row tile and at the auto rule (chunk = 0) against
eg_attention_causal in the same build, and against eg_attention_stable_split without a mask (its auto rule) as what the call
costs where the mask hides little.  q, kk, v are U[-0.5, 0.5), stored [1, seq, head, feat] and resident on the device; every
entry stores its Stats.

Time per call between two events on the stream: warm-up first, then ROUNDS rounds of at least INNER calls and ROUND_SECONDS of
work each, the median of the rounds.  A turn is a fresh process that measures every side of one shape, one after the other;
three turns per shape, so a drift of the clocks hits all sides alike.  A side's figure is the median of its turns and its spread
their min-max range; two sides differ when the difference exceeds the larger of the two spreads.

tools/bench_attention_causal_split.py [HEADSxIxJxKxOFFSET ...]   K = D; the six shapes of profiles/attention_causal_split.txt by default
tools/bench_attention_causal_split.py --turn SHAPE               one turn, one JSON line"""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ["128x512x512x64x0", "128x2048x2048x64x0", "32x128x8192x128x8064", "32x16x8192x128x8176", "32x1x8192x128x8191", "8x16384x16384x64x0"]
ROUNDS, INNER, ROUND_SECONDS, WARM_SECONDS = 9, 10, 0.03, 0.15
SCALE = 0.125


def sides(I, J, offset):
    longest = (min(J, I + offset) + 63) // 64
    return ["causal", "unmasked split", "auto"] + ["chunk %d" % (1 << n) for n in range(longest.bit_length()) if (1 << n) <= longest]


def turn(spec):
    sys.path.insert(0, HERE)
    import time
    import torch
    import exprgrad_amd as eg
    from exprgrad_amd import ops
    H, I, J, K, offset = [int(x) for x in spec.split("x")]
    D = K
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = eg.newGpuContext(0, stream=stream.cuda_stream)
    torch.manual_seed(0)
    q, kk, v = (torch.rand(s, device="cuda") - 0.5 for s in ((1, I, H, K), (1, J, H, K), (1, J, H, D)))
    out, stats = torch.full((1, I, H, D), float("nan"), device="cuda"), torch.zeros((1, H, 2, I), device="cuda")
    rows = lambda t, n, w: (t, H * w, (n * H * w, w))
    x = rows(q, I, K) + rows(kk, J, K) + rows(v, J, D) + rows(out, I, D) + (stats, I, (H * 2 * I, 2 * I))
    rows_ref = slice(max(0, I - 256), I)   # float64, the last head, its last rows: the longest key ranges
    q1, k1, v1 = (t[0, :, H - 1].double() for t in (q, kk, v))
    masked = torch.arange(J, device="cuda")[None, :] > torch.arange(I, device="cuda")[rows_ref, None] + offset
    ref = torch.softmax((q1[rows_ref] @ k1.T * SCALE).masked_fill(masked, float("-inf")), dim=1) @ v1
    result = {}
    for side in sides(I, J, offset):
        if side == "causal":
            run = lambda: ops.attention_causal(ctx, 1, H, I, J, K, D, SCALE, *x, offset=offset)
        elif side == "unmasked split":
            run = lambda: ops.attention_stable_split(ctx, 1, H, I, J, K, D, SCALE, *x, splits=0)
        else:
            n = 0 if side == "auto" else int(side.split()[1])
            run = lambda: ops.attention_causal_split(ctx, 1, H, I, J, K, D, SCALE, *x, offset=offset, chunk=n)
        out.fill_(float("nan"))
        run()
        torch.cuda.synchronize()
        err = float((out[0, rows_ref, H - 1].double() - ref).abs().max() / ref.abs().max())
        t0, calls = time.perf_counter(), 0
        while time.perf_counter() - t0 < WARM_SECONDS:
            run()
            torch.cuda.synchronize()
            calls += 1
        inner = max(INNER, min(1000, int(ROUND_SECONDS * calls / WARM_SECONDS)))
        rounds = []
        for _ in range(ROUNDS):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(stream)
            for _ in range(inner):
                run()
            end.record(stream)
            torch.cuda.synchronize()
            rounds.append(start.elapsed_time(end) / inner * 1e3)
        result[side] = {"us": statistics.median(rounds), "err": err}
    return result


def child(spec):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--turn", spec], capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        sys.exit("turn %s failed (exit %d):\n%s" % (spec, out.returncode, out.stderr[-3000:]))
    return json.loads(out.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv[:1] == ["--turn"]:
        print(json.dumps(turn(argv[1])))
        sys.exit(0)
    for spec in argv or DEFAULT:
        turns = [child(spec) for _ in range(3)]
        print(f"causal attention, heads x I x J x K x offset = {spec} (D = K), device events, median of {ROUNDS} rounds of at least {INNER} calls and "
              f"{ROUND_SECONDS} s, 3 turns of fresh processes")
        med, spread = {}, {}
        for side in turns[0]:
            us = [t[side]["us"] for t in turns]
            med[side], spread[side] = statistics.median(us), max(us) - min(us)
        best = min((s for s in med if s.startswith("chunk")), key=med.get)
        for side in turns[0]:
            print(f"  {side:14s} {med[side]:9.1f} us per call (turns: {', '.join('%.1f' % t[side]['us'] for t in turns)}; spread {spread[side]:.1f}), "
                  f"{med[side] / med['causal']:.3f} of causal, err vs float64 {turns[-1][side]['err']:.1e}")
        gap, room = med["auto"] - med[best], max(spread["auto"], spread[best])
        print(f"  best: {best}; auto - best: {gap:.1f} us against a spread of {room:.1f} us: {'within' if gap <= room else 'outside'} the spread")
        gain, room = med["causal"] - med[best], max(spread["causal"], spread[best])
        print(f"  causal - best: {gain:.1f} us against a spread of {room:.1f} us: {'a gain' if gain > room else 'no gain'} beyond the spread", flush=True)
