"""Every group-2 library entry except the contractions, called on guarded, unaligned ranges inside larger allocations.

The cases are those of tests/range_cases.py, which says how the allocations are laid out, what the float64 references are
and where the bounds come from; tests/test_range_cases_cpu.py holds them to the oracle.  Every case allocates with
ctx.allocBuffer (16-byte aligned bases, asserted), uploads the WHOLE allocation of every operand (NaN around the inputs,
a sentinel around the result), passes the pointers behind the gaps, reads the WHOLE written allocation back and checks:
nothing outside the result changed by a bit, no NaN came in from behind an operand or from the result's own start values,
and the result meets the float64 reference within the project's bounds.

Which kernel or branch a case reaches
    elementwise.hip   eg_map, eg_map_grad, eg_axpy, eg_fill_f32: pattern "aligned" with n >= 4 takes the 16-byte chunked path
                      (4099: one chunk and a tail; 12289: three blocks and a tail), every other pattern and n < 4 the
                      grid-stride scalar path (70001: 274 blocks), forced by each operand alone in turn.  eg_bias_add:
                      chunked for cols % 4 == 0 with bias and out aligned; scalar for (64, 33) and for bias1 / out2.
                      chunk_range's second trip of a block needs the grid cap of 32 blocks per CU: the "large" test.
    reduce.hip        eg_sum: vector partials for n >= 4 and an aligned input.  eg_rowsum: range_cases.ROWSUM_SHAPES.
                      eg_colsum: range_cases.COLSUM_ROUTES lists first and second pass of every case (all six pairs of
                      vec / scalar with slab / tree / thread occur); the aligned patterns run
                      again in a child process that starts with EG_NO_SLAB_SUM=1, the slab sum off (tree and thread finals
                      behind a vector first pass).  eg_colsum_f64 has a single form.
    convolutions      the comments of range_cases.CONV_SHAPES, row by row, read from the dispatch code for 256 compute
                      units (the library reports no route, so the routes are a reading of the code, not an assertion).  Not reached by any row: conv2_direct.cpp's switch of its loads on the image's alignment
                      (it is in the float64 kernel of the model route; the float32 per-pixel kernel loads element by
                      element always).  The halo kernel is not reached by the two shapes the halo tests are named after
                      (too few or too empty patches on 256 compute units, asserted in the CPU test); 8 x 66 x 66 x 16 ->
                      64 (forward) and 8 x 64 x 64 x 64 -> 16 (image gradient) were added to reach it.
    fills             eg_fill_uniform / eg_fill_uniform_f64 / eg_fill_f64 have one grid-stride form each.

Nothing was trimmed for time: every convolution shape runs its five patterns in both modes.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import range_cases as rc
from conftest import TOL
from exprgrad_amd import _lib, ops

pytestmark = pytest.mark.gpu


def vp(p):
    return ctypes.c_void_p(int(p))


def launch(ctx, c, p):
    """The library call of case c on the device pointers p (operand -> address)."""
    a, f, acc = c.args, c.family, c.accumulate
    if f == "map":
        ops.map_(ctx, a["op"], a["n"], p["in"], p["out"], a["param"], accumulate=acc)
    elif f == "map_grad":
        ops.map_grad(ctx, a["op"], a["n"], p["in"], p["gout"], p["gin"], a["param"], accumulate=acc)
    elif f == "axpy":
        ops.axpy(ctx, a["n"], a["alpha"], p["x"], p["y"])
    elif f == "fill" and c.dtype == np.float32:
        ops.fill(ctx, a["n"], a["value"], p["out"])
    elif f == "fill":
        _lib.call("eg_fill_f64", ctx.handle, a["n"], float(a["value"]), vp(p["out"]))
    elif f == "bias_add":
        ops.bias_add(ctx, a["rows"], a["cols"], p["bias"], p["out"], accumulate=acc)
    elif f == "sum":
        ops.total(ctx, a["n"], p["in"], p["out"], accumulate=acc)
    elif f == "rowsum":
        ops.rowsum(ctx, a["rows"], a["cols"], p["in"], p["out"], accumulate=acc)
    elif f == "colsum":
        ops.colsum(ctx, a["rows"], a["cols"], p["in"], p["out"], accumulate=acc)
    elif f == "colsum_f64":
        _lib.call("eg_colsum_f64", ctx.handle, a["rows"], a["cols"], vp(p["in"]), vp(p["out"]), int(acc))
    elif f == "conv_fwd":
        ops.conv2_nhwc(ctx, *a["shape"], p["img"], p["flt"], p["out"], accumulate=acc)
    elif f == "conv_gf":
        ops.conv2_nhwc_grad_filter(ctx, *a["shape"], p["img"], p["gout"], p["gflt"], accumulate=acc)
    elif f == "conv_gi":
        ops.conv2_nhwc_grad_image(ctx, *a["shape"], p["flt"], p["gout"], p["gimg"], accumulate=acc)
    else:
        raise KeyError(f)


def upload(ctx, host):
    buf = ctx.allocBuffer(host.nbytes)
    assert buf.ptr % 16 == 0
    buf.write(host)
    return buf


def call(ctx, c, times=1):
    """The case's call on fresh device buffers; returns the whole written allocation as it is afterwards (one per call)."""
    item = c.dtype.itemsize
    hosts = c.buffers()
    bufs = {name: upload(ctx, h) for name, h in hosts.items()}
    ptrs = {name: b.ptr + item * c.first(name) for name, b in bufs.items()}
    for name, ptr in ptrs.items():
        assert (ptr % 16 == 0) == c.is_aligned(name)
    gots = []
    for t in range(times):
        if t:
            bufs[c.written].write(hosts[c.written])
        launch(ctx, c, ptrs)
        gots.append(bufs[c.written].read(c.dtype))
    for b in bufs.values():
        b.dealloc()
    return gots[0] if times == 1 else gots


def set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def by_name(cases):
    return {c.name: c for c in cases}


ELEMENTWISE = by_name(rc.map_cases() + rc.map_grad_cases() + rc.axpy_cases() + rc.fill_cases() + rc.bias_cases())
REDUCTIONS = by_name(rc.sum_cases() + rc.rowsum_cases() + rc.colsum_cases() + rc.colsum_f64_cases())


@pytest.mark.parametrize("name", list(ELEMENTWISE))
def test_elementwise_on_a_range(gpu_ctx, name):
    c = ELEMENTWISE[name]
    c.check(call(gpu_ctx, c))


@pytest.mark.parametrize("name", list(REDUCTIONS))
def test_reduction_on_a_range(gpu_ctx, name):
    c = REDUCTIONS[name]
    c.check(call(gpu_ctx, c))


@pytest.mark.parametrize("family,rows,cols,pattern", rc.TWICE)
def test_the_same_column_sum_twice_gives_the_same_bits(gpu_ctx, family, rows, cols, pattern):
    offs = rc.COLSUM_PATTERNS[pattern]
    for acc in (False, True):
        c = rc.RangeCase(family, offs, acc, pattern=pattern, rows=rows, cols=cols)
        first, second = call(gpu_ctx, c, times=2)
        c.check(first)
        assert np.array_equal(first.view(np.uint8), second.view(np.uint8)), c.name


def no_slab_pass():
    """Child process under EG_NO_SLAB_SUM=1: the aligned column sums again, tree and thread finals instead of the slab sum."""
    import exprgrad_amd as eg
    ctx = eg.newGpuContext()
    for c in rc.colsum_no_slab_cases():
        c.check(call(ctx, c))
    ctx.sync()
    print("no-slab pass ok")


def test_column_sum_routes_on_this_device(gpu_ctx):
    """The routes of range_cases.COLSUM_ROUTES are written down for 256 compute units and held to a restatement of
    reduce.hip's dispatch (range_cases.colsum_route), not to the dispatch itself: the library reports no route.  What can be
    held here: with this device's compute units the restated dispatch still sends the cases through all six pairs of first
    and second pass, and on 256 compute units through exactly the listed ones."""
    _, cus = large_length(gpu_ctx)
    seen = set()
    for (rows, cols), routes in rc.COLSUM_ROUTES.items():
        for pat, (i, o) in rc.COLSUM_PATTERNS.items():
            route = rc.colsum_route(rows, cols, rc.aligned(i), rc.aligned(o), cus=cus)
            assert cus != 256 or route == routes[pat]
            seen.add((route.split("+")[0], route.split("+")[1].split("(")[0]))
    assert seen == {(a, b) for a in ("vec", "scalar") for b in ("slab", "tree", "thread")}, (cus, seen)


def test_column_sums_without_the_slab_sum():
    """The pass again with EG_NO_SLAB_SUM=1, in a child process that starts with the switch set."""
    env = dict(os.environ, EG_NO_SLAB_SUM="1")
    done = subprocess.run([sys.executable, os.path.abspath(__file__), "no-slab-pass"], env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "no-slab pass ok" in done.stdout, done.stdout[-3000:] + done.stderr[-3000:]


# ---- convolutions ------------------------------------------------------------------------------------------------------------------
CONV = {s.id: s for s in rc.CONV_SHAPES}


@pytest.mark.parametrize("call_name", rc.CONV_CALLS)
@pytest.mark.parametrize("shape", list(CONV))
def test_convolution_on_ranges(gpu_ctx, monkeypatch, shape, call_name):
    """The five pointer patterns in both modes against the float64 reference; every unaligned result within 2 * TOL * max|want|
    of the aligned one (two orders of one sum, each within TOL of its value), bit-identical where only the form of the
    stores differs; filter gradients twice, bit for bit (fixed-order second passes, whatever gflt's alignment)."""
    s = CONV[shape]
    set_env(monkeypatch, s.env)
    cases = s.cases(call_name)
    results = {}
    for (pat, acc), c in cases.items():
        if call_name == "conv_gf":
            got, again = call(gpu_ctx, c, times=2)
            assert np.array_equal(got.view(np.uint8), again.view(np.uint8)), c.name
        else:
            got = call(gpu_ctx, c)
        c.check(got)
        results[pat, acc] = c.interior(got)
    for acc in (False, True):
        base, want = results["aligned", acc], cases["aligned", acc].want()
        limit = 2 * TOL * float(np.abs(want).max())
        for pat in rc.CONV_PATTERNS:
            if pat == "aligned":
                continue
            apart = float(np.abs(results[pat, acc].astype(np.float64) - base).max())
            print("%s: %.3g from the aligned result, limit %.3g" % (cases[pat, acc].name, apart, limit))
            assert apart <= limit, cases[pat, acc].name
        if call_name in s.same_bits:
            assert np.array_equal(results["out1", acc].view(np.uint32), base.view(np.uint32)), cases["out1", acc].name


# ---- fills -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in rc.fill_f64_cases()])
def test_fill_f64_on_a_range(gpu_ctx, name):
    c = by_name(rc.fill_f64_cases())[name]
    c.check(call(gpu_ctx, c))


def uniform(ctx, dtype, n, off, state, stream):
    """eg_fill_uniform / eg_fill_uniform_f64 into a guarded range; the guards checked, the n values returned."""
    c = rc.uniform_cases(dtype)[n, off]
    lo, hi = rc.UNIFORM_RANGE
    host = c.buffers()["out"]
    buf = upload(ctx, host)
    ptr = buf.ptr + c.dtype.itemsize * c.first("out")
    entry = "eg_fill_uniform" if c.dtype == np.float32 else "eg_fill_uniform_f64"
    _lib.call(entry, ctx.handle, n, lo, hi, vp(state.ptr), stream, vp(ptr))
    got = buf.read(c.dtype)
    buf.dealloc()
    c.check_outside(got)
    vals = c.interior(got)
    assert np.isfinite(vals).all() and (vals >= lo).all() and (vals < hi).all(), (entry, n, off, vals.min(), vals.max())
    return vals.copy()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_uniform_fills_on_ranges(gpu_ctx, dtype):
    """Guards exact, every value in [lo, hi), the same numbers at either alignment, and element i a function of i alone."""
    state = upload(gpu_ctx, np.array([12345, 7], dtype=np.uint64))
    draws = {(n, off): uniform(gpu_ctx, dtype, n, off, state, stream=3) for n in rc.UNIFORM_LENGTHS for off in rc.UNIFORM_OFFSETS}
    for n in rc.UNIFORM_LENGTHS:
        assert np.array_equal(draws[n, 0], draws[n, 1]), n
    assert np.array_equal(draws[70001, 1][:1000], draws[1000, 0])
    assert np.array_equal(draws[1000, 0][:5], draws[5, 1]) and draws[5, 0][0] == draws[1, 0][0]
    assert np.unique(draws[70001, 0]).size > 60000                        # numbers, not a constant
    assert not np.array_equal(uniform(gpu_ctx, dtype, 1000, 1, state, stream=4), draws[1000, 1])
    state.dealloc()


# ---- the loop small lengths cannot reach ---------------------------------------------------------------------------------------------
def large_length(ctx):
    cu, clock, hbm = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    arch = ctypes.create_string_buffer(64)
    _lib.call("eg_device_props", 0, ctypes.byref(cu), ctypes.byref(clock), ctypes.byref(hbm), arch, 64)
    return 4 * (2 * 32 * cu.value * 1024 + 1024) + 3, cu.value


@pytest.mark.parametrize("what", ["fill", "scale"])
def test_chunked_path_past_the_grid_cap(gpu_ctx, what):
    """chunk_range gives a block a second trip of 1024 sixteen-byte groups only when the grid is capped at 32 blocks per
    CU: n = 4 * (2 * 32 * cus * 1024 + 1024) + 3, two trips and a ragged third for every block, the last block's chunk
    ending early, and a 3-element tail (268 MB per operand on 256 CUs).  Guards exact; the values exact on the whole array
    (a fill, and one correctly rounded multiply by 2.5)."""
    n, cus = large_length(gpu_ctx)
    assert n // 4 > 32 * cus * 1024
    rng = np.random.default_rng(n)
    out0 = rc.embed(np.full(n, np.nan, dtype=np.float32), 0, np.float32(rc.SENTINEL))
    out = upload(gpu_ctx, out0)
    if what == "fill":
        ops.fill(gpu_ctx, n, 1.5, out.ptr + 4 * rc.GUARD)
        want = np.full(n, 1.5, dtype=np.float32)
    else:
        x = (rng.random(n, dtype=np.float32) - 0.5) * 8
        xin = upload(gpu_ctx, rc.embed(x, 0, np.float32(np.nan)))
        ops.map_(gpu_ctx, "scale", n, xin.ptr + 4 * rc.GUARD, out.ptr + 4 * rc.GUARD, 2.5)
        want = (x.astype(np.float64) * 2.5).astype(np.float32)
    got = out.read(np.float32)
    out.dealloc()
    if what == "scale":
        xin.dealloc()
    lo = rc.GUARD
    assert np.array_equal(got[:lo].view(np.uint32), out0[:lo].view(np.uint32)) and np.array_equal(got[lo + n:].view(np.uint32), out0[lo + n:].view(np.uint32))
    wrong = np.flatnonzero(got[lo:lo + n] != want)
    assert wrong.size == 0, (what, wrong.size, "first at", int(wrong[0]), got[lo + wrong[0]], want[wrong[0]])


if __name__ == "__main__" and sys.argv[1:] == ["no-slab-pass"]:
    no_slab_pass()
