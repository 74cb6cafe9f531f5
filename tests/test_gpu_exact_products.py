"""Every contraction route of the library on operands whose product is known exactly (tests/exact_cases.py has the
generators, the references and the derivation of every bound; tests/test_exact_cases_cpu.py holds them on the CPU).

The other contraction tests bound the error by the largest element of C, or compare with a sibling that shares the
arithmetic.  Here every element of C is held to its own value: with monomial operands it is one product, with grid
operands an exact sum, so an operand that lost low bits, a wrong element among small ones, or a split-bf16 product that
lost one of its 2^-16 terms fails.  C is always compared whole, inside the guard-and-NaN embedding of
tests/gemm_view_cases.py: a stray store is a changed sentinel, an element read from outside an operand is a NaN in C.

  a. eg_sgemm's exact routes: for every (route, second pass) of tests/golden/gemm_routes.json its smallest row, as the row
     states it (exact_cases.sgemm_table; EG_NO_SPLIT_GEMM=1, so the route is the planner's).
  b. the split-bf16 product at the smallest shape its gate admits, on both loops and both split passes.
  c. eg_sgemm_batched and eg_sgemm_batched2 on the shapes of their own tests' tables, one per kernel form.
  d. eg_dgemm on the smallest row per tile choice of tests/golden/dgemm_routes.json, eg_dgemm_batched on its table's shapes.
"""
import ctypes
import functools
import zlib

import numpy as np
import pytest

import batched2_cases as b2
import exact_cases as ec
from exprgrad_amd import _lib, ops

pytestmark = pytest.mark.gpu


def seed_of(*words):
    return zlib.crc32(" ".join(str(w) for w in words).encode())


class OnDevice:
    """A Call's operands on the device; run() uploads C's start, launches and reads the WHOLE C allocation back."""

    def __init__(self, ctx, call):
        self.ctx, self.call = ctx, call
        self.bufs = [self._up(h) for h in (call.a, call.b)] + [ctx.allocBuffer(call.c0.nbytes)] + ([self._up(call.bias)] if call.bias is not None else [])

    def _up(self, host):
        buf = self.ctx.allocBuffer(host.nbytes)
        assert buf.ptr % 16 == 0
        buf.write(host)
        return buf

    def run(self):
        c = self.call
        item = c.dtype.itemsize
        self.bufs[2].write(c.c0)
        pa, pb, pc = (self.bufs[n].ptr + item * s for n, s in enumerate(c.starts()[:3]))
        pbias = self.bufs[3].ptr + item * c.starts()[3] if c.bias is not None else None
        M, N, K = c.dims
        if c.dtype == np.float32:
            ops.sgemm(self.ctx, M, N, K, pa, c.lda, pb, c.ldb, pc, c.ldc, c.ta, c.tb, c.accumulate, pbias)
        else:
            _lib.call("eg_dgemm", self.ctx.handle, int(c.ta), int(c.tb), M, N, K, ctypes.c_void_p(pa), c.lda, ctypes.c_void_p(pb), c.ldb,
                      ctypes.c_void_p(pc), c.ldc, int(c.accumulate), ctypes.c_void_p(pbias) if pbias else None)
        got = self.bufs[2].read(c.dtype)
        c.check_outside(got)
        return c.interior(got)

    def free(self):
        for b in self.bufs:
            b.dealloc()


def run_once(ctx, call):
    dev = OnDevice(ctx, call)
    try:
        return dev.run()
    finally:
        dev.free()


def operands(kind, M, N, K, rng, dtype=np.float32):
    """-> op(A), op(B) and the two factors of every element of C (None for `grid`).  `epilogue` is `rows` again."""
    if kind == "grid":
        return ec.grid((M, K), rng, dtype), ec.grid((K, N), rng, dtype), None
    if kind == "cols":
        opa = ec.values((M, K), rng, dtype)
        opb, k, b = ec.monomial_cols(K, N, rng, dtype)
        return opa, opb, ec.cols_factors(opa, k, b)
    opa, k, a = ec.monomial_rows(M, K, rng, dtype)
    opb = ec.values((K, N), rng, dtype)
    return opa, opb, ec.rows_factors(k, a, opb)


def exact_route_case(ctx, make_call, kind, M, N, K, dtype, needs_bias, order_stated, what):
    """One run of the four an exact route gets.  rows / cols / grid: the bits of the exact result in a NaN-filled C.
    epilogue: start values and a bias of +-[1, 2) on monomial rows under the 3u bound, and where the route's header states
    the order C = (old + sum) + bias (order_stated), the bits of that order."""
    rng = np.random.default_rng(seed_of(what, kind))
    opa, opb, factors = operands(kind, M, N, K, rng, dtype)
    if kind != "epilogue":
        # a row whose plan needs a bias gets one of zeros: +0 onto a nonzero product, or onto an exact sum, changes no bit
        # (a grid sum of exactly -0 does not occur: an in-order sum from +0 never gives -0)
        got = run_once(ctx, make_call(opa, opb, bias=np.zeros(N, dtype=dtype) if needs_bias else None))
        ec.same_bits(got, ec.grid_reference(opa, opb) if factors is None else ec.rounded_product(*factors), what + " " + kind)
        return
    old, bias = ec.values((M, N), rng, dtype), ec.values(N, rng, dtype)
    got = run_once(ctx, make_call(opa, opb, start=old, bias=bias))
    ab = ec.exact_product(*factors)
    worst = ec.within(got, old.astype(ab.dtype) + ab + bias.astype(ab.dtype), ec.epilogue_bound(old, ab, bias[None, :], dtype), what + " epilogue")
    print("%s: (old + ab) + bias off by at most %.3f of 3u (|old| + |ab| + |bias|)" % (what, worst))
    if order_stated:
        ec.same_bits(got, ec.epilogue_in_order(old, ec.rounded_product(*factors), bias[None, :]), what + " epilogue, in the stated order")


# ---- a. eg_sgemm, the exact routes -----------------------------------------------------------------------------------------
SGEMM_TABLE = ec.sgemm_table()
KINDS = ["rows", "cols", "grid", "epilogue"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", SGEMM_TABLE, ids=[ec.route_id(r) for r in SGEMM_TABLE])
def test_sgemm_exact_route(gpu_ctx, monkeypatch, row, kind):
    """The fixture row's call — its layout, leading dimensions, base alignments and switches — so the route and the second
    pass are the ones its id names (tests/test_gemm_plan_cpu.py).  The epilogue run adds a bias where the row has none,
    which may move a `tree` row to split_reduce: that run is about the epilogue's arithmetic, the other three about the
    route's.  The second passes' headers (gemm_f32_mfma.hpp: split-K, tail tiles) state C = (old + slabs) + bias."""
    monkeypatch.setenv("EG_NO_SPLIT_GEMM", "1")
    for k, v in ec.switch_env(row["switches"]).items():
        monkeypatch.setenv(k, v)
    exact_route_case(gpu_ctx, functools.partial(ec.sgemm_call, row), kind, row["M"], row["N"], row["K"], np.float32, row["bias"] != 0,
                     row["expect"].get("second") in ("split_reduce", "tail_reduce"), ec.route_id(row))


# ---- b. the split-bf16 product ---------------------------------------------------------------------------------------------
SPLIT_M = SPLIT_N = 4096           # 256 tiles of 256 x 256 on 256 CUs, K >= 2048: the smallest shape inside the gate
# id -> monomial operand, layout, K, (pad_a, pad_b, pad_c)
SPLIT_CASES = {
    "rows-NN": ("rows", False, False, 2048, (0, 0, 0)),
    "rows-TN": ("rows", True, False, 2048, (0, 0, 0)),             # op(A)'s k runs along lda: split_tiles_kernel
    "cols-NN": ("cols", False, False, 2048, (0, 0, 0)),
    "cols-NT": ("cols", False, True, 2048, (0, 0, 0)),             # op(B) k-contiguous
    "rows-TT": ("rows", True, True, 2048, (0, 0, 0)),
    "rows-NN-padded": ("rows", False, False, 2048, (4, 4, 8)),     # NaN behind every row of A and B, sentinels behind C's
    "rows-NN-K2112": ("rows", False, False, 2112, (0, 0, 0)),      # 132 k-tiles: the ring of three stages ends on another stage than with 128
}
SPLIT_MODES = {"default": {}, "no-skew": {"EG_GEMM_NO_SKEW": "1"}, "scalar-pass": {"EG_SPLIT_PASS_SCALAR": "1"}}


@functools.lru_cache(maxsize=1)
def split_case(name):
    """Operands, factors and references of one split case, shared by its three modes (the tests run case by case)."""
    kind, ta, tb, K, pad = SPLIT_CASES[name]
    opa, opb, factors = operands(kind, SPLIT_M, SPLIT_N, K, np.random.default_rng(seed_of("split", name)))
    lda, ldb = (SPLIT_M if ta else K) + pad[0], (K if tb else SPLIT_N) + pad[1]
    call = ec.Call(opa, opb, ta, tb, lda, ldb, SPLIT_N + pad[2])
    ab = ec.exact_product(*factors)
    return call, ab, ab.astype(np.float32)


def set_split_mode(monkeypatch, mode):
    monkeypatch.delenv("EG_NO_SPLIT_GEMM", raising=False)
    for k in ("EG_GEMM_NO_SKEW", "EG_SPLIT_PASS_SCALAR"):
        if k in SPLIT_MODES[mode]:
            monkeypatch.setenv(k, "1")
        else:
            monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("name,mode", [(n, m) for n in SPLIT_CASES for m in SPLIT_MODES])
def test_split_product_holds_every_element(gpu_ctx, monkeypatch, name, mode):
    """Every one of the 16 M elements within 8 units of 2^-24 |ab| of its own product (exact_cases has the derivation), on
    the ping-pong loop, on the in-phase loop (EG_GEMM_NO_SKEW=1) and behind the scalar split pass (EG_SPLIT_PASS_SCALAR=1).
    Some element must differ from fl(ab): the exact kernel, which stands in when an operand does not split or the gate
    refuses, would be bit-exact, so a difference shows that the split route ran.  The emulation expects 4 to 24 % to
    differ."""
    call, ab, fl_ab = split_case(name)
    set_split_mode(monkeypatch, mode)
    got = run_once(gpu_ctx, call)
    what = "split %s %s" % (name, mode)
    worst = ec.SPLIT_UNITS * ec.within(got, ab, ec.split_bound(ab), what)
    differ = float((got != fl_ab).mean())
    print("%s: at most %.3f units of 2^-24 |ab|; %.2f %% of the elements differ from fl(ab)" % (what, worst, 100 * differ))
    assert differ > 0, what + ": every element is fl(ab): the exact kernel ran, not the split product"


@pytest.mark.parametrize("ta", [False, True], ids=["NN", "TN"])
def test_split_product_of_grid_operands_is_exact(gpu_ctx, monkeypatch, ta):
    """Grid values are exact in bf16: plane 0 holds them, planes 1 and 2 are zero, every sum is exact, so the result has the
    bits of numpy's float32 product.  The split and the exact route cannot be told apart on such data; the same call shapes
    ran the split route in test_split_product_holds_every_element (rows-NN, rows-TN), and grid values always split exactly
    (tests/test_exact_cases_cpu.py), so the fallback to the exact kernel was not involved here."""
    set_split_mode(monkeypatch, "default")
    rng = np.random.default_rng(seed_of("split grid", ta))
    opa, opb, _ = operands("grid", SPLIT_M, SPLIT_N, 2048, rng)
    got = run_once(gpu_ctx, ec.Call(opa, opb, ta, False))
    ec.same_bits(got, ec.grid_reference(opa, opb), "split grid %s" % ("TN" if ta else "NN"))


def test_split_product_onto_start_values_with_a_bias(gpu_ctx, monkeypatch):
    """Monomial rows, NN, accumulate and a bias: the split bound plus the epilogue's 3u (|old| + |ab| + |bias|)."""
    set_split_mode(monkeypatch, "default")
    rng = np.random.default_rng(seed_of("split epilogue"))
    opa, opb, factors = operands("rows", SPLIT_M, SPLIT_N, 2048, rng)
    old, bias = ec.values((SPLIT_M, SPLIT_N), rng), ec.values(SPLIT_N, rng)
    got = run_once(gpu_ctx, ec.Call(opa, opb, start=old, bias=bias))
    ab = ec.exact_product(*factors)
    worst = ec.within(got, old + ab + bias, ec.split_bound(ab) + ec.epilogue_bound(old, ab, bias[None, :], np.float32), "split epilogue")
    print("split product onto start values with a bias: %.3f of the summed bounds" % worst)


# ---- c. eg_sgemm_batched, eg_sgemm_batched2 --------------------------------------------------------------------------------
def one_index(batch, M, N, K, ta=False, tb=False, pad_ld=0, pad_stride=0, offset=0, share_a=False, share_b=False, dtype=np.float32):
    """The addressing of tests/test_gpu_sgemm_batched.py's and tests/dgemm_batched_cases.py's Case, as a Batch with batch0 = 1."""
    ra, ca = (K, M) if ta else (M, K)
    rb, cb = (N, K) if tb else (K, N)
    lda, ldb, ldc = ca + pad_ld, cb + pad_ld, N + pad_ld
    lay = lambda rows, ld, shared: (ld, 0, 0 if shared else rows * ld + pad_stride)
    return ec.Batch(1, batch, M, N, K, ta, tb, lay(ra, lda, share_a), lay(rb, ldb, share_b), lay(M, ldc, False), offset, dtype)


# one shape per kernel form of gemm_batched.hip (whole tiles | ragged with 16-byte loads | ragged with element loads; direct
# stores | whole tiles through LDS from K = 128), from the tables of tests/test_gpu_sgemm_batched.py
BATCHED = {
    "tiny-NN": lambda: one_index(3, 33, 17, 5),
    "whole-tiles-NT": lambda: one_index(5, 64, 64, 64, tb=True),
    "ragged-elements-TT-offset1": lambda: one_index(7, 65, 130, 48, True, True, pad_ld=3, pad_stride=5, offset=1),
    "ragged-padded-TN": lambda: one_index(7, 65, 130, 48, True, False, pad_ld=3, pad_stride=5),
    "lds-stores-whole-NN": lambda: one_index(3, 128, 64, 128, pad_stride=4),
    "lds-stores-ragged-NN": lambda: one_index(5, 130, 72, 160, pad_stride=4),      # a ragged last tile in M and N
    "shared-a-NN": lambda: one_index(4, 96, 96, 40, share_a=True),
    "shared-b-TN": lambda: one_index(4, 96, 96, 40, ta=True, share_b=True),
}


def two_index(b0, b1, M, N, K, ta=False, tb=False, a=None, b=None, c=None, offset=0, share_a=(), share_b=()):
    """The addressing of batched2_cases.Case."""
    ra, ca = (K, M) if ta else (M, K)
    rb, cb = (N, K) if tb else (K, N)
    share = lambda lay, which: (lay[0],) + tuple(0 if q in which else s for q, s in enumerate(lay[1:]))
    return ec.Batch(b0, b1, M, N, K, ta, tb, share(a or b2.nested(b1, ra, ca), share_a), share(b or b2.nested(b1, rb, cb), share_b),
                    c or b2.nested(b1, M, N), offset)


def head_in_row(K, N, offset):
    return two_index(2, 3, 33, N, K, tb=True, a=b2.in_row(3, 33, K), b=b2.in_row(3, N, K), c=b2.in_row(3, 33, N), offset=offset)


# the shapes of tests/batched2_cases.py's table and of test_stores_through_lds_leave_the_gaps
BATCHED2 = {
    "nested-TN": lambda: two_index(2, 3, 33, 17, 5, ta=True),
    "head-in-row-16-byte": lambda: head_in_row(16, 20, 0),
    "head-in-row-elements": lambda: head_in_row(17, 19, 1),
    "ragged-TT-offset1": lambda: two_index(2, 3, 65, 130, 48, True, True, a=b2.nested(3, 48, 65, 3, 5), b=b2.nested(3, 130, 48, 3, 5),
                                           c=b2.nested(3, 65, 130, 3, 5), offset=1),
    "ragged-NN": lambda: two_index(2, 3, 65, 130, 48, a=b2.nested(3, 65, 48, 3, 5), b=b2.nested(3, 48, 130, 3, 5), c=b2.nested(3, 65, 130, 3, 5)),
    "shared-b-inner": lambda: two_index(2, 3, 40, 24, 12, share_b=(1,)),
    "shared-a-all": lambda: two_index(2, 3, 40, 24, 12, share_a=(0, 1)),
    "lds-stores-in-row": lambda: two_index(2, 2, 128, 64, 128, c=b2.in_row(2, 128, 64, pad_cols=4, pad_stride=8)),
}


def run_batch(ctx, batch, entry):
    hosts = (batch.a, batch.b, batch.c0)
    bufs = [ctx.allocBuffer(h.nbytes) for h in hosts]
    try:
        for buf, h in zip(bufs, hosts):
            buf.write(h)
        pa, pb, pc = (buf.ptr + batch.offset * batch.dtype.itemsize for buf in bufs)
        b0, b1, M, N, K = batch.dims
        al, bl, cl = batch.a_lay, batch.b_lay, batch.c_lay
        if entry == "batched2":
            ops.sgemm_batched2(ctx, b0, b1, M, N, K, pa, al[0], al[1:], pb, bl[0], bl[1:], pc, cl[0], cl[1:], batch.ta, batch.tb)
        else:
            assert b0 == 1
            fn = ops.sgemm_batched if batch.dtype == np.float32 else ops.dgemm_batched
            fn(ctx, b1, M, N, K, pa, al[0], al[2], pb, bl[0], bl[2], pc, cl[0], cl[2], batch.ta, batch.tb)
        return bufs[2].read(batch.dtype)
    finally:
        for buf in bufs:
            buf.dealloc()


@pytest.mark.parametrize("kind", ["rows", "cols", "grid"])
@pytest.mark.parametrize("name", list(BATCHED))
def test_sgemm_batched_items_are_exact(gpu_ctx, name, kind):
    """Every item has the bits of its exact result, and nothing outside the items changed."""
    batch = ec.fill_batch(BATCHED[name](), kind, seed_of("batched", name, kind))
    batch.check(run_batch(gpu_ctx, batch, "batched"), "eg_sgemm_batched %s %s" % (name, kind))


@pytest.mark.parametrize("kind", ["rows", "cols", "grid"])
@pytest.mark.parametrize("name", list(BATCHED2))
def test_sgemm_batched2_items_are_exact(gpu_ctx, name, kind):
    batch = ec.fill_batch(BATCHED2[name](), kind, seed_of("batched2", name, kind))
    batch.check(run_batch(gpu_ctx, batch, "batched2"), "eg_sgemm_batched2 %s %s" % (name, kind))


# ---- d. eg_dgemm, eg_dgemm_batched -----------------------------------------------------------------------------------------
DGEMM_TABLE = ec.dgemm_table()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", DGEMM_TABLE, ids=[ec.dgemm_id(r) for r in DGEMM_TABLE])
def test_dgemm_exact(gpu_ctx, monkeypatch, row, kind):
    """The smallest fixture row per tile (128 x 128, 128 x 64, 64 x 64), sliced and not, with and without the XCD remap and
    the 16-byte loads; a row that forces its tile does so through EG_DGEMM_TILE.  Monomial: the bits of the correctly rounded
    float64 product.  The epilogue run holds the 3u bound alone: the float64 headers (gemm_f64_tile.hpp) name the three
    addends of out = old + slabs + bias without fixing the order of the two additions (the kernels add the bias to the
    product first), so there are no bits to assert."""
    if row["tile"] != "-":
        monkeypatch.setenv("EG_DGEMM_TILE", row["tile"])
    exact_route_case(gpu_ctx, functools.partial(ec.dgemm_call, row), kind, row["M"], row["N"], row["K"], np.float64, False, False, ec.dgemm_id(row))


# the shapes of tests/dgemm_batched_cases.py: ragged, the XCD remap, both load forms, a base one double off, shared operands,
# six tiles per item
DGEMM_BATCHED = {
    "ragged-NT": lambda: one_index(3, 65, 63, 33, tb=True, dtype=np.float64),
    "remap-TN": lambda: one_index(8, 128, 64, 24, ta=True, dtype=np.float64),
    "odd-ld-NN": lambda: one_index(5, 66, 36, 18, pad_ld=1, dtype=np.float64),
    "even-ld-odd-stride-NT": lambda: one_index(5, 66, 36, 18, tb=True, pad_ld=2, pad_stride=1, dtype=np.float64),
    "even-ld-even-stride-TT": lambda: one_index(5, 66, 36, 18, True, True, pad_ld=2, pad_stride=4, dtype=np.float64),
    "offset-1-NN": lambda: one_index(5, 66, 36, 18, offset=1, dtype=np.float64),
    "shared-a-NN": lambda: one_index(4, 65, 63, 33, share_a=True, dtype=np.float64),
    "shared-b-TN": lambda: one_index(4, 65, 63, 33, ta=True, share_b=True, dtype=np.float64),
    "six-tiles-NN": lambda: one_index(7, 130, 70, 40, dtype=np.float64),
}


@pytest.mark.parametrize("kind", ["rows", "cols", "grid"])
@pytest.mark.parametrize("name", list(DGEMM_BATCHED))
def test_dgemm_batched_items_are_exact(gpu_ctx, name, kind):
    batch = ec.fill_batch(DGEMM_BATCHED[name](), kind, seed_of("dgemm batched", name, kind))
    batch.check(run_batch(gpu_ctx, batch, "batched"), "eg_dgemm_batched %s %s" % (name, kind))
