"""The cases of eg_dgemm_batched, shared by tests/test_gpu_dgemm_batched.py (the device against the oracle) and
tests/test_dgemm_batched_oracle_cpu.py (the oracle against a numpy.longdouble product: the bound is only worth relying on
where the reference itself stays well inside it).

The bound is the project's own for eg_dgemm (tests/test_gpu_f64.py): elementwise
    |got - want| <= 4e-16 * sqrt(K) * (|opA| @ |opB| + |accumulate start| + |bias|) + 1e-300.
"""
import numpy as np

POISON = -777.25
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]     # (ta, tb): NN NT TN TT
LAYOUT_IDS = ["NN", "NT", "TN", "TT"]

# batch, M, N, K: the smallest shapes that reach each part of the kernel
SHAPES = [(3, 1, 1, 1), (9, 16, 16, 4),    # one MFMA, one lane
          (2, 64, 64, 16),                 # a whole tile, one k-tile
          (3, 65, 63, 33),                 # one past the tile in M, one short in N, K ends inside a k-tile and an MFMA's four
          (5, 33, 20, 17),                 # ragged in every extent
          (7, 130, 70, 40)]                # six tiles per item, 42 blocks: the (item, tile) decode without remap
REMAP = (8, 128, 64, 24)                   # 16 blocks, a multiple of 8: the XCD remap is active (NN and TN)
EVEN = (5, 66, 36, 18)                     # every extent even: the padding alone decides the parity of ld and stride
# name -> keyword arguments of Case on the EVEN shape
ALIGNMENT = {
    "odd_ld": dict(pad_ld=1),                              # every leading dimension odd: the 8-byte load form
    "even_ld_odd_stride": dict(pad_ld=2, pad_stride=1),    # items 1, 3 misaligned: the call must take the 8-byte form
    "offset_1": dict(offset=1),                            # base not 16-byte aligned
    "even_ld_even_stride": dict(pad_ld=2, pad_stride=4),   # the 16-byte form with padding
}
SHARED = (4, 65, 63, 33)
EPILOGUE = (5, 33, 20, 17)
EPILOGUES = {"accumulate": dict(accumulate=True), "bias": dict(bias=True), "accumulate_bias": dict(accumulate=True, bias=True)}


def bound(K, mags):
    return 4e-16 * np.sqrt(K) * mags + 1e-300


class Case:
    """Host buffers of one batched call (float64) and what the call has to leave in C."""

    def __init__(self, batch, M, N, K, ta=False, tb=False, pad_ld=0, pad_stride=0, offset=0, share_a=False, share_b=False,
                 accumulate=False, bias=False, seed=0):
        rng = np.random.default_rng(seed)
        self.dims = (batch, M, N, K)
        self.ta, self.tb, self.accumulate, self.offset = ta, tb, accumulate, offset
        ra, ca = (K, M) if ta else (M, K)
        rb, cb = (N, K) if tb else (K, N)
        self.lda, self.ldb, self.ldc = ca + pad_ld, cb + pad_ld, N + pad_ld
        self.stride_a = 0 if share_a else ra * self.lda + pad_stride
        self.stride_b = 0 if share_b else rb * self.ldb + pad_stride
        self.stride_c = M * self.ldc + pad_stride
        u = lambda n: rng.random(n) - 0.5
        self.a = u(offset + (batch - 1) * self.stride_a + ra * self.lda)
        self.b = u(offset + (batch - 1) * self.stride_b + rb * self.ldb)
        c_len = offset + batch * self.stride_c
        self.c0 = u(c_len) if accumulate else np.full(c_len, POISON)
        self.bias = u(N) if bias else None
        item = lambda buf, i, stride, rows, ld, cols: buf[offset + i * stride:][:rows * ld].reshape(rows, ld)[:, :cols]
        self.a_items = [np.ascontiguousarray(item(self.a, i, self.stride_a, ra, self.lda, ca)) for i in range(batch)]
        self.b_items = [np.ascontiguousarray(item(self.b, i, self.stride_b, rb, self.ldb, cb)) for i in range(batch)]
        self.c_item = lambda buf, i: item(buf, i, self.stride_c, M, self.ldc, N)

    def label(self):
        return "eg_dgemm_batched %dx%dx%dx%d %s%s" % (self.dims + ("T" if self.ta else "N", "T" if self.tb else "N"))

    def start(self, i):
        _, M, N, _ = self.dims
        return np.ascontiguousarray(self.c_item(self.c0, i)) if self.accumulate else np.zeros((M, N))

    def ops(self, i):
        return (self.a_items[i].T if self.ta else self.a_items[i]), (self.b_items[i].T if self.tb else self.b_items[i])

    def oracle_item(self, refcpu, i):
        """refcpu.dgemm64 on item i's operands, from the accumulate start, plus the bias."""
        want = refcpu.dgemm64(self.a_items[i], self.b_items[i], self.ta, self.tb, out=self.start(i).copy())
        return want + self.bias[None, :] if self.bias is not None else want

    def magnitudes(self, i):
        opa, opb = self.ops(i)
        mags = np.abs(opa) @ np.abs(opb)
        if self.accumulate:
            mags = mags + np.abs(self.start(i))
        if self.bias is not None:
            mags = mags + np.abs(self.bias)[None, :]
        return mags

    def longdouble_item(self, i):
        opa, opb = self.ops(i)
        exact = opa.astype(np.longdouble) @ opb.astype(np.longdouble) + self.start(i).astype(np.longdouble)
        return exact + self.bias.astype(np.longdouble)[None, :] if self.bias is not None else exact


def seed_of(dims, ta, tb, extra=0):
    return 1000 * extra + sum(dims) + 2 * int(ta) + int(tb)


def table():
    """Every (id, Case keyword arguments) of the table in tests/test_gpu_dgemm_batched.py."""
    rows = []
    for dims in SHAPES:
        for (ta, tb), lid in zip(LAYOUTS, LAYOUT_IDS):
            rows.append(("%dx%dx%dx%d-%s" % (dims + (lid,)), dict(zip(("batch", "M", "N", "K"), dims), ta=ta, tb=tb, seed=seed_of(dims, ta, tb))))
    for (ta, tb), lid in ((LAYOUTS[0], "NN"), (LAYOUTS[2], "TN")):
        rows.append(("remap-%s" % lid, dict(zip(("batch", "M", "N", "K"), REMAP), ta=ta, tb=tb, seed=seed_of(REMAP, ta, tb))))
    for n, (name, kw) in enumerate(ALIGNMENT.items()):
        for (ta, tb), lid in zip(LAYOUTS, LAYOUT_IDS):
            rows.append(("%s-%s" % (name, lid), dict(zip(("batch", "M", "N", "K"), EVEN), ta=ta, tb=tb, seed=seed_of(EVEN, ta, tb, n + 1), **kw)))
    for n, share in enumerate(("share_a", "share_b")):
        for (ta, tb), lid in zip(LAYOUTS, LAYOUT_IDS):
            rows.append(("%s-%s" % (share, lid), dict(zip(("batch", "M", "N", "K"), SHARED), ta=ta, tb=tb, seed=seed_of(SHARED, ta, tb, n + 6), **{share: True})))
    for n, (name, kw) in enumerate(EPILOGUES.items()):
        for (ta, tb), lid in zip(LAYOUTS, LAYOUT_IDS):
            rows.append(("%s-%s" % (name, lid), dict(zip(("batch", "M", "N", "K"), EPILOGUE), ta=ta, tb=tb, seed=seed_of(EPILOGUE, ta, tb, n + 9), **kw)))
    return rows
