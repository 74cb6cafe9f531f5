"""The cases of eg_sgemm_batched2, shared by tests/test_gpu_sgemm_batched2.py (the device against the oracle and a float64
product) and tests/test_batched2_oracle_cpu.py (the oracle against the float64 product: the device's bound is only worth
relying on where the oracle itself is well inside it).

An operand is addressed by (ld, stride0, stride1) in floats: item (o, i) starts at offset + o * stride0 + i * stride1 and
is rows x cols with leading dimension ld.  `nested` lays items out one behind the other (padded on request), `in_row`
keeps the inner index inside the row as [outer, rows, inner, cols] does (q[b,i,h,k], o[b,i,h,d])."""
import numpy as np

POISON = np.float32(-777.25)


def nested(b1, rows, cols, pad_ld=0, pad_stride=0):
    ld = cols + pad_ld
    s1 = rows * ld + pad_stride
    return ld, b1 * s1 + pad_stride, s1


def in_row(b1, rows, cols, pad_cols=0, pad_stride=0):
    ld = b1 * (cols + pad_cols)
    return ld, rows * ld + pad_stride, cols + pad_cols


def span(b0, b1, rows, cols, lay):
    ld, s0, s1 = lay
    return (b0 - 1) * s0 + (b1 - 1) * s1 + (rows - 1) * ld + cols


def view(buf, offset, o, i, rows, cols, lay):
    ld, s0, s1 = lay
    start = offset + o * s0 + i * s1
    assert start + (rows - 1) * ld + cols <= buf.size
    return np.lib.stride_tricks.as_strided(buf[start:], shape=(rows, cols), strides=(4 * ld, 4))


class Case:
    """Host buffers of one call and what the call has to leave in C."""

    def __init__(self, b0, b1, M, N, K, ta=False, tb=False, a=None, b=None, c=None, offset=0, share_a=(), share_b=(), accumulate=False,
                 bias=False, tail=3, seed=0):
        rng = np.random.default_rng(seed)
        self.dims = (b0, b1, M, N, K)
        self.ta, self.tb, self.accumulate, self.offset = ta, tb, accumulate, offset
        self.ra, self.ca = (K, M) if ta else (M, K)
        self.rb, self.cb = (N, K) if tb else (K, N)
        share = lambda lay, which: (lay[0],) + tuple(0 if q in which else s for q, s in enumerate(lay[1:]))
        self.a_lay = share(a or nested(b1, self.ra, self.ca), share_a)     # share_x: the batch indices (0 outer, 1 inner) the
        self.b_lay = share(b or nested(b1, self.rb, self.cb), share_b)     # operand does not depend on
        self.c_lay = c or nested(b1, M, N)
        u = lambda n: (rng.random(n, dtype=np.float32) - np.float32(0.5)).astype(np.float32)
        self.a = u(offset + span(b0, b1, self.ra, self.ca, self.a_lay))
        self.b = u(offset + span(b0, b1, self.rb, self.cb, self.b_lay))
        c_len = offset + span(b0, b1, M, N, self.c_lay) + tail
        self.c0 = u(c_len) if accumulate else np.full(c_len, POISON, dtype=np.float32)
        self.bias = u(N) if bias else None

    def items(self):
        return [(o, i) for o in range(self.dims[0]) for i in range(self.dims[1])]

    def a_item(self, o, i):
        return np.ascontiguousarray(view(self.a, self.offset, o, i, self.ra, self.ca, self.a_lay))

    def b_item(self, o, i):
        return np.ascontiguousarray(view(self.b, self.offset, o, i, self.rb, self.cb, self.b_lay))

    def c_item(self, buf, o, i):
        return view(buf, self.offset, o, i, self.dims[2], self.dims[3], self.c_lay)

    def label(self):
        return "eg_sgemm_batched2 %dx%dx%dx%dx%d %s%s" % (self.dims + ("T" if self.ta else "N", "T" if self.tb else "N"))

    def start(self, o, i):
        M, N = self.dims[2:4]
        return np.ascontiguousarray(self.c_item(self.c0, o, i)) if self.accumulate else np.zeros((M, N), dtype=np.float32)

    def oracle(self, refcpu, o, i):
        ref = refcpu.sgemm(self.a_item(o, i), self.b_item(o, i), self.ta, self.tb, out=self.start(o, i).copy(), threads=1)
        if self.bias is not None:
            refcpu.bias_add(self.bias, ref)
        return ref

    def exact(self, o, i):
        opa = self.a_item(o, i).T if self.ta else self.a_item(o, i)
        opb = self.b_item(o, i).T if self.tb else self.b_item(o, i)
        e = opa.astype(np.float64) @ opb.astype(np.float64) + (self.start(o, i).astype(np.float64) if self.accumulate else 0.0)
        return e + self.bias.astype(np.float64) if self.bias is not None else e


LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]


def head_in_row(K, N, offset, seed):
    """q[b,i,h,k] * kk[b,j,h,k] -> o[b,i,h,n] at (batch, heads, M) = (2, 3, 33): NT, the head index inside every operand's row."""
    b0, b1, M = 2, 3, 33
    return Case(b0, b1, M, N, K, tb=True, a=in_row(b1, M, K), b=in_row(b1, N, K), c=in_row(b1, M, N), offset=offset, seed=seed)


def table():
    """(id, constructor) of every case that is compared with the oracle: K <= 96."""
    t = []
    for ta, tb in LAYOUTS:
        t.append(("nested-%d%d" % (ta, tb), lambda ta=ta, tb=tb: Case(2, 3, 33, 17, 5, ta, tb, seed=20 + 2 * ta + tb)))
    t.append(("head-in-row-16-byte", lambda: head_in_row(16, 20, 0, 31)))
    t.append(("head-in-row-elements", lambda: head_in_row(17, 19, 1, 32)))
    for offset in (0, 1):
        for ta, tb in LAYOUTS:
            def ragged(ta=ta, tb=tb, offset=offset):
                ra, ca = (48, 65) if ta else (65, 48)
                rb, cb = (130, 48) if tb else (48, 130)
                return Case(2, 3, 65, 130, 48, ta, tb, a=nested(3, ra, ca, 3, 5), b=nested(3, rb, cb, 3, 5), c=nested(3, 65, 130, 3, 5),
                            offset=offset, seed=40 + 2 * ta + tb + 4 * offset)
            t.append(("ragged-%d%d-offset%d" % (ta, tb, offset), ragged))
    for name, kw in (("b-inner", {"share_b": (1,)}), ("b-all", {"share_b": (0, 1)}), ("a-inner", {"share_a": (1,)}), ("a-all", {"share_a": (0, 1)})):
        t.append(("shared-" + name, lambda kw=kw: Case(2, 3, 40, 24, 12, seed=50, **kw)))
    t.append(("accumulate-bias", lambda: Case(2, 3, 70, 40, 33, accumulate=True, bias=True, seed=60)))
    return t
