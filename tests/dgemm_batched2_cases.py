"""The cases of eg_dgemm_batched2, shared by tests/test_gpu_dgemm_batched2.py (the device against the oracle) and
tests/test_dgemm_batched2_oracle_cpu.py (the oracle against a numpy.longdouble product: the bound is only worth relying on
where the reference itself stays well inside it).  The float64 form of tests/batched2_cases.py.

An operand is addressed by (ld, stride0, stride1) in doubles: item (o, i) starts at offset + o * stride0 + i * stride1 and
is rows x cols with leading dimension ld.  `nested` lays items out one behind the other (padded on request), `in_row`
keeps the inner index inside the row as [outer, rows, inner, cols] does (q[b,i,h,k], o[b,i,h,d]).  A C that is not
accumulated into is POISON everywhere, as in tests/dgemm_batched_cases.py: a store outside the items shows.

The bound is the project's own for eg_dgemm (tests/test_gpu_f64.py, tests/test_gpu_dgemm_batched.py): elementwise
    |got - want| <= 4e-16 * sqrt(K) * (|opA| @ |opB| + |accumulate start| + |bias|) + 1e-300.
"""
import numpy as np

POISON = -777.25
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]     # (ta, tb): NN NT TN TT
LAYOUT_IDS = ["NN", "NT", "TN", "TT"]


def bound(K, mags):
    return 4e-16 * np.sqrt(K) * mags + 1e-300


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
    return np.lib.stride_tricks.as_strided(buf[start:], shape=(rows, cols), strides=(8 * ld, 8))


class Case:
    """Host buffers of one call (float64) and what the call has to leave in C."""

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
        u = lambda n: rng.random(n) - 0.5
        self.a = u(offset + span(b0, b1, self.ra, self.ca, self.a_lay))
        self.b = u(offset + span(b0, b1, self.rb, self.cb, self.b_lay))
        c_len = offset + span(b0, b1, M, N, self.c_lay) + tail
        self.c0 = np.full(c_len, POISON)
        if accumulate:      # values in the items, poison between and behind them
            fill = u(c_len)
            for o, i in self.items():
                self.c_item(self.c0, o, i)[...] = self.c_item(fill, o, i)
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
        return "eg_dgemm_batched2 %dx%dx%dx%dx%d %s%s" % (self.dims + ("T" if self.ta else "N", "T" if self.tb else "N"))

    def start(self, o, i):
        M, N = self.dims[2:4]
        return np.ascontiguousarray(self.c_item(self.c0, o, i)) if self.accumulate else np.zeros((M, N))

    def ops(self, o, i):
        a, b = self.a_item(o, i), self.b_item(o, i)
        return (a.T if self.ta else a), (b.T if self.tb else b)

    def oracle_item(self, refcpu, o, i):
        """refcpu.dgemm64 on item (o, i)'s operands, from the accumulate start, plus the bias."""
        want = refcpu.dgemm64(self.a_item(o, i), self.b_item(o, i), self.ta, self.tb, out=self.start(o, i).copy())
        return want + self.bias[None, :] if self.bias is not None else want

    def magnitudes(self, o, i):
        opa, opb = self.ops(o, i)
        mags = np.abs(opa) @ np.abs(opb)
        if self.accumulate:
            mags = mags + np.abs(self.start(o, i))
        if self.bias is not None:
            mags = mags + np.abs(self.bias)[None, :]
        return mags

    def longdouble_item(self, o, i):
        opa, opb = self.ops(o, i)
        exact = opa.astype(np.longdouble) @ opb.astype(np.longdouble) + self.start(o, i).astype(np.longdouble)
        return exact + self.bias.astype(np.longdouble)[None, :] if self.bias is not None else exact


def scores_in_row(K, N, offset, seed):
    """s[b,h,i,j] ++= q[b,i,h,k] * kk[b,j,h,k] at (batch, heads, I) = (2, 3, 33): NT, ld = H * K and inner stride K for both
    operands; the scores nested."""
    b0, b1, M = 2, 3, 33
    return Case(b0, b1, M, N, K, tb=True, a=in_row(b1, M, K), b=in_row(b1, N, K), offset=offset, seed=seed)


def context_in_row(J, D, offset, seed):
    """o[b,i,h,d] ++= p[b,h,i,j] * v[b,j,h,d]: NN, p nested, v and the output with the head index inside the row — the
    items of C interleave (ldc = H * D, stride_c1 = D)."""
    b0, b1, M = 2, 3, 33
    return Case(b0, b1, M, D, J, b=in_row(b1, J, D), c=in_row(b1, M, D), offset=offset, seed=seed)


# (2, 3) items of 34 x 36 x 18: every extent even, so the padding alone decides the parity of ld and of the strides
EVEN = (2, 3, 34, 36, 18)


def even_case(ta, tb, odd=None, offset=0, seed=0):
    """Even leading dimensions everywhere; `odd` names the one batch stride that is odd ("a0", "a1", "b0", "b1"), None: all
    four even, the 16-byte path when offset == 0.  offset = 1 puts every pointer one double off 16-byte alignment."""
    b0, b1, M, N, K = EVEN
    ra, ca = (K, M) if ta else (M, K)
    rb, cb = (N, K) if tb else (K, N)

    def lay(rows, cols, which):
        ld = cols + 2
        s1 = rows * ld + 4
        s0 = b1 * s1 + 6
        if odd == which + "1":
            s1 += 1            # the inner stride alone: three odd strides and 7 keep the outer one even
            s0 = b1 * s1 + 7
        if odd == which + "0":
            s0 += 1
        return ld, s0, s1
    return Case(b0, b1, M, N, K, ta, tb, a=lay(ra, ca, "a"), b=lay(rb, cb, "b"), c=nested(b1, M, N, 2, 4), offset=offset, seed=seed)


def table():
    """(id, constructor) of every case that is compared with the oracle."""
    t = []
    for n, ((ta, tb), lid) in enumerate(zip(LAYOUTS, LAYOUT_IDS)):
        t.append(("one-ragged-tile-" + lid, lambda ta=ta, tb=tb, n=n: Case(2, 3, 33, 20, 19, ta, tb, seed=20 + n)))

        def four(ta=ta, tb=tb, n=n):      # 2 x 2 ragged tiles, padded rows and items
            ra, ca = (35, 70) if ta else (70, 35)
            rb, cb = (65, 35) if tb else (35, 65)
            return Case(2, 3, 70, 65, 35, ta, tb, a=nested(3, ra, ca, 3, 5), b=nested(3, rb, cb, 3, 5), c=nested(3, 70, 65, 3, 5), seed=30 + n)
        t.append(("four-ragged-tiles-" + lid, four))
    t.append(("k-16", lambda: Case(2, 3, 33, 20, 16, tb=True, seed=40)))
    t.append(("k-17", lambda: Case(2, 3, 33, 20, 17, tb=True, seed=41)))
    t.append(("scores-in-row-16-byte", lambda: scores_in_row(16, 20, 0, 42)))
    t.append(("scores-in-row-odd", lambda: scores_in_row(17, 19, 1, 43)))
    t.append(("context-in-row-16-byte", lambda: context_in_row(20, 16, 0, 44)))
    t.append(("context-in-row-odd", lambda: context_in_row(19, 17, 1, 45)))
    for name, kw in (("a-outer", {"share_a": (0,)}), ("a-inner", {"share_a": (1,)}), ("b-outer", {"share_b": (0,)}), ("b-inner", {"share_b": (1,)})):
        t.append(("stride-0-" + name, lambda kw=kw: Case(2, 3, 40, 24, 12, seed=50, **kw)))
    for n, ((ta, tb), lid) in enumerate(zip(LAYOUTS, LAYOUT_IDS)):
        t.append(("even-16-byte-" + lid, lambda ta=ta, tb=tb, n=n: even_case(ta, tb, seed=60 + n)))
        t.append(("even-offset-1-" + lid, lambda ta=ta, tb=tb, n=n: even_case(ta, tb, offset=1, seed=64 + n)))
    for n, odd in enumerate(("a0", "a1", "b0", "b1")):
        t.append(("odd-stride-" + odd, lambda odd=odd, n=n: even_case(False, n % 2 == 1, odd=odd, seed=70 + n)))
    t.append(("accumulate-bias", lambda: Case(2, 3, 70, 40, 33, accumulate=True, bias=True, c=nested(3, 70, 40, 3, 5), seed=80)))
    # one row per item, interleaved in C with ldc BELOW N: o[b,h,d] for H = 3 heads, item (b, h) is the row at b * 3 * N + h * N;
    # ldc addresses nothing when M == 1
    t.append(("one-row-ldc-below-n", lambda: Case(2, 3, 1, 20, 19, c=(7, 3 * 20, 20), seed=83)))
    t.append(("batch0-1", lambda: Case(1, 5, 33, 20, 19, tb=True, seed=81)))
    t.append(("batch1-1", lambda: Case(5, 1, 33, 20, 19, ta=True, seed=82)))
    return t
