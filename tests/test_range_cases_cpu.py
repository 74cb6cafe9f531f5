"""tests/range_cases.py held to the project's own oracle before any GPU sees it (no GPU, no HIP).

For every case of every table the float64 reference and oracle/refcpu.c agree on the unpadded values within the bound the
GPU test uses (RangeCase.check with the oracle's result embedded in the case's own written allocation), so the inputs keep
the reference side inside the bounds; eg_colsum_f64 has no oracle entry and is held to an 80-bit sum instead.  The checker
itself must catch a planted stray store in the front guard, in the gap and directly behind the range, and a planted NaN
inside.  The tables' claims about routes are asserted as far as they can be without a device: pointer alignment,
n >= 4, cols % 4, rows >= 64, and COLSUM_ROUTES against the dispatch restated in colsum_route().
"""
import numpy as np
import pytest

import range_cases as rc
from range_cases import GUARD, SENTINEL


def oracle_result(refcpu, c):
    """The oracle's float32 result of the case on the unpadded values (start values included when it accumulates)."""
    v, a = c.values(), c.args
    out = np.array(v[c._start_key], dtype=np.float32) if c.accumulate else np.zeros(v[c._start_key].shape, dtype=np.float32)
    f = c.family
    if f == "map":
        return refcpu.map_(a["op"], v["in"], a["param"], out=out)
    if f == "map_grad":
        return refcpu.map_grad(a["op"], v["in"], v["gout"], a["param"], out=out)
    if f == "axpy":
        return refcpu.axpy(a["alpha"], v["x"], out)
    if f == "fill":
        return np.full(a["n"], a["value"], dtype=c.dtype)
    if f == "bias_add":
        return refcpu.bias_add(v["bias"], out)
    if f == "sum":
        return refcpu.total(v["in"], out=out)
    if f == "rowsum":
        return refcpu.rowsum(v["in"], out=out)
    if f == "colsum":
        return refcpu.colsum(v["in"], out=out)
    if f == "colsum_f64":       # no oracle entry: the sum in extended precision, rounded once
        s = v["in"].astype(np.longdouble).sum(axis=0)
        return (s + (v[c._start_key].astype(np.longdouble) if c.accumulate else 0)).astype(np.float64)
    if f == "conv_fwd":
        return refcpu.conv2_nhwc(v["img"], v["flt"], out=out, threads_n=8)
    if f == "conv_gf":
        return refcpu.conv2_nhwc_grad_filter(v["img"], v["gout"], v["flt"].shape, out=out)
    if f == "conv_gi":
        return refcpu.conv2_nhwc_grad_image(v["flt"], v["gout"], v["img"].shape, out=out)
    raise KeyError(f)


def as_allocation(c, result):
    """`result` placed in the case's written allocation as a correct kernel would leave it."""
    return rc.embed(np.asarray(result, dtype=c.dtype), c.offs[c.written], c.dtype.type(SENTINEL))


def hold_to_oracle(refcpu, cases):
    """One oracle run per distinct problem: the values do not depend on the offsets."""
    seen, worst = {}, 0.0
    for c in cases:
        problem = (c.family, c.key, c.accumulate)
        if problem not in seen:
            seen[problem] = oracle_result(refcpu, c)
        worst = max(worst, c.check(as_allocation(c, seen[problem])))
    return worst


TABLES = {
    "map": rc.map_cases, "map_grad": rc.map_grad_cases, "axpy": rc.axpy_cases, "fill": rc.fill_cases, "fill_f64": rc.fill_f64_cases,
    "bias_add": rc.bias_cases, "sum": rc.sum_cases, "rowsum": rc.rowsum_cases, "colsum": rc.colsum_cases,
    "colsum_no_slab": rc.colsum_no_slab_cases, "colsum_f64": rc.colsum_f64_cases,
}


@pytest.mark.parametrize("table", sorted(TABLES))
def test_reference_agrees_with_the_oracle(refcpu, table):
    cases = TABLES[table]()
    assert cases and len({c.name for c in cases}) == len(cases)      # the names serve as test ids
    hold_to_oracle(refcpu, cases)


@pytest.mark.parametrize("shape", rc.CONV_SHAPES, ids=lambda s: s.id)
def test_convolution_references_agree_with_the_oracle(refcpu, shape):
    for call in rc.CONV_CALLS:
        hold_to_oracle(refcpu, shape.cases(call).values())


def sample_cases():
    return [rc.RangeCase("map", (1, 2), False, op="tanh", param=0.0, n=37), rc.RangeCase("colsum", (0, 3), True, rows=9, cols=5),
            rc.RangeCase("colsum_f64", (1, 1), True, rows=9, cols=5), rc.RangeCase("fill", (3,), n=6, value=1.5, dtype="float32")]


@pytest.mark.parametrize("c", sample_cases(), ids=repr)
def test_the_checker_catches_planted_stray_stores_and_a_nan(c):
    good = as_allocation(c, c.want())
    c.check(good)
    lo, n = c.first(c.written), c.result_size()
    for at, where in ((17, "front guard"), (GUARD + c.offs[c.written] - 1, "gap"), (lo + n, "back guard, 1 elements behind")):
        bad = good.copy()
        bad[at] = 3.0
        with pytest.raises(AssertionError, match=where):
            c.check_outside(bad)
        with pytest.raises(AssertionError, match=where):
            c.check(bad)
    flipped = good.copy()                         # one changed bit of a sentinel is a change
    flipped.view(np.uint32 if c.dtype == np.float32 else np.uint64)[lo + n + GUARD - 1] ^= 1
    with pytest.raises(AssertionError, match="back guard, %d elements behind" % GUARD):
        c.check_outside(flipped)
    nan = good.copy()
    nan[lo + n // 2] = np.nan
    c.check_outside(nan)
    with pytest.raises(AssertionError, match="NaN or Inf"):
        c.check(nan)
    wrong = good.copy()
    wrong[lo] += 1.0
    with pytest.raises(AssertionError, match="exceeds"):
        c.check(wrong)


def test_buffers_are_laid_out_as_the_module_says():
    c = rc.RangeCase("map_grad", (1, 2, 3), False, op="relu", param=0.0, n=5)
    b = c.buffers()
    assert list(b) == ["in", "gout", "gin"]
    for name, off in (("in", 1), ("gout", 2), ("gin", 3)):
        assert b[name].size == GUARD + off + 5 + GUARD and c.first(name) == GUARD + off
    assert np.isnan(b["in"][:GUARD + 1]).all() and np.isnan(b["in"][GUARD + 6:]).all() and np.isfinite(b["in"][GUARD + 1:GUARD + 6]).all()
    assert (b["gin"][:GUARD + 3] == SENTINEL).all() and (b["gin"][GUARD + 8:] == SENTINEL).all() and np.isnan(b["gin"][GUARD + 3:GUARD + 8]).all()
    acc = rc.RangeCase("map_grad", (1, 2, 3), True, op="relu", param=0.0, n=5)
    assert np.array_equal(acc.buffers()["gin"][GUARD + 3:GUARD + 8], acc.values()["start"])
    assert np.array_equal(acc.values()["in"], c.values()["in"])          # the same problem
    y = rc.RangeCase("axpy", (0, 1), n=5, alpha=-0.1)
    assert y.accumulate and np.isfinite(y.buffers()["y"][GUARD + 1:GUARD + 6]).all()
    assert GUARD % 4 == 0 and rc.aligned(0) and not any(rc.aligned(o) for o in (1, 2, 3))
    assert rc.aligned(0, np.float64) and not rc.aligned(1, np.float64) and rc.aligned(2, np.float64)


def test_elementwise_tables_reach_both_paths_from_every_side():
    for cases, operands in ((rc.map_cases(), ("in", "out")), (rc.map_grad_cases(), ("in", "gout", "gin")), (rc.axpy_cases(), ("x", "y"))):
        by = {}
        for c in cases:
            by.setdefault((c.args.get("op"), c.args["n"], c.pattern), c)
            assert rc.elementwise_vector_path(c) == (c.pattern == "aligned" and c.args["n"] >= 4), c
        for o in operands:       # the scalar path forced by this operand alone, on several blocks (70001 = 274 blocks of 256)
            assert any(not c.is_aligned(o) and all(c.is_aligned(p) for p in operands if p != o) and c.args["n"] == 70001 for c in cases), o
        assert {c.args["n"] for c in cases} == set(rc.LENGTHS)
    every = {(c.args["op"], c.args["n"], c.pattern, c.accumulate) for c in rc.map_cases()}
    for op, _ in rc.MAPS:
        for n in (4099, 70001):
            assert all((op, n, pat, acc) in every for pat in ("aligned", "out1") for acc in (False, True)), (op, n)
    assert 4099 == 4 * 1024 + 3 and 12289 == 4 * (3 * 1024) + 1 and -(-70001 // 256) == 274
    for c in rc.bias_cases():
        assert rc.elementwise_vector_path(c) == (c.pattern == "aligned" and c.args["cols"] % 4 == 0)
    # one row, several rows in one block, more than one block of 1024 groups (300 x 132 / 4 = 9900), rows ending inside a group's block
    assert [(c.args["rows"], c.args["cols"]) for c in rc.bias_cases()[::6]] == rc.BIAS_SHAPES and 300 * 132 // 4 > 1024 * 4
    assert {(c.args["cols"] % 4 == 0, c.pattern) for c in rc.bias_cases()} >= {(True, "bias1"), (True, "out2"), (True, "aligned"), (False, "aligned")}


def test_reduction_tables_name_the_kernels_the_dispatch_takes():
    assert {(c.args["n"], c.offs["in"], c.offs["out"], c.accumulate) for c in rc.sum_cases()} == {
        (n, i, o, a) for n in (1, 3, 4, 7, 1027, 70001) for i in (0, 1) for o in (0, 1) for a in (False, True)}
    assert {(c.args["n"] >= 4 and c.is_aligned("in"), c.is_aligned("out")) for c in rc.sum_cases()} == {(a, b) for a in (False, True) for b in (False, True)}
    for (rows, cols), (when_aligned, when_off) in rc.ROWSUM_SHAPES.items():
        assert rc.rowsum_route(rows, cols, True) == when_aligned and rc.rowsum_route(rows, cols, False) == when_off
        assert (when_aligned == "thread") == (cols <= 32) and (when_aligned == "vec") == (cols > 32 and cols % 4 == 0)
    assert {v for pair in rc.ROWSUM_SHAPES.values() for v in pair} == {"thread", "vec", "wave"}
    seen = set()
    for (rows, cols), routes in rc.COLSUM_ROUTES.items():
        for pat, (i, o) in rc.COLSUM_PATTERNS.items():
            route = routes[pat]
            assert rc.colsum_route(rows, cols, rc.aligned(i), rc.aligned(o)) == route, (rows, cols, pat)
            first, final = route.split("+")[0], route.split("+")[1].split("(")[0]
            assert (first == "vec") == (cols % 4 == 0 and rows >= 64 and i == 0), (rows, cols, pat)
            if final == "slab":
                assert cols % 4 == 0 and o == 0
            seen.add((first, final))
    assert seen == {(a, b) for a in ("vec", "scalar") for b in ("slab", "tree", "thread")}
    no_slab = {rc.colsum_route(c.args["rows"], c.args["cols"], True, True, no_slab=True).split("+")[1].split("(")[0] for c in rc.colsum_no_slab_cases()}
    assert no_slab == {"tree", "thread"} and all(c.pattern == "aligned" and c.env == {"EG_NO_SLAB_SUM": "1"} for c in rc.colsum_no_slab_cases())
    assert (70000, 8) not in rc.COLSUM_F64_SHAPES and len(rc.COLSUM_F64_SHAPES) == 8
    names = {c.name for c in rc.colsum_cases() + rc.colsum_f64_cases()}
    for family, rows, cols, pat in rc.TWICE:
        assert any(n.startswith("%s-%d-%d-" % (family, rows, cols)) for n in names)


def test_uniform_fill_tables():
    for dtype in (np.float32, np.float64):
        cases = rc.uniform_cases(dtype)
        assert set(cases) == {(n, off) for n in (1, 5, 1000, 70001) for off in (0, 1)}
        for (n, off), c in cases.items():
            assert c.dtype == dtype and c.result_size() == n and c.is_aligned("out") == (off == 0) and c.first("out") == GUARD + off
    assert rc.UNIFORM_RANGE == (-2.0, 3.0)


def test_convolution_table_has_every_row_pattern_and_call():
    rows = {}
    for s in rc.CONV_SHAPES:
        rows.setdefault(s.row, []).append(s.shape)
        for call in rc.CONV_CALLS:
            cases = s.cases(call)
            assert len(cases) == 10 and {p for p, _ in cases} == set(rc.CONV_PATTERNS)
            for (pat, acc), c in cases.items():
                offs = [c.offs[o] for o in c.inputs + (c.written,)]
                assert tuple(offs) == rc.CONV_PATTERNS[pat] and c.accumulate == acc and c.env == s.env
    assert rows["tiny"] == [(5, 9, 11, 3, 7, 2, 4), (1, 3, 3, 2, 4, 3, 3)]
    assert rows["band"] == [(3, 70, 90, 3, 5, 3, 3), (130, 16, 20, 16, 16, 3, 3)]
    assert rows["direct"] == [(64, 50, 50, 3, 4, 3, 3), (64, 50, 50, 2, 20, 3, 3)]
    assert rows["halo"][:2] == [(2, 130, 70, 32, 64, 3, 3), (3, 100, 120, 48, 48, 2, 3)]
    assert rows["gradf_halo"] == [(1, 34, 34, 64, 64, 3, 3), (2, 40, 70, 32, 96, 3, 3)]
    assert rows["gemm"] == [(2, 20, 20, 32, 64, 3, 3), (2, 7, 9, 5, 6, 3, 2)] and rows["1x1"] == [(3, 6, 6, 4, 8, 1, 1)]
    # the halo kernel's own gate (conv2_halo_suits: patches of 8 x 32 pixels x 64 filters, 70 % full, compute_units / 2 of them)
    def halo(n, ho, wo, f, cus=256):
        ty, tx, tf = -(-ho // 8), -(-wo // 32), -(-f // 64)
        return n * ty * tx * tf >= cus // 2 and (ho * wo) / (ty * 8 * tx * 32) * f / (tf * 64) >= 0.7
    assert not halo(2, 128, 68, 64) and not halo(2, 130, 70, 32) and not halo(3, 99, 118, 48) and not halo(3, 100, 120, 48)
    assert halo(8, 64, 64, 64) and not halo(8, 66, 66, 16)           # 8 x 66 x 66 x 16 -> 64: forward yes, image gradient no
    assert halo(8, 64, 64, 64) and not halo(8, 62, 62, 16)           # 8 x 64 x 64 x 64 -> 16: image gradient yes, forward no
    # tiny limits (conv2_tiny.hip: 6 Mi multiply-adds): 3 x 70 x 90 x 3 -> 5 is below them, hence EG_CONV_NO_TINY on that row
    assert 3 * 68 * 88 * 5 * 27 < 6 << 20 and 3 * 70 * 90 * 3 * 45 < 6 << 20 and 130 * 14 * 18 * 16 * 144 > 6 << 20
