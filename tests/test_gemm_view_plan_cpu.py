"""What tests/test_gpu_gemm_views.py covers, stated on the CPU: the float32 table of tests/gemm_view_cases.py through the
planner (exprgrad_amd/csrc/kernels/gemm_plan.cpp next to tests/gemm_plan_driver.cpp, plain g++, 256 CUs).  Nothing new is
asserted about the planner (tests/golden/gemm_routes.json does that); the assertions are about the table: with padded
leading dimensions it reaches every route, every second pass and every load / store variant, and the padded, aligned
cases run the plan of the tight call on the same shape."""
import pytest

import gemm_view_cases as views
from test_gemm_plan_cpu import ROUTES, _plans

SAME_AS_TIGHT = ("route", "bm", "bn", "kb", "splits", "edge_splits", "tail_tiles", "x_rows", "second")


def _driver_cases(cases):
    out = []
    for c in cases:
        f = c.driver_line().split()
        out.append(dict(zip(("mode", "M", "N", "K", "ta", "tb", "lda", "ldb", "ldc", "a", "b", "c", "bias", "vec"), [f[0]] + [int(x) for x in f[1:14]]),
                        switches=f[14]))
    return out


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    cases = views.f32_table()
    plans = _plans(tmp_path_factory.mktemp("view_plans"), _driver_cases(cases + [c.tight() for c in cases]))
    return cases, plans[:len(cases)], plans[len(cases):]


def test_every_case_is_a_view(planned):
    cases, _, _ = planned
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert c.ldc > c.dims[1] and c.lda > c.ca and c.ldb > c.cb, c.name


def test_padded_cases_reach_every_route_in_two_layouts(planned):
    cases, plans, _ = planned
    layouts = {}
    for c, p in zip(cases, plans):
        layouts.setdefault(p["route"], set()).add((c.ta, c.tb))
    assert set(layouts) == ROUTES
    # skinny runs NN only and extra rows TN only
    assert all(len(v) >= 2 for r, v in layouts.items() if r not in ("skinny", "extra_rows")), layouts


def test_every_shape_reaches_the_route_it_is_in_the_table_for(planned):
    """Removing a route's padded cases from the table fails here or above; a shape whose padded call left its route would
    no longer test it."""
    cases, plans, tight = planned
    for c, p, t in zip(cases, plans, tight):
        assert t["route"] == c.route, (c.name, "tight", t["route"])
        if c.kind in "af":
            assert p["route"] == c.route, (c.name, p["route"])


def test_padded_cases_reach_every_second_pass_and_never_the_tree(planned):
    cases, plans, tight = planned
    assert {p["second"] for p in plans} == {"none", "split_reduce", "tail_reduce", "streamk_fixup"}     # tree needs ldc == N
    assert any(t["second"] == "tree" for t in tight)        # ... and the table has shapes whose tight call takes it


def test_aligned_padding_keeps_the_plan_of_the_tight_call(planned):
    """Layout (a) — and (f), the same with a bias and three different pads — differ from the tight call in the leading
    dimensions only.  The one exception: the tree sum over the slabs needs ldc == N, a padded C takes split_reduce."""
    cases, plans, tight = planned
    seen_tree = 0
    for c, p, t in zip(cases, plans, tight):
        if c.kind not in "af":
            continue
        assert (t["second"] == "tree") == c.tree_when_tight, c.name
        for k in SAME_AS_TIGHT:
            if k == "second" and t[k] == "tree":
                assert p[k] == "split_reduce", c.name
                seen_tree += 1
            else:
                assert p[k] == t[k], (c.name, k, p[k], t[k])
    assert seen_tree >= 3


def test_load_and_store_variants(planned):
    cases, plans, _ = planned
    assert {p["vec"] for p in plans} >= {"4", "41", "1"}
    assert {p["wide_store"] for p in plans} == {"0", "1"}
    assert any(p["vec"] == "1" and p["wide_store"] == "1" for p in plans)      # scalar loads with 16-byte stores
    for second in ("split_reduce", "tail_reduce"):                             # slabs and tail tiles, both load forms
        assert {p["vec"] for p in plans if p["second"] == second} >= {"4", "1"}
    parts = {p["parts"].count("/") + 1 for p in plans if p["route"] == "remainder"}
    assert parts == {2, 3}                                                     # rows alone; rows and columns
    assert {p["x_rows"] for p in plans if p["route"] == "extra_rows"} == {"4", "16"}
    assert {p["edge"] for p in plans if p["route"] == "kw8"} == {"0", "1"}
    assert {p["kb"] for p in plans if p["route"] == "pair"} == {"16", "32"}
    assert any(p["route"] == "generic" and int(p["edge_splits"]) > 0 for p in plans)


def test_kinds_of_the_table(planned):
    """Every shape has the layouts (a), (b) and (d); every shape but the large ones all of them; every route has a case
    with A alone off its alignment; about half the cases accumulate."""
    cases, plans, tight = planned
    by_shape, route_e = {}, set()
    for c, t in zip(cases, tight):
        by_shape.setdefault(c.dims, set()).add(c.kind)
        if c.kind == "e":
            route_e.add(t["route"])
    for dims, kinds in by_shape.items():
        assert kinds >= set(views.BIG_KINDS), dims
        if max(dims[0], dims[1]) < 4096:
            assert kinds == set(views.ALL_KINDS), dims
    assert route_e == ROUTES
    acc = sum(c.accumulate for c in cases)
    assert 0.35 * len(cases) <= acc <= 0.65 * len(cases)
    assert any(c.bias and c.off_bias for c in cases) and any(c.bias and not c.off_bias for c in cases)
    assert any(len({c.pad_a, c.pad_b, c.pad_c}) == 3 for c in cases)
