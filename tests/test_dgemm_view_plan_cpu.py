"""What the float64 half of tests/test_gpu_gemm_views.py covers, stated on the CPU: the float64 table of
tests/gemm_view_cases.py through plan_dgemm (exprgrad_amd/csrc/kernels/gemm_plan.cpp next to tests/dgemm_plan_driver.cpp,
plain g++).  Nothing new is asserted about the planner (tests/golden/dgemm_routes.json does that); the assertions are about
the table: every forced case ends on the tile its name says, sliced wherever it names four slices, both load forms run on
every tile, and the default case is sliced by the library's own choice."""
import pytest

import gemm_view_cases as views
from test_dgemm_plan_cpu import dgemm_plans


@pytest.fixture(scope="module", params=[64, 256, 304])
def planned(request, tmp_path_factory):
    cases = views.f64_table()
    return cases, dgemm_plans(tmp_path_factory.mktemp("dgemm_view_plans"), [c.dgemm_driver_case(request.param) for c in cases])


def test_every_forced_case_ends_where_its_name_says(planned):
    cases, plans = planned
    forced = [(c, p) for c, p in zip(cases, plans) if "EG_DGEMM_TILE" in c.env]
    assert len(forced) == len(cases) - 1
    for c, p in forced:
        config, slices = (int(v) for v in c.env["EG_DGEMM_TILE"].split(","))
        assert c.name.startswith("tile%d-slices%d-" % (config, slices)) and slices in (1, 4)
        assert p["config"] == config, (c.name, p)
        if slices == 4:
            assert p["splits"] > 1 and p["reduce"] == 1 and p["workspace_doubles"] == p["splits"] * c.dims[0] * c.dims[1], (c.name, p)
        else:
            assert p["splits"] == 1 and p["reduce"] == 0 and p["workspace_doubles"] == 0, (c.name, p)
    seen = {(p["config"], p["splits"] > 1, p["vec"]) for _, p in forced}
    assert seen == {(k, s, v) for k in (0, 1, 2) for s in (False, True) for v in (0, 1)}
    assert {p["splits"] for _, p in forced} >= {1, 2, 4}            # K = 17 holds two slices of one k-tile


def test_bases_off_their_alignment_take_8_byte_loads(planned):
    """Whatever the leading dimensions: kind ab_off has A and B one double off."""
    cases, plans = planned
    off = [p for c, p in zip(cases, plans) if c.kind == "ab_off"]
    assert len(off) == 3 * 2 * 3 * 4 and all(p["vec"] == 0 for p in off)


def test_the_default_case_is_sliced_by_the_library(planned):
    cases, plans = planned
    (c, p), = [(c, p) for c, p in zip(cases, plans) if c.kind == "default"]
    assert c.name == "default-64x48x40000-NN" and not c.env
    assert (p["config"], p["splits"], p["k_per_split"], p["reduce"]) == (2, 63, 640, 1) and c.ldc != c.dims[1]
