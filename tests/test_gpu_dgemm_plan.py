"""eg_dgemm launches what plan_dgemm plans.  tests/test_dgemm_plan_cpu.py pins the planner on the CPU; here the launch code
(kernels/gemm_f64_mfma.hip) is tied to it: a product run with the library's own choice and the same product run with
EG_DGEMM_TILE set to the config and slice count that the CPU driver reports for this device's compute units must agree to
the bit — a launch that ignored the plan's splits or k_per_split, or planned something else than the driver, would sum in
another order.  Both are held to the float64 bound of tests/test_gpu_gemm_views.py (tests/gemm_view_cases.py)."""
import ctypes

import numpy as np
import pytest

import gemm_view_cases as views
from exprgrad_amd import _lib
from test_dgemm_plan_cpu import dgemm_plans
from test_gpu_gemm_views import call, set_env

pytestmark = pytest.mark.gpu

SHAPES = [(65, 63, 17), (130, 70, 1027), (257, 129, 1000)]
LAYOUTS = ["NN", "TN"]
SAME = ("config", "bm", "bn", "vec", "splits", "k_per_split", "tiles_m", "tiles_n", "remap", "grid", "workspace_doubles", "reduce")


def case(M, N, K, layout, env=None):
    ta, tb = views.LAYOUTS[layout]
    return views.ViewCase("plan-%dx%dx%d-%s" % (M, N, K, layout), np.float64, M, N, K, ta, tb, accumulate=True, bias=True, seed=M + K, env=env)


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """(M, N, K, layout) -> (the library's plan, the plan under the EG_DGEMM_TILE made from it), on this device's CUs."""
    cu, clock, hbm = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    arch = ctypes.create_string_buffer(64)
    _lib.call("eg_device_props", 0, ctypes.byref(cu), ctypes.byref(clock), ctypes.byref(hbm), arch, 64)
    keys = [(M, N, K, layout) for M, N, K in SHAPES for layout in LAYOUTS]
    tmp = tmp_path_factory.mktemp("dgemm_gpu_plans")
    own = dgemm_plans(tmp, [case(*k).dgemm_driver_case(cu.value) for k in keys])
    tiles = ["%d,%d" % (p["config"], p["splits"]) for p in own]
    forced = dgemm_plans(tmp, [case(*k, env={"EG_DGEMM_TILE": t}).dgemm_driver_case(cu.value) for k, t in zip(keys, tiles)])
    return {k: (p, t, f) for k, p, t, f in zip(keys, own, tiles, forced)}


def test_the_shapes_take_sliced_and_unsliced_plans(planned):
    assert {p["splits"] > 1 for p, _, _ in planned.values()} == {False, True}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_the_librarys_choice_is_the_plan_of_the_cpu_driver(gpu_ctx, monkeypatch, planned, M, N, K, layout):
    own_plan, tile, forced_plan = planned[(M, N, K, layout)]
    assert all(own_plan[k] == forced_plan[k] for k in SAME), (own_plan, tile, forced_plan)
    c = case(M, N, K, layout)
    f = case(M, N, K, layout, env={"EG_TUNING": "1", "EG_DGEMM_TILE": tile})
    try:
        monkeypatch.delenv("EG_DGEMM_TILE", raising=False)
        own = call(gpu_ctx, c)
        set_env(monkeypatch, f)
        forced = call(gpu_ctx, f)
        c.check(own)
        f.check(forced)
        assert np.array_equal(c.a_vals, f.a_vals) and np.array_equal(c.b_vals, f.b_vals) and np.array_equal(c.c_vals, f.c_vals)
        assert np.array_equal(own.view(np.uint64), forced.view(np.uint64)), (own_plan, tile)
    finally:
        c.release()
        f.release()
