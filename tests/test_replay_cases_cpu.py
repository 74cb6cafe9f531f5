"""What tests/replay_cases.py chose on the CPU, held to the tools it was chosen with: the colliding pair of gradient scales,
the batch at which the dense net's weight gradient runs in k-slices (the planner, through tests/gemm_plan_driver.cpp), the
library call that regrows the workspace, and every scenario once on the oracle."""
import numpy as np

import replay_cases as rc
from test_gemm_plan_cpu import _plans


def test_the_pair_prints_alike_and_differs_as_floats():
    p0, p1 = rc.colliding_pair()
    a, b = np.float32(p0), np.float32(p1)
    assert float(a) == p0 and float(b) == p1            # both are float32 values: nothing is lost on the way into the C ABI
    assert a != b and a.view(np.uint32) != b.view(np.uint32)
    assert "%g" % p0 == "%g" % p1                       # ostream's default: six significant digits
    assert "%.9g" % p0 != "%.9g" % p1
    # four ulps apart: a product with one differs from the product with the other for any float32 operand
    assert int(b.view(np.uint32)) - int(a.view(np.uint32)) == 4


def test_the_workspace_batch_is_the_first_with_k_slices(tmp_path):
    """Scenario 6 needs a step that uses the context's workspace: the first layer's weight gradient [24, 32] over the batch."""
    cases = [rc.weight_gradient_case(k) for k in range(1, rc.WS_BATCH + 1)]
    plans = _plans(tmp_path, cases)
    assert all(int(p["splits"]) == 1 and int(p["workspace_floats"]) == 0 for p in plans[:-1])
    assert int(plans[-1]["splits"]) > 1 and int(plans[-1]["workspace_floats"]) == rc.WS_MODEL_FLOATS
    # the two-model scenario: the wide net's weight gradient at four times the batch needs more than the block the small one
    # leaves behind (ensure_workspace allocates a quarter more than it is asked for)
    wide = _plans(tmp_path, [rc.weight_gradient_case(4 * rc.WS_BATCH, 48, 64)])[0]
    assert int(wide["splits"]) > 1 and int(wide["workspace_floats"]) > 2 * rc.WS_MODEL_FLOATS


def test_the_stranger_regrows_the_workspace(tmp_path):
    c = rc.stranger_case()
    assert c["mode"] == "exact" and int(c["expect"]["splits"]) > 1
    assert int(c["expect"]["workspace_floats"]) >= 16 * rc.WS_MODEL_FLOATS
    plan = _plans(tmp_path, [c])[0]                     # (the table is what the planner says today)
    assert plan["splits"] == str(c["expect"]["splits"]) and plan["workspace_floats"] == str(c["expect"]["workspace_floats"])
    # every operand of the call stays inside what GpuSession.stranger allocates
    M, N, K = c["M"], c["N"], c["K"]
    assert c["lda"] == (M if c["ta"] else K) and c["ldb"] == (K if c["tb"] else N) and c["ldc"] == N


def test_every_scenario_runs_on_the_oracle():
    for name, (_, _, oracle) in rc.SCENARIOS.items():
        if oracle != "state":
            continue
        S = rc.run_on_oracle(name)
        assert S.models, name
        for m in S.models:
            for what, ref, exact in m.final():
                assert np.all(np.isfinite(ref)), (name, what)
                assert exact is None or np.all(np.isfinite(exact)), (name, what)

