"""The f32 contraction's planner (exprgrad_amd/csrc/kernels/gemm_plan.cpp) on the CPU: compiled with plain g++ next to a
small driver (tests/gemm_plan_driver.cpp), its plans must match tests/golden/gemm_routes.json — the kernels, tiles,
grids, GemmArgs fields, workspace sizes and second passes the host code launched before the planner was split out of it
(256 CUs)."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_routes.json")
ROUTES = {"small", "skinny", "kw8", "t96", "streamk", "remainder", "extra_rows", "bk32", "pair", "generic"}


def _plans(tmp_path, cases):
    exe = str(tmp_path / "gemm_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "exprgrad_amd", "csrc", "kernels", "gemm_plan.cpp"),
                           os.path.join(ROOT, "tests", "gemm_plan_driver.cpp"), "-o", exe])
    lines = ["%s %d %d %d %d %d %d %d %d %d %d %d %d %d %s" % (c["mode"], c["M"], c["N"], c["K"], c["ta"], c["tb"], c["lda"], c["ldb"], c["ldc"],
                                                             c["a"], c["b"], c["c"], c["bias"], c["vec"], c["switches"]) for c in cases]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    plans = [dict(kv.split("=", 1) for kv in l.split()) for l in out.stdout.splitlines()]
    assert len(plans) == len(cases)
    return plans


def test_plans_match_the_recorded_launches(tmp_path):
    doc = json.load(open(GOLDEN))
    assert doc["cus"] == 256
    cases = doc["cases"]
    plans = _plans(tmp_path, cases)
    bad = []
    for c, p in zip(cases, plans):
        for k, want in c["expect"].items():
            if str(p.get(k)) != str(want):
                bad.append("%s %dx%dx%d ta=%d tb=%d %s: %s = %s, recorded %s" % (c["mode"], c["M"], c["N"], c["K"], c["ta"], c["tb"], c["switches"], k,
                                                                              p.get(k), want))
    assert not bad, "\n".join(bad[:40])


def test_table_covers_every_route_and_both_verdicts():
    cases = json.load(open(GOLDEN))["cases"]
    layouts = {}
    for c in cases:
        r = c["expect"].get("route")
        if r:
            layouts.setdefault(r, set()).add((c["ta"], c["tb"]))
    assert set(layouts) == ROUTES
    # skinny runs NN only and extra rows TN only; every other route is seen in at least two layouts
    assert all(len(v) >= 2 for r, v in layouts.items() if r not in ("skinny", "extra_rows"))
    seconds = {c["expect"].get("second") for c in cases}
    assert {"none", "split_reduce", "tail_reduce", "streamk_fixup", "tree"} <= seconds
    verdicts = {c["expect"]["single"] for c in cases if c["mode"] == "single"}
    assert verdicts == {0, 1}
    forced = {c["switches"].split("=")[0] for c in cases}
    assert {"no_pair", "no_t96", "no_streamk", "no_xrow", "no_bk32", "force_tile"} <= forced


def test_wide_and_direct_store_cases_differ_in_the_store_alone(tmp_path):
    """tests/test_gpu_ops.py::test_wide_and_direct_stores_agree_bit_for_bit compares a run with EG_GEMM_NO_WIDE_STORE=1 to one
    without, bit for bit.  That only says something about the two stores while both runs launch the same kernel: for every
    case the two plans must agree in every field — route, tile, k-slices, second pass — except `wide_store`, 1 and 0, and
    be the plan the case was chosen for."""
    from wide_store_cases import CASES, SWITCHES, case_id
    assert set(SWITCHES) == {"EG_GEMM_NO_PAIR", "EG_GEMM_NO_T96", "EG_GEMM_NO_STREAMK"}
    lines = []
    for M, N, K, layout, tile, _ in CASES:
        ta, tb = int(layout[0] == "t"), int(layout[1] == "t")
        for direct in (False, True):
            switches = "no_pair,no_t96,no_streamk" + (",force_tile=%dx%d" % tile if tile else "") + (",no_wide_store" if direct else "")
            lines.append(dict(mode="exact", M=M, N=N, K=K, ta=ta, tb=tb, lda=M if ta else K, ldb=K if tb else N, ldc=N, a=1, b=1, c=1, bias=1,
                              vec=0, switches=switches))
    plans = _plans(tmp_path, lines)
    for n, case in enumerate(CASES):
        wide, direct = plans[2 * n], plans[2 * n + 1]
        assert (wide["wide_store"], direct["wide_store"]) == ("1", "0"), case_id(case)
        assert {k: v for k, v in wide.items() if k != "wide_store"} == {k: v for k, v in direct.items() if k != "wide_store"}, case_id(case)
        expect = dict(case[5], route=case[5].get("route", "generic"))
        if case[4]:
            expect.update(bm=case[4][0], bn=case[4][1])
        for k, want in expect.items():
            assert wide[k] == str(want), (case_id(case), k, wide[k], want)
