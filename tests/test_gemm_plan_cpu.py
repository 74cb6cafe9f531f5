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
