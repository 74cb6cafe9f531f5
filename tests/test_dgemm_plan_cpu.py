"""The plain float64 product's planner (exprgrad_amd/csrc/kernels/gemm_plan.cpp: plan_dgemm) on the CPU: compiled with
plain g++ next to a small driver (tests/dgemm_plan_driver.cpp), its plans must match tests/golden/dgemm_routes.json — the
config, tile, 16-byte-load decision, k-slices, tiles, XCD remap, grid and workspace that eg::gemm::dgemm() decided inline
(tile model, EG_DGEMM_TILE, slice normalisation, launch_one) before the planner was split out of it.  That code was copied
into a host program and run over the table; the program is not kept, the table is."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dgemm_routes.json")
RECORDED = ("config", "bm", "bn", "vec", "splits", "k_per_split", "tiles_m", "tiles_n", "remap", "grid", "workspace_doubles", "reduce")
TILES = {0: (128, 128), 1: (128, 64), 2: (64, 64)}


def force_of(tile):
    """EG_DGEMM_TILE's text ('-': unset) as gemm_f64_mfma.hip hands it to the planner: `<config>[,<slices>]`, a slice count
    below 1 is 1, and without a count the model's slices stay (0)."""
    if tile == "-":
        return -1, 0
    config, comma, slices = tile.partition(",")
    return int(config), (max(int(slices), 1) if comma else 0)


def dgemm_plans(tmp_path, cases):
    """cases: dicts with M N K lda ldb a b cus tile -> one dict of the driver's fields per case (grid as text, the rest int)."""
    exe = str(tmp_path / "dgemm_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "exprgrad_amd", "csrc", "kernels", "gemm_plan.cpp"),
                           os.path.join(ROOT, "tests", "dgemm_plan_driver.cpp"), "-o", exe])
    lines = ["%d %d %d %d %d %d %d %d %d %d" % ((c["M"], c["N"], c["K"], c["lda"], c["ldb"], c["a"], c["b"], c["cus"]) + force_of(c["tile"]))
             for c in cases]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    plans = [{k: (v if k == "grid" else int(v)) for k, v in (kv.split("=", 1) for kv in l.split())} for l in out.stdout.splitlines()]
    assert len(plans) == len(cases)
    return plans


def _name(c):
    return "%dx%dx%d lda=%d ldb=%d a=%d b=%d cus=%d tile=%s" % (c["M"], c["N"], c["K"], c["lda"], c["ldb"], c["a"], c["b"], c["cus"], c["tile"])


def test_plans_match_the_recorded_decisions(tmp_path):
    cases = json.load(open(GOLDEN))["cases"]
    bad = []
    for c, p in zip(cases, dgemm_plans(tmp_path, cases)):
        assert set(c["expect"]) == set(RECORDED), _name(c)
        for k, want in c["expect"].items():
            if p.get(k) != want:
                bad.append("%s: %s = %s, recorded %s" % (_name(c), k, p.get(k), want))
        if (p["wr"], p["wc"]) != ((4, 2) if p["config"] == 1 else (2, 4)):      # the template arguments of the three tiles
            bad.append("%s: wave grid %d x %d" % (_name(c), p["wr"], p["wc"]))
    assert not bad, "\n".join(bad[:40])


def _find(cases, M, N, K, cus, tile="-"):
    hits = [c for c in cases if (c["M"], c["N"], c["K"], c["cus"], c["tile"]) == (M, N, K, cus, tile) and c["lda"] == K and c["ldb"] == N
            and c["a"] == c["b"] == 1]
    assert len(hits) == 1, (M, N, K, cus, tile, len(hits))
    return hits[0]["expect"]


def test_table_covers_every_config_sliced_and_not():
    cases = json.load(open(GOLDEN))["cases"]
    assert len(cases) >= 150 and {c["cus"] for c in cases} == {64, 256, 304}
    own = [c for c in cases if c["tile"] == "-"]
    assert {(c["expect"]["config"], c["expect"]["splits"] > 1) for c in own} == {(k, s) for k in (0, 1, 2) for s in (False, True)}
    assert {(c["expect"]["config"], c["expect"]["splits"] > 1) for c in cases if c["tile"] != "-"} == {(k, s) for k in (0, 1, 2) for s in (False, True)}
    assert {c["expect"]["vec"] for c in cases} == {0, 1} and {c["expect"]["remap"] for c in cases} == {0, 1}
    assert any(min(c["M"], c["N"]) == 1 for c in cases)

    def plan(*key, **kw):
        e = _find(cases, *key, **kw)
        return e["config"], e["splits"], e["k_per_split"]

    # every config chosen unsliced and sliced
    assert plan(4096, 4096, 4096, 256) == (0, 1, 4096) and plan(2048, 2048, 2048, 256) == (1, 1, 2048) and plan(1024, 1024, 1024, 256) == (2, 1, 1024)
    assert plan(512, 512, 65536, 64) == (0, 8, 8192) and plan(3000, 200, 5000, 64) == (1, 4, 1264)
    # (64 rows on 128 x 128 tiles would waste half of every tile: the model takes 64 x 64 here, as it does for 64 x 4096 x 4096)
    assert plan(64, 2048, 65536, 64) == (2, 4, 16384) and plan(64, 4096, 4096, 64) == (2, 2, 2048)
    for cus in (64, 256, 304):
        assert plan(130, 70, 1027, cus) == (2, 4, 272)
        assert plan(16, 16, 1 << 20, cus) == (2, 64, 16384)          # the cap of 64 slices
        assert plan(64, 48, 40000, cus) == (2, 63, 640)              # 64 slices asked for, 63 of whole k-tiles hold K
        for K in (0, 1, 17, 255, 256, 511, 512):
            slices, per = plan(65, 63, K, cus)[1:]
            assert slices == 1 if K < 512 else slices <= 2                  # two slices need 256 each
            if slices == 1:
                assert per == max(-(-K // 16) * 16, 16)                     # K = 0 and K = 1: one k-tile
    # forced plans: the count is normalised like the model's own
    assert plan(130, 70, 16, 256, tile="2,4") == (2, 1, 16) and plan(130, 70, 17, 256, tile="2,4") == (2, 2, 16)
    assert plan(130, 70, 100, 256, tile="0,64") == (0, 7, 16)
    assert plan(130, 70, 1027, 256, tile="1") == (1, 4, 272)         # the config alone: the model's slices stay


def test_every_recorded_plan_is_a_launch_that_stays_in_bounds():
    """What the kernels rely on: slices of whole k-tiles that cover K with none empty, slabs for every slice, a grid of
    tiles x slices, and the XCD remap only where it is a permutation."""
    for c in json.load(open(GOLDEN))["cases"]:
        e, (M, N, K) = c["expect"], (c["M"], c["N"], c["K"])
        assert (e["bm"], e["bn"]) == TILES[e["config"]], _name(c)
        assert e["k_per_split"] % 16 == 0 and e["k_per_split"] >= 16 and 1 <= e["splits"] <= 64, _name(c)
        assert e["splits"] * e["k_per_split"] >= K and (e["splits"] - 1) * e["k_per_split"] < max(K, 1), _name(c)
        tiles = -(-M // e["bm"]) * -(-N // e["bn"])
        assert (e["tiles_m"], e["tiles_n"]) == (-(-M // e["bm"]), -(-N // e["bn"])) and e["grid"] == "%dx%d" % (tiles, e["splits"]), _name(c)
        assert e["remap"] == int(tiles % 8 == 0 and tiles >= 16), _name(c)
        assert e["reduce"] == int(e["splits"] > 1) and e["workspace_doubles"] == (e["splits"] * M * N if e["splits"] > 1 else 0), _name(c)
        assert e["vec"] == int(c["lda"] % 2 == 0 and c["ldb"] % 2 == 0 and c["a"] == 1 and c["b"] == 1), _name(c)
