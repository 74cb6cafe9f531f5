"""The wide row analysis over collapsed leading axes (csrc/host/rowfuse_wide.cpp: wide_width_of with `lead`,
analyse_wide_kernel with `lead`) on the CPU: a small driver (tests/wide_collapse_driver.cpp) is built with the host compiler
against kd.cpp and the rowfuse_*.cpp units — which shows that the analysis needs no HIP — and fed the programs of
tests/attention_programs.py.  The softmax members must qualify with the right kind and row count, also where the extents
cannot tell the registers apart (I == J, a leading extent equal to W); every near miss must be refused; and the [B, W]
decisions over tests/refcases.py's dense_softmax_net must be those of the commit before collapsed rows existed
(tests/golden/wide_rank2_parent.txt, printed by the same driver built against that commit)."""
import os
import subprocess

import pytest

import attention_programs as ap
import refcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exprgrad_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "wide_rank2_parent.txt")

# dense_softmax_net(n_in, n_hidden, n_out) at batch B: widths at and around the bounds, B == W, one row
RANK2_CASES = [(300, 64), (300, 65), (300, 100), (100, 100), (1, 1000), (7, 4096), (7, 4097)]
N_IN, N_HIDDEN = 24, 16


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("collapse") / "wide_collapse_driver")
    units = [os.path.join(ROOT, "tests", "wide_collapse_driver.cpp")] + [os.path.join(CSRC, u) for u in (
        "host/kd.cpp", "host/codegen.cpp", "host/match.cpp", "host/rowfuse_common.cpp", "host/rowfuse_row.cpp", "host/rowfuse_wide.cpp",
        "host/rowfuse_sample.cpp", "host/rowfuse_sample_conv.cpp", "host/rowfuse_small.cpp", "switches.cpp", "error.cpp")]
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC] + units + ["-o", exe],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def shape_args(shapes):
    return ["%s=%s" % (name, "x".join(str(d) for d in shape)) for name, shape in sorted(shapes.items())]


def lines_of(exe, mode, path, target, shapes):
    out = subprocess.run([exe, mode, path, target] + shape_args(shapes), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return out.stdout.splitlines()


def rows(exe, tmp_path, name, graphs, target, shapes):
    path = str(tmp_path / (name + ".kd"))
    with open(path, "w") as f:
        f.write(refcases.program_text(graphs()))
    return {r["write"]: r for r in (dict(kv.split("=", 1) for kv in line.split()) for line in lines_of(exe, "collapsed", path, target, shapes))}


def rank2_text(exe, tmp_path):
    """What the driver's rank2 mode prints for RANK2_CASES, a header line per case (also how the golden file was made)."""
    text = []
    for batch, n_out in RANK2_CASES:
        path = str(tmp_path / ("dense_%d.kd" % n_out))
        with open(path, "w") as f:
            f.write(refcases.program_text(refcases.dense_softmax_net(N_IN, N_HIDDEN, n_out)))
        text.append("# dense_softmax_net(%d, %d, %d) train, batch %d" % (N_IN, N_HIDDEN, n_out, batch))
        text += lines_of(exe, "rank2", path, "train", {"x": (batch, N_IN), "y": (batch, n_out)})
    return "\n".join(text) + "\n"


@pytest.mark.parametrize("shape", ap.FORWARD_SHAPES)
def test_the_softmax_members_qualify(driver, tmp_path, shape):
    """Fails without the feature (the driver does not build: wide_width_of reports no rows)."""
    B, H, I, J = shape
    got = rows(driver, tmp_path, "forward", ap.softmax_forward, "out", {"s": shape})
    want = {"scaled": "map", "softmax.sums": "rowsum", "softmax": "map"}
    assert set(got) == set(want), got
    for name, kind in want.items():
        r = got[name]
        assert (r["ok"], r["kind"], int(r["R"]), int(r["W"]), r["rows"]) == ("1", kind, B * H * I, J, "%dx%dx%d" % (B, H, I)), r


def test_rank3_rows(driver, tmp_path):
    G, I, J = ap.RANK3_SHAPE
    got = rows(driver, tmp_path, "rank3", ap.softmax_forward_rank3, "out", {"s": ap.RANK3_SHAPE})
    for name, kind in {"scaled": "map", "softmax.sums": "rowsum", "softmax": "map"}.items():
        r = got[name]
        assert (r["ok"], r["kind"], int(r["R"]), int(r["W"]), r["rows"]) == ("1", kind, G * I, J, "%dx%d" % (G, I)), r


@pytest.mark.parametrize("dims", [ap.TRAINING_SHAPE, (2, 3, 70, 70, 16, 16), (2, 70, 5, 70, 8, 8)])
def test_the_training_step_holds_the_forward_and_gradient_kernels(driver, tmp_path, dims):
    """`derive` adds the three gradient kernels of the softmax and the scale's gradient; the products (five loops), the loss
    over the context and the updates of the parameters are no members."""
    B, H, I, J, K, D = dims
    path = str(tmp_path / "step.kd")
    with open(path, "w") as f:
        f.write(refcases.program_text(ap.attention_training(*dims)()))
    got = [dict(kv.split("=", 1) for kv in line.split()) for line in lines_of(driver, "collapsed", path, "fit", {"labels": (B, I, H, D)})]
    members = [r for r in got if r["ok"] == "1"]
    assert all((int(r["R"]), int(r["W"]), r["rows"]) == (B * H * I, J, "%dx%dx%d" % (B, H, I)) for r in members), members
    kinds = [r["kind"] for r in members]
    # forward: scale, sums, normalise; backward: two maps and a row sum from the softmax, one map from the scale
    assert kinds.count("rowsum") == 2 and kinds.count("map") == 5 and len(kinds) == 7, got
    # they form two runs, each around its row sum, with the context product and the loss between them
    positions = [int(r["pos"]) for r in members]
    assert positions[:3] == [positions[0], positions[0] + 1, positions[0] + 2] and positions[3:] == list(range(positions[3], positions[3] + 4)), positions
    assert positions[3] > positions[2] + 1


@pytest.mark.parametrize("name", sorted(ap.NEAR_MISSES))
def test_near_misses_are_refused(driver, tmp_path, name):
    graphs, shapes = ap.NEAR_MISSES[name]
    got = rows(driver, tmp_path, name, graphs, "out", shapes)
    assert got, name
    if name == "maps_only":
        # its members qualify one by one; the planner forms no group without a sum over the row (tests/test_gpu_attention_rows.py)
        assert all(r["ok"] == "1" and r["kind"] == "map" for r in got.values()), got
        return
    # no kernel that sums over the row qualifies, so no run holds one
    assert not [r for r in got.values() if r["ok"] == "1" and r["kind"] != "map"], got
    if name in ("rank5", "width_64", "width_4097"):
        assert all(r["ok"] == "0" for r in got.values()), got


def test_rank2_decisions_are_those_of_the_parent(driver, tmp_path):
    with open(GOLDEN) as f:
        want = f.read()
    got = rank2_text(driver, tmp_path)
    assert got == want
    assert sum("ok=1" in line for line in got.splitlines()) >= 20     # (the fixture does hold wide row kernels)
