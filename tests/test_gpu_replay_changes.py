"""Captured steps after every change of what their graphs bake in.

A launch range on the context's stream runs eagerly once, is captured on its second run and replayed afterwards (host/run.cpp
run_range; host/fit.cpp launch_group for groups of batches).  Whatever lands in a kernel argument is baked into the graph:

    baked in                          lands in                                     what sends the next call back to a capture
    --------------------------------  -------------------------------------------  ------------------------------------------------
    input pointers                    tensor_ptr of an input                       Captured::stamp != eg_model::inputs_gen (every
                                                                                   bind, clear and fit bumps it), then the key's
                                                                                   `tensor=pointer;` entries
    input shapes                      grids, extents, arena offsets                a plan per shape signature (plan.cpp shape_key);
                                                                                   graphs belong to their plan
    the context's four scratch blocks workspace, aux, side_workspace, side_aux     Captured::ptrs[0..3], the key's w / x / s / y
    the gradient bucket               tensor_ptr of a parameter gradient           Captured::ptrs[4], the key's b
    the gradient scale                the seed fill, GS of generated kernels, the  Captured::grad_scale (the float itself), the
                                      epilogue operand block                       key's g: the scale's BIT PATTERN
    the epoch                         EP of generated kernels, epoch slots, the    Captured::epoch, the key's e; a program with
                                      epilogue operand block                       epoch() in a host value gets a plan per epoch
    the plan's arena                  tensor_ptr of every result                   graphs live in the Plan and die with it
                                                                                   (release_plan)
    keep_values                       which plan                                   shape_key's v, inputs_gen
    parameters, caches, rng state     fixed addresses for the model's life         nothing: params[tid] = ..., load_state and set_seed
                                                                                   rewrite the contents in place, replays read them
    fit's group graph                 all of the above, per batch of the group     the same key + plan, group size and launch count;
                                                                                   its copy nodes / the sample kernel's input
                                                                                   arguments are re-pointed before every launch

Every scenario of tests/replay_cases.py is held to three checks:

  * the same sequence issued launch by launch (ONE child process per module, EG_NO_GRAPH=1, all scenarios, one .npz; the
    child runs every scenario twice and reports run-to-run differences): parameters, caches, bucket and random tensors after EVERY
    call, bit for bit;
  * the oracle at the end of the scenario: float32 models through parity.Trio.check (oracle and float64 shadow step through the
    same sequence), float64 models against the oracle's compile[float64] form at the 1e-12 of tests/test_gpu_f64.py; the
    oracle of a dropout net is handed, call by call, the masks the GPU drew (as tests/test_dropout.py does) — catches a
    change that both routes ignore;
  * not vacuous: under EG_DEBUG_GRAPH=1 the lines `captured N nodes for slot S of target T` and `fit group of ...` are counted
    per phase; "capture" = the phase must capture (first use, or a change that the graph bakes in), "none" = the replay is
    right as it stands and nothing may be captured.  Asserted only when conftest.debug_toggles_active() is false.

Scenarios whose eager twin is not reproducible run to run would be compared within the oracle bound only; there are none: the
child lists such scenarios as `unstable` and each test asserts that its own is not among them, so a kernel that starts to sum in
arrival order shows up here by name.

Phases and expected captures (three calls per phase unless noted; `-s` prints the measured counts next to them):

    scale_apply, scale_apply_adam, scale_split, scale_f64, scale_mlp   scale 1.0 capture | 0.25 capture | 1.0 (2 calls) capture
    scale_fit (2 fits per phase, EG_FIT_GROUP=5)                       the same; every phase also captures a fit group
    scale_pair_{apply,split,f64,fit}                                   p0 capture | p1 capture | p0 capture, where p0 and p1 print
                                                                       alike with six digits (the key used to hold six digits:
                                                                       p1 replayed p0's graph)
    epoch_kernel_argument (adam)                                       epoch 1 capture | 2 capture | 1 (2 calls) capture
    epoch_kernel_argument_pool (pool_chain_adam)                       the same
    epoch_host_value                                                   epoch 1 capture | 2 capture | 1 capture (the released plan
                                                                       is rebuilt)
    pointer_device                                                     a capture | b capture | a (2 calls) capture | a rewritten
                                                                       in place none
    pointer_host                                                       capture | new values on every call none
    shape_host, shape_adam, shape_f64                                  64 capture | 200 capture | 64 (2 calls) capture (the staging
                                                                       buffers were regrown: the old graph names freed memory)
    shape_device                                                       64 capture | 200 capture | 64 none (live tensors)
    scratch_stranger (own context, batch 497: k-sliced weight          capture | after eg_sgemm regrew the workspace capture
    gradient)
    scratch_two_models (own context)                                   small capture | large capture | small capture |
                                                                       alternating none
    gradient_bucket                                                    library's capture | torch bucket capture | another capture
    keep_values                                                        off capture | on capture | off none
    params_rewritten                                                   capture | params[tid] = ... none
    state_reloaded                                                     capture | six calls around load_state none
    seed_between_replays (dropout inside the MLP: the net of           seed 5 capture | seed 99 none | fresh model capture
    tests/test_dropout.py is one launch, which is never captured)
    fit_apply_fashion, fit_apply_dense (EG_FIT_GROUP=5)                fit capture | applies - | fit of another row count capture |
                                                                       apply -
"""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import replay_cases as rc
from conftest import debug_toggles_active
from parity import Trio

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL64 = 1e-12
CAPTURED = re.compile(r"captured \d+ nodes for slot \d+ of target \S+")
FIT_GROUP = re.compile(r"fit group of \d+ batches")


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """The eager twin: one fresh process for the whole module."""
    out = str(tmp_path_factory.mktemp("replay") / "eager.npz")
    env = dict(os.environ, EG_NO_GRAPH="1")
    env.pop("EG_DEBUG_GRAPH", None)
    t0 = time.time()
    child = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "replay_cases.py"), out], cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=900)
    assert child.returncode == 0 and "TWIN-OK" in child.stdout, child.stdout[-3000:] + child.stderr[-4000:]
    print("\neager twin: %.1f s\n%s" % (time.time() - t0, child.stdout))
    return np.load(out)


def first_difference(name, got, twin):
    """The first record (in call order) whose bits differ from the twin's, described; None when all agree."""
    prefix = name + "|"
    want = {k[len(prefix):]: twin[k] for k in twin.files if k.startswith(prefix)}
    if sorted(want) != sorted(got):
        return "records differ: %s" % sorted(set(want) ^ set(got))[:6]
    bad = [k for k in sorted(got) if not rc.same_bits(got[k], want[k])]
    if not bad:
        return None
    k = bad[0]
    a, b = np.asarray(got[k], np.float64).ravel(), np.asarray(want[k], np.float64).ravel()
    off = a != b
    scale = max(float(np.max(np.abs(b))), 1e-300)
    return ("%d of %d records differ from the eager twin, first: model.call.what = %s (%d of %d elements, largest difference %.3g of the "
            "largest value); then %s" % (len(bad), len(got), k, int(off.sum()), a.size, float(np.max(np.abs(a - b))) / scale, bad[1:5]))


def check_state_against_the_oracle(name, S):
    O = rc.run_on_oracle(name, S.out)
    assert len(O.models) == len(S.finals)
    for i, (om, got) in enumerate(zip(O.models, S.finals)):
        for what, ref, exact in om.final():
            label = "%s: model %d %s at the end" % (name, i, what)
            if exact is None:       # a float64 model against the oracle's compile[float64] form
                scale = max(float(np.max(np.abs(ref))), 1e-300)
                err = float(np.max(np.abs(got[what] - ref))) / scale
                assert np.all(np.isfinite(got[what])) and err <= TOL64, (label, err)
            else:
                Trio.check(got[what], ref, exact, what=label)


def records_of(out, model, call):
    tag = "%d.%02d." % (model, call)
    return {k[len(tag):]: v for k, v in out.items() if k.startswith(tag)}


def same_records(a, b):
    return sorted(a) == sorted(b) and all(rc.same_bits(a[k], b[k]) for k in a)


def check_properties(name, out, twin):
    """What a scenario promises beyond agreeing with its twin."""
    if name in rc.PAIRS:
        assert rc.probes_differ(out), "one step with p0 and one with p1 must differ in bits"
    if name == "state_reloaded":        # calls 6 to 8 repeat calls 3 to 5
        for c in (3, 4, 5):
            assert same_records(records_of(out, 0, c), records_of(out, 0, c + 3)), ("call", c + 3, "does not repeat call", c)
        assert not same_records(records_of(out, 0, 2), records_of(out, 0, 5))
    if name == "seed_between_replays":  # the masks after set_seed are those of a fresh model with that seed
        for c in range(3):
            assert same_records(records_of(out, 0, 3 + c), records_of(out, 1, c)), ("call", 3 + c, "after set_seed")
        masks = [v for k, v in sorted(out.items()) if k.startswith("0.") and ".mask" in k]
        assert len(masks) == 6 and all(0.0 <= m.min() and m.max() < 1.0 for m in masks)
        assert all(not rc.same_bits(masks[i], masks[j]) for i in range(6) for j in range(i)), "a mask was drawn twice"
    if name == "keep_values":           # toggling keep_values changes no bit: the twin that never toggles
        never = {k[len("keep_values_never|"):]: twin[k] for k in twin.files if k.startswith("keep_values_never|")}
        assert same_records(out, never), "keep_values changed a result"


@pytest.mark.parametrize("name", list(rc.SCENARIOS))
def test_scenario(gpu_ctx, twin, monkeypatch, capfd, name):
    _, env, oracle = rc.SCENARIOS[name]
    monkeypatch.setenv("EG_DEBUG_GRAPH", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()

    def captures_since_the_last_mark():
        err = capfd.readouterr().err
        return len(CAPTURED.findall(err)), len(FIT_GROUP.findall(err))

    t0 = time.time()
    S = rc.run_on_gpu(name, gpu_ctx, captures_since_the_last_mark)
    seconds = time.time() - t0
    with capfd.disabled():
        print("\n%-28s %.2f s  " % (name, seconds) + " | ".join("%s: %d range%s, %d fit group%s [%s]" % (
            label, ncap, "" if ncap == 1 else "s", nfit, "" if nfit == 1 else "s", expect or "-") for label, expect, ncap, nfit in S.phases))
    assert name not in list(twin["unstable"]), "the eager twin of this scenario is not reproducible run to run"
    failures = []
    if not debug_toggles_active():
        for label, expect, ncap, nfit in S.phases:
            if expect == "capture" and ncap + nfit < 1:
                failures.append("phase '%s' captured nothing: it replayed a graph made for other values, or never captures" % label)
            if expect == "none" and ncap + nfit > 0:
                failures.append("phase '%s' captured %d graph(s) where the replay is right as it stands" % (label, ncap + nfit))
    diff = first_difference(name, S.out, twin)
    if diff:
        failures.append(diff)
    assert not failures, "\n".join([name] + failures)
    check_properties(name, S.out, twin)
    if oracle == "state":
        check_state_against_the_oracle(name, S)
