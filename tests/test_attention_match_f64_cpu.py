"""match_attention (csrc/host/match_attention.cpp) on the `kd 1 f64` text of the attention programs, without a device: the
matcher answers for a float64 program what it answers for the float32 one — the group of eg_model_fuse_attention_f64 takes
exactly the chains a float32 model runs as eg_attn, and refuses, for the same reason, what that one refuses.  Built like
tests/test_attention_match_cpu.py (its driver, tests/attention_match_driver.cpp, with the host compiler).  What needs a model
— that eg_model_plan_text carries the eg_attn annotation only with the setting on — is in
tests/test_gpu_attention_model_f64.py."""
import subprocess

import pytest

import attention_fused_programs as fp
import attention_programs as ap
from exprgrad_amd import dsl
from test_attention_match_cpu import REASONS, driver, hits     # noqa: F401 (a fixture)

PROGRAMS = {"forward": fp.attention_forward(), "unscaled": fp.attention_forward_unscaled, "scale_first": fp.attention_forward_scale_first,
            "training": ap.attention_training(*ap.TRAINING_SHAPE)}
PROGRAMS.update({name: row[0] for name, row in fp.NEAR_MISSES.items()})


def rows_of(exe, tmp_path, name, graphs, scalar):
    prog = dsl.to_program(*graphs())
    prog.scalar = scalar
    text = prog.to_text()
    assert text.splitlines()[0].split()[:3] == ["kd", "1", scalar]
    path = str(tmp_path / ("%s_%s.kd" % (name, scalar)))
    with open(path, "w") as f:
        f.write(text)
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return [dict(kv.split("=", 1) for kv in line.split()) for line in out.stdout.splitlines()]


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_the_float64_text_matches_where_the_float32_text_does(driver, tmp_path, name):
    f32, f64 = rows_of(driver, tmp_path, name, PROGRAMS[name], "f32"), rows_of(driver, tmp_path, name, PROGRAMS[name], "f64")
    assert f64 == f32 and f64, name
    if name in fp.NEAR_MISSES:
        assert not hits(f64) and [r for r in f64 if r["pos"] == "0"][0]["why"] == REASONS[name]
    else:
        got = hits(f64)
        assert len(got) == 1 and got[0]["pos"] == "0" and got[0]["scale"] == ("1" if name == "unscaled" else "0.125"), f64
        assert not hits(f64, "fit")
