"""The float64 convolution entry points at the drop-in boundary, without a device: the built library exports them,
include/exprgrad_hip.h declares them with the argument lists of their float32 namesakes over double, exprgrad_amd._lib
binds them and exprgrad_amd.ops wraps them; a NULL context is refused with a message before anything touches a device;
the switch that turns the implicit-GEMM kernel off is in the closed table."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "exprgrad_hip.h")
EG_ERR_INVALID = 1
PAIRS = {"eg_conv2_nhwc_f64": "eg_conv2_nhwc", "eg_conv2_nhwc_grad_filter_f64": "eg_conv2_nhwc_grad_filter",
         "eg_conv2_nhwc_grad_image_f64": "eg_conv2_nhwc_grad_image"}


def declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text)
    assert m, name + " is not declared in the header"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_declared_like_the_float32_form(name):
    d, s = declaration(name), declaration(PAIRS[name])
    assert d == [a.replace("float", "double") for a in s] and len(d) == 12


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_exported_and_bound(name):
    from exprgrad_amd import _lib, ops
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert name in {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert name in _lib.declared_symbols()
    assert len(getattr(_lib.lib(), name).argtypes) == len(getattr(_lib.lib(), PAIRS[name]).argtypes) == 12
    assert callable(getattr(ops, name[len("eg_"):]))


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_null_context_is_refused_without_a_device(name):
    from exprgrad_amd import _lib
    null = ctypes.c_void_p(0)
    rc = getattr(_lib.lib(), name)(null, 1, 9, 10, 17, 17, 3, 3, null, null, null, 0)
    assert rc == EG_ERR_INVALID
    assert name in _lib.last_error()


def test_the_switch_is_in_the_table():
    from exprgrad_amd import _lib
    n = _lib.lib().eg_switch_table(None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    _lib.lib().eg_switch_table(buf, n + 1)
    rows = {r.split("\t")[0]: r.split("\t")[1] for r in buf.value.decode().splitlines()}
    assert rows.get("EG_CONV_NO_MFMA64") == "execution"
