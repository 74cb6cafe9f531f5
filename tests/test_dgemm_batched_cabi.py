"""eg_dgemm_batched at the drop-in boundary, without a device: the built library exports it, include/exprgrad_hip.h
declares it with the argument list of eg_sgemm_batched over double, exprgrad_amd._lib binds it and exprgrad_amd.ops wraps
it; a NULL context is refused with a message before anything touches a device."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "exprgrad_hip.h")
EG_ERR_INVALID = 1


def declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text)
    assert m, name + " is not declared in the header"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_declared_like_the_float32_form():
    d, s = declaration("eg_dgemm_batched"), declaration("eg_sgemm_batched")
    assert d == [a.replace("float", "double") for a in s]
    assert d[3:7] == ["int64_t batch", "int64_t M", "int64_t N", "int64_t K"] and d[-1] == "const double* bias"


def test_exported_and_bound():
    from exprgrad_amd import _lib, ops
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert "eg_dgemm_batched" in {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert "eg_dgemm_batched" in _lib.declared_symbols()
    fn = _lib.lib().eg_dgemm_batched
    assert len(fn.argtypes) == len(_lib.lib().eg_sgemm_batched.argtypes) == 18
    assert callable(ops.dgemm_batched)


def test_null_context_is_refused_without_a_device():
    from exprgrad_amd import _lib
    null = ctypes.c_void_p(0)
    rc = _lib.lib().eg_dgemm_batched(null, 0, 0, 2, 1, 1, 1, null, 1, 1, null, 1, 1, null, 1, 1, 0, null)
    assert rc == EG_ERR_INVALID
    assert "eg_dgemm_batched" in _lib.last_error()
