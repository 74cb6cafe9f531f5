"""eg_sgemm_batched2 at the drop-in boundary, without a device: the built library exports it, include/exprgrad_hip.h
declares it with its 22 arguments, exprgrad_amd._lib binds it and exprgrad_amd.ops wraps it; a NULL context is refused with
a message before anything touches a device."""
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


def test_declared_with_two_strides_per_operand():
    d = declaration("eg_sgemm_batched2")
    assert len(d) == 22
    assert d[:8] == ["eg_ctx* ctx", "int trans_a", "int trans_b", "int64_t batch0", "int64_t batch1", "int64_t M", "int64_t N", "int64_t K"]
    assert d[8:12] == ["const float* A", "int64_t lda", "int64_t stride_a0", "int64_t stride_a1"]
    assert d[12:16] == ["const float* B", "int64_t ldb", "int64_t stride_b0", "int64_t stride_b1"]
    assert d[16:] == ["float* C", "int64_t ldc", "int64_t stride_c0", "int64_t stride_c1", "int accumulate", "const float* bias"]


def test_exported_and_bound():
    from exprgrad_amd import _lib, ops
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert "eg_sgemm_batched2" in {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert "eg_sgemm_batched2" in _lib.declared_symbols()
    assert len(_lib.lib().eg_sgemm_batched2.argtypes) == 22
    assert callable(ops.sgemm_batched2)


def test_null_context_is_refused_without_a_device():
    from exprgrad_amd import _lib
    null = ctypes.c_void_p(0)
    rc = _lib.lib().eg_sgemm_batched2(null, 0, 0, 2, 2, 1, 1, 1, null, 1, 2, 1, null, 1, 2, 1, null, 1, 2, 1, 0, null)
    assert rc == EG_ERR_INVALID
    assert "eg_sgemm_batched2" in _lib.last_error()
