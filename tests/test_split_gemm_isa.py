"""Instruction-level check of the split-bf16 product kernel, without a GPU (kernels/gemm_split_bf16.hip).

The product kernel puts two bf16 terms into every v_mfma_f32_16x16x32_bf16 (lane groups 0-1 and 2-3 read different
planes).  This test compiles the file for gfx950 (device code only), disassembles it and checks that the product
kernel's matrix instructions are all of that form (96 per 16-deep k-tile), that no 32x32 form is left, and that it runs
at two waves per SIMD with no scratch and its three LDS stages within the CU's 160 KiB."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exprgrad_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LLVM_BIN = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "lib", "llvm", "bin")
KERNEL = "split_gemm_kernel"


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("isa") / "split.co")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                    "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "--no-gpu-bundle-output", "-c",
                    os.path.join(CSRC, "kernels", "gemm_split_bf16.hip"), "-o", out], check=True, capture_output=True)
    return out


def _tool(name):
    path = os.path.join(LLVM_BIN, name)
    return path if os.path.exists(path) else "/opt/rocm/lib/llvm/bin/" + name


def _kernel_isa(co):
    dis = subprocess.run([_tool("llvm-objdump"), "-d", co], capture_output=True, text=True, check=True).stdout
    body, inside = [], False
    for line in dis.splitlines():
        head = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if head:
            inside = KERNEL in head.group(1) and not head.group(1).endswith(".kd")
            continue
        if inside and line.strip():
            body.append(line.strip())
    assert body, "product kernel not found in the disassembly"
    return body


def _kernel_meta(co):
    notes = subprocess.run([_tool("llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    meta = {}
    for blk in re.split(r"\n  - (?=\.)", notes):    # one YAML map per kernel
        name = re.search(r"^ {4}\.name:\s+(\S+)", blk, re.M)   # the kernel's own, not an argument's
        if not name or KERNEL not in name.group(1):
            continue
        for key in ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count", "agpr_count"):
            m = re.search(r"\." + key + r":\s+(\d+)", blk)
            if m:
                meta[key] = int(m.group(1))
    assert meta, "product kernel metadata not found"
    return meta


def test_product_kernel_uses_two_term_16x16x32_mfma_only(code_object):
    isa = _kernel_isa(code_object)
    mfma = [ln.split()[0] for ln in isa if ln.split()[0].startswith("v_mfma")]
    assert mfma and set(mfma) == {"v_mfma_f32_16x16x32_bf16"}, sorted(set(mfma))
    # 8 x 4 blocks of 16 x 16 per wave, three instructions each, per 16-deep k-tile
    assert len(mfma) == 96, len(mfma)
    assert not any("32x32x16" in ln for ln in isa)


def test_product_kernel_has_no_scratch_and_two_waves_per_simd(code_object):
    meta = _kernel_meta(code_object)
    assert meta["private_segment_fixed_size"] == 0
    assert not any(ln.split()[0].startswith("scratch_") for ln in _kernel_isa(code_object))
    regs = meta["vgpr_count"] + meta.get("agpr_count", 0)
    assert regs <= 256, regs                                # 512 registers per SIMD lane: two waves
    assert meta["group_segment_fixed_size"] <= 160 * 1024    # three 48 KiB stages in one CU's LDS
