"""Shape of the split-bf16 product kernel's staggered k loop, without a GPU (kernels/gemm_split_bf16.hip).

The two waves of a SIMD take different roles inside ONE loop body: whatever is not an MFMA (the LDS-DMA issue, the
fragment reads of the period's start) sits behind scalar branches in front of or behind the MFMA section, so that one
wave's runs while its partner multiplies.  This test compiles the file for gfx950 as tests/test_split_gemm_isa.py does,
finds the loop in the disassembly and checks that between its first and last v_mfma there is no LDS-DMA and no s_barrier,
that the loop's LDS-DMA instructions are reached through a scalar conditional branch, and that the library build reads no
clock (the in-kernel stamps are a diagnostic build's, -DEG_SPLIT_GEMM_STAMPS)."""
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


def _tool(name):
    path = os.path.join(LLVM_BIN, name)
    return path if os.path.exists(path) else "/opt/rocm/lib/llvm/bin/" + name


@pytest.fixture(scope="module")
def kernel(tmp_path_factory):
    """[(address, mnemonic, operands)] of the product kernel, in address order."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    co = str(tmp_path_factory.mktemp("isa") / "split.co")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                    "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "--no-gpu-bundle-output", "-c",
                    os.path.join(CSRC, "kernels", "gemm_split_bf16.hip"), "-o", co], check=True, capture_output=True)
    dis = subprocess.run([_tool("llvm-objdump"), "-d", co], capture_output=True, text=True, check=True).stdout
    insts, inside = [], False
    for line in dis.splitlines():
        head = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if head:
            # (labels inside the kernel, <L0> and the like, do not end it)
            if not re.match(r"^L\d+$", head.group(1)):
                inside = KERNEL in head.group(1) and not head.group(1).endswith(".kd")
            continue
        m = re.match(r"^\s*(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if inside and m:
            insts.append((int(m.group(3), 16), m.group(1), m.group(2)))
    assert insts, "product kernel not found in the disassembly"
    return insts


def _is_dma(mn, ops):
    return mn.startswith("buffer_load") and re.search(r"\blds\b", ops) is not None


def _branch_target(addr, mn, ops):
    """Address a branch instruction jumps to (objdump prints it as a symbol, or as a signed dword count)."""
    m = re.search(r"<[^>]*\+0x([0-9a-fA-F]+)>", ops)
    if m:
        return None, int(m.group(1), 16)
    return int(ops.split()[0], 0), None


def _loop(insts):
    """The loop that holds the MFMAs: (first, last) index of the innermost backward branch's range around them."""
    base = insts[0][0]
    mfma = [i for i, (_, mn, _) in enumerate(insts) if mn.startswith("v_mfma")]
    assert mfma
    best = None
    for i, (addr, mn, ops) in enumerate(insts):
        if not (mn == "s_branch" or mn.startswith("s_cbranch")):
            continue
        count, off = _branch_target(addr, mn, ops)
        target = base + off if off is not None else addr + 4 + 4 * (count - (1 << 16) if count >= (1 << 15) else count)
        if target <= insts[mfma[0]][0] and addr >= insts[mfma[-1]][0]:
            start = next(j for j, ins in enumerate(insts) if ins[0] >= target)
            if best is None or i - start < best[1] - best[0]:
                best = (start, i)
    assert best, "no backward branch around the MFMAs"
    return best


def test_nothing_but_lds_reads_between_the_loops_mfmas(kernel):
    lo, hi = _loop(kernel)
    body = kernel[lo:hi + 1]
    mfma = [i for i, (_, mn, _) in enumerate(body) if mn.startswith("v_mfma")]
    assert len(mfma) == 96
    section = body[mfma[0]:mfma[-1] + 1]
    assert not [ins for ins in section if _is_dma(ins[1], ins[2])]
    assert not [ins for ins in section if ins[1] == "s_barrier"]
    assert not [ins for ins in section if ins[1].startswith("s_cbranch") or ins[1] == "s_branch"]
    assert sum(1 for ins in body if ins[1] == "s_barrier") == 1          # one barrier per k-tile


def test_the_loops_lds_dma_sits_behind_a_scalar_branch(kernel):
    lo, hi = _loop(kernel)
    body = kernel[lo:hi + 1]
    dma = [i for i, ins in enumerate(body) if _is_dma(ins[1], ins[2])]
    assert len(dma) == 12, len(dma)          # a loader's own six pieces and its partner's
    barrier = next(i for i, ins in enumerate(body) if ins[1] == "s_barrier")
    first_mfma = next(i for i, ins in enumerate(body) if ins[1].startswith("v_mfma"))
    assert barrier < dma[0] and dma[-1] < first_mfma
    # a conditional branch on SCC (a scalar compare, not a lane mask) between the barrier and the first piece
    assert any(ins[1] in ("s_cbranch_scc0", "s_cbranch_scc1") for ins in body[barrier:dma[0]])
    # and no lane masking in the loop: the roles are wave-uniform
    assert not [ins for ins in body if ins[1].startswith("s_cbranch_exec") or "saveexec" in ins[1]]
    # the fragment reads of the period's start (late waves) and of the next k-tile (early waves) are branched around too
    reads_front = sum(1 for ins in body[barrier:first_mfma] if ins[1] == "ds_read_b128")
    last_mfma = max(i for i, ins in enumerate(body) if ins[1].startswith("v_mfma"))
    reads_back = sum(1 for ins in body[last_mfma:] if ins[1] == "ds_read_b128")
    assert reads_front >= 14 and reads_back == 14, (reads_front, reads_back)
    assert any(ins[1].startswith("s_cbranch") for ins in body[last_mfma:last_mfma + 4])


def test_library_build_reads_no_clock(kernel):
    assert not [ins for ins in kernel if ins[1] in ("s_memtime", "s_memrealtime")]
