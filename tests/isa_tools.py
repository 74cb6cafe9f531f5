"""What the CPU-only ISA tests share: compile one kernel file for gfx950 (device code only, the library's flags),
disassemble it, and find a kernel, its metadata and its k loop in the text.  A file is compiled once per process."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exprgrad_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LLVM_BIN = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "lib", "llvm", "bin")


def _tool(name):
    path = os.path.join(LLVM_BIN, name)
    return path if os.path.exists(path) else "/opt/rocm/lib/llvm/bin/" + name


@functools.lru_cache(maxsize=None)
def _compiled(path):
    """(disassembly, notes) of the file's gfx950 code object."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, "kernels.co")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "--no-gpu-bundle-output", "-c",
                        path, "-o", co], check=True, capture_output=True)
        dis = subprocess.run([_tool("llvm-objdump"), "-d", co], capture_output=True, text=True, check=True).stdout
        notes = subprocess.run([_tool("llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    return dis, notes


def kernel_file(name):
    return os.path.join(CSRC, "kernels", name)


def kernel_insts(path, kernel):
    """[(address, mnemonic, operands)] of the kernel, in address order."""
    insts, inside = [], False
    for line in _compiled(path)[0].splitlines():
        head = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if head:
            if not re.match(r"^L\d+$", head.group(1)):     # (labels inside the kernel, <L0> and the like, do not end it)
                inside = kernel in head.group(1) and not head.group(1).endswith(".kd")
            continue
        m = re.match(r"^\s*(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if inside and m:
            insts.append((int(m.group(3), 16), m.group(1), m.group(2)))
    assert insts, kernel + " not found in the disassembly"
    return insts


def kernel_meta(path, kernel):
    """The kernel's segment sizes and register counts from the code object's notes."""
    meta = {}
    for blk in re.split(r"\n  - (?=\.)", _compiled(path)[1]):    # one YAML map per kernel
        name = re.search(r"^ {4}\.name:\s+(\S+)", blk, re.M)      # the kernel's own, not an argument's
        if not name or kernel not in name.group(1):
            continue
        for key in ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count", "agpr_count"):
            m = re.search(r"\." + key + r":\s+(\d+)", blk)
            if m:
                meta[key] = int(m.group(1))
    assert meta, kernel + " metadata not found"
    return meta


def is_dma(ins):
    return ins[1].startswith("buffer_load") and re.search(r"\blds\b", ins[2]) is not None


def is_branch(ins):
    return ins[1] == "s_branch" or ins[1].startswith("s_cbranch")


def is_mfma(ins):
    return ins[1].startswith("v_mfma")


def branch_target(insts, ins):
    """Address a branch jumps to (objdump prints it as a symbol plus offset, or as a signed dword count)."""
    addr, _, ops = ins
    m = re.search(r"<[^>]*\+0x([0-9a-fA-F]+)>", ops)
    if m:
        return insts[0][0] + int(m.group(1), 16)
    count = int(ops.split()[0], 0)
    return addr + 4 + 4 * (count - (1 << 16) if count >= (1 << 15) else count)


def innermost_loop(insts):
    """The loop that holds the MFMAs: (first, last) index of the innermost backward branch's range around them."""
    mfma = [i for i, ins in enumerate(insts) if is_mfma(ins)]
    assert mfma
    best = None
    for i, ins in enumerate(insts):
        if not is_branch(ins):
            continue
        target = branch_target(insts, ins)
        if target <= insts[mfma[0]][0] and ins[0] >= insts[mfma[-1]][0]:
            start = next(j for j, other in enumerate(insts) if other[0] >= target)
            if best is None or i - start < best[1] - best[0]:
                best = (start, i)
    assert best, "no backward branch around the MFMAs"
    return best


def loop_to_last_back_branch(insts):
    """The innermost loop head with matrix instructions behind it, up to the LAST branch back to it (a loop whose paths
    end in a backward branch each)."""
    back = []          # (head index, branch index) of every backward branch around matrix instructions
    for i, ins in enumerate(insts):
        if not is_branch(ins):
            continue
        target = branch_target(insts, ins)
        if target > ins[0]:
            continue
        start = next(j for j, other in enumerate(insts) if other[0] >= target)
        if any(is_mfma(x) for x in insts[start:i + 1]):
            back.append((start, i))
    assert back, "no loop around the MFMAs"
    head = min(back, key=lambda b: b[1] - b[0])[0]
    return insts[head:max(i for start, i in back if start == head) + 1]
