"""Shape of split_pingpong_kernel's k loop, without a GPU (kernels/gemm_split_bf16.hip, kernels/split_schedule.hpp).

Two barriers per k-tile, with the two waves of a SIMD one barrier apart: a load phase (the loaders' LDS-DMA issue behind
a scalar branch, the fragment reads of the phase's start, the loaders' counted vmcnt), a barrier, the 96 MFMAs, a
barrier.  One wave's MFMAs run beside its partner's load phase only if ALL of them stay between the two barriers, so
this test compiles the file for gfx950 as tests/test_split_gemm_isa.py does, finds the loop in the disassembly (the
compiler peels the first iteration, so counts are per loop body, not per kernel) and checks exactly that."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exprgrad_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LLVM_BIN = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "lib", "llvm", "bin")
KERNEL = "split_pingpong_kernel"


def _tool(name):
    path = os.path.join(LLVM_BIN, name)
    return path if os.path.exists(path) else "/opt/rocm/lib/llvm/bin/" + name


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    co = str(tmp_path_factory.mktemp("isa") / "split.co")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                    "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "--no-gpu-bundle-output", "-c",
                    os.path.join(CSRC, "kernels", "gemm_split_bf16.hip"), "-o", co], check=True, capture_output=True)
    return co


@pytest.fixture(scope="module")
def kernel(code_object):
    """[(address, mnemonic, operands)] of the kernel, in address order."""
    dis = subprocess.run([_tool("llvm-objdump"), "-d", code_object], capture_output=True, text=True, check=True).stdout
    insts, inside = [], False
    for line in dis.splitlines():
        head = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if head:
            if not re.match(r"^L\d+$", head.group(1)):     # (labels inside the kernel do not end it)
                inside = KERNEL in head.group(1) and not head.group(1).endswith(".kd")
            continue
        m = re.match(r"^\s*(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if inside and m:
            insts.append((int(m.group(3), 16), m.group(1), m.group(2)))
    assert insts, "kernel not found in the disassembly"
    return insts


def _is_dma(ins):
    return ins[1].startswith("buffer_load") and re.search(r"\blds\b", ins[2]) is not None


def _is_branch(ins):
    return ins[1] == "s_branch" or ins[1].startswith("s_cbranch")


def _is_mfma(ins):
    return ins[1].startswith("v_mfma")


def _target(insts, ins):
    """Address a branch jumps to (objdump prints it as a symbol plus offset, or as a signed dword count)."""
    addr, _, ops = ins
    m = re.search(r"<[^>]*\+0x([0-9a-fA-F]+)>", ops)
    if m:
        return insts[0][0] + int(m.group(1), 16)
    count = int(ops.split()[0], 0)
    return addr + 4 + 4 * (count - (1 << 16) if count >= (1 << 15) else count)


@pytest.fixture(scope="module")
def body(kernel):
    """The k loop's body: the innermost loop head with matrix instructions behind it, up to the last branch back to it
    (the roles' paths through the load phase end in a backward branch each)."""
    back = []          # (head index, branch index) of every backward branch around matrix instructions
    for i, ins in enumerate(kernel):
        if not _is_branch(ins):
            continue
        target = _target(kernel, ins)
        if target > ins[0]:
            continue
        start = next(j for j, other in enumerate(kernel) if other[0] >= target)
        if any(_is_mfma(x) for x in kernel[start:i + 1]):
            back.append((start, i))
    assert back, "no loop around the MFMAs"
    head = min(back, key=lambda b: b[1] - b[0])[0]
    return kernel[head:max(i for start, i in back if start == head) + 1]


def test_every_matrix_instruction_is_the_two_term_form(kernel):
    assert {ins[1] for ins in kernel if _is_mfma(ins)} == {"v_mfma_f32_16x16x32_bf16"}


def test_the_96_mfmas_stand_alone_between_the_two_barriers(body):
    mfma = [i for i, ins in enumerate(body) if _is_mfma(ins)]
    assert len(mfma) == 96, len(mfma)
    section = body[mfma[0]:mfma[-1] + 1]
    assert not [ins for ins in section if ins[1] == "s_barrier"]
    assert not [ins for ins in section if _is_dma(ins)]
    assert not [ins for ins in section if _is_branch(ins)]
    barriers = [i for i, ins in enumerate(body) if ins[1] == "s_barrier"]
    assert len(barriers) == 2, len(barriers)
    assert barriers[0] < mfma[0] and mfma[-1] < barriers[1]      # one in front of the run, one behind it
    # the multiplying wave runs at raised priority, from the opening barrier to the closing one and nowhere else
    prio = [(i, ins[2].strip()) for i, ins in enumerate(body) if ins[1] == "s_setprio"]
    assert [p for _, p in prio] == ["1", "0"], prio
    assert barriers[0] < prio[0][0] < mfma[0] and mfma[-1] < prio[1][0] < barriers[1]


def test_the_lds_dma_sits_behind_a_scalar_branch_in_front_of_the_first_barrier(body):
    # the compiler may rotate the loop (in memory: MFMA phase, then the next k-tile's load phase, then the branch back):
    # read the body as a cycle that starts behind the barrier that closes the MFMA run
    last_mfma = max(i for i, ins in enumerate(body) if _is_mfma(ins))
    closing = next(i for i, ins in enumerate(body) if i > last_mfma and ins[1] == "s_barrier")
    body = body[closing + 1:] + body[:closing + 1]
    dma = [i for i, ins in enumerate(body) if _is_dma(ins)]
    assert len(dma) == 12, len(dma)                              # a loader's own six pieces and its partner's
    first_barrier = next(i for i, ins in enumerate(body) if ins[1] == "s_barrier")
    assert dma[-1] < first_barrier
    # the branch that guards the pieces (the last one in front of them) is on SCC: a scalar compare, not a lane mask
    guard = [ins for ins in body[:dma[0]] if _is_branch(ins)][-1]
    assert guard[1] in ("s_cbranch_scc0", "s_cbranch_scc1"), guard
    assert not [ins for ins in body[dma[0]:dma[-1]] if _is_branch(ins)]
    # the roles are wave-uniform: no lane masking anywhere in the loop
    assert not [ins for ins in body if ins[1].startswith("s_cbranch_exec") or "saveexec" in ins[1]]
    # the loaders' counted wait stands between the pieces and the first barrier, and nothing drains them earlier
    waits = [ins[2] for ins in body[dma[0]:first_barrier] if ins[1] == "s_waitcnt" and "vmcnt" in ins[2]]
    assert sorted(set(waits)) == ["vmcnt(0)", "vmcnt(12)"], waits
    assert not [ins for ins in body[first_barrier:] if ins[1] == "s_waitcnt" and "vmcnt" in ins[2]]


def test_no_scratch_two_waves_per_simd_and_three_stages_of_lds(code_object, kernel):
    notes = subprocess.run([_tool("llvm-readelf"), "--notes", code_object], capture_output=True, text=True, check=True).stdout
    meta = {}
    for blk in re.split(r"\n  - (?=\.)", notes):                 # one YAML map per kernel
        name = re.search(r"^ {4}\.name:\s+(\S+)", blk, re.M)
        if not name or KERNEL not in name.group(1):
            continue
        for key in ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count", "agpr_count"):
            m = re.search(r"\." + key + r":\s+(\d+)", blk)
            if m:
                meta[key] = int(m.group(1))
    assert meta, "kernel metadata not found"
    assert meta["private_segment_fixed_size"] == 0
    assert not [ins for ins in kernel if ins[1].startswith("scratch_")]
    assert meta["vgpr_count"] + meta.get("agpr_count", 0) <= 256
    assert meta["group_segment_fixed_size"] <= 160 * 1024


def test_library_build_reads_no_clock(kernel):
    assert not [ins for ins in kernel if ins[1] in ("s_memtime", "s_memrealtime")]
