"""Shape of split_pingpong_kernel's k loop, without a GPU (kernels/gemm_split_bf16.hip, kernels/split_schedule.hpp).

Two barriers per k-tile, with the two waves of a SIMD one barrier apart: a load phase (the loaders' LDS-DMA issue behind
a scalar branch, the fragment reads of the phase's start, the loaders' counted vmcnt), a barrier, the 96 MFMAs, a
barrier.  One wave's MFMAs run beside its partner's load phase only if ALL of them stay between the two barriers, so
this test compiles the file for gfx950 (tests/isa_tools.py), finds the loop in the disassembly (the
compiler peels the first iteration, so counts are per loop body, not per kernel) and checks exactly that."""
import pytest

from isa_tools import is_branch as _is_branch, is_dma as _is_dma, is_mfma as _is_mfma
from isa_tools import kernel_file, kernel_insts, kernel_meta, loop_to_last_back_branch

SOURCE = kernel_file("gemm_split_bf16.hip")
KERNEL = "split_pingpong_kernel"


@pytest.fixture(scope="module")
def kernel():
    """[(address, mnemonic, operands)] of the kernel, in address order."""
    return kernel_insts(SOURCE, KERNEL)


@pytest.fixture(scope="module")
def body(kernel):
    """The k loop's body: the innermost loop head with matrix instructions behind it, up to the last branch back to it
    (the roles' paths through the load phase end in a backward branch each)."""
    return loop_to_last_back_branch(kernel)


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


def test_no_scratch_two_waves_per_simd_and_three_stages_of_lds(kernel):
    meta = kernel_meta(SOURCE, KERNEL)
    assert meta["private_segment_fixed_size"] == 0
    assert not [ins for ins in kernel if ins[1].startswith("scratch_")]
    assert meta["vgpr_count"] + meta.get("agpr_count", 0) <= 256
    assert meta["group_segment_fixed_size"] <= 160 * 1024


def test_library_build_reads_no_clock(kernel):
    assert not [ins for ins in kernel if ins[1] in ("s_memtime", "s_memrealtime")]
