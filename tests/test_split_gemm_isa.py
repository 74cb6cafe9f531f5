"""Instruction-level check of split_gemm_kernel, the split-bf16 product's in-phase k loop, without a GPU
(kernels/gemm_split_bf16.hip).

The product kernel puts two bf16 terms into every v_mfma_f32_16x16x32_bf16 (lane groups 0-1 and 2-3 read different
planes).  This test compiles the file for gfx950 (device code only, tests/isa_tools.py), disassembles it and checks that
the product kernel's matrix instructions are all of that form (96 per 16-deep k-tile), that no 32x32 form is left, and
that it runs at two waves per SIMD with no scratch and its three LDS stages within the CU's 160 KiB.

The loop: one barrier per k-tile, every wave in phase.  Whatever is not an MFMA (the wave's six LDS-DMA pieces of k-tile
kt + 2 behind a scalar branch, the fragment reads of the period's start) stands between the barrier and the first MFMA;
between the first and the last v_mfma there is no LDS-DMA, no s_barrier and no branch, and the library build reads no
clock."""
import pytest

from isa_tools import innermost_loop, is_dma, kernel_file, kernel_insts, kernel_meta

SOURCE = kernel_file("gemm_split_bf16.hip")
KERNEL = "split_gemm_kernel"


@pytest.fixture(scope="module")
def kernel():
    """[(address, mnemonic, operands)] of the product kernel, in address order."""
    return kernel_insts(SOURCE, KERNEL)


@pytest.fixture(scope="module")
def isa(kernel):
    return ["%s %s" % (mn, ops) for _, mn, ops in kernel]


def _is_dma(mn, ops):
    return is_dma((None, mn, ops))


_loop = innermost_loop


def test_product_kernel_uses_two_term_16x16x32_mfma_only(isa):
    mfma = [ln.split()[0] for ln in isa if ln.split()[0].startswith("v_mfma")]
    assert mfma and set(mfma) == {"v_mfma_f32_16x16x32_bf16"}, sorted(set(mfma))
    # 8 x 4 blocks of 16 x 16 per wave, three instructions each, per 16-deep k-tile
    assert len(mfma) == 96, len(mfma)
    assert not any("32x32x16" in ln for ln in isa)


def test_product_kernel_has_no_scratch_and_two_waves_per_simd(isa):
    meta = kernel_meta(SOURCE, KERNEL)
    assert meta["private_segment_fixed_size"] == 0
    assert not any(ln.split()[0].startswith("scratch_") for ln in isa)
    regs = meta["vgpr_count"] + meta.get("agpr_count", 0)
    assert regs <= 256, regs                                # 512 registers per SIMD lane: two waves
    assert meta["group_segment_fixed_size"] <= 160 * 1024    # three 48 KiB stages in one CU's LDS


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
    assert len(dma) == 6, len(dma)           # the wave's own six pieces of k-tile kt + 2
    barrier = next(i for i, ins in enumerate(body) if ins[1] == "s_barrier")
    first_mfma = next(i for i, ins in enumerate(body) if ins[1].startswith("v_mfma"))
    assert barrier < dma[0] and dma[-1] < first_mfma
    # a conditional branch on SCC (a scalar compare, not a lane mask) between the barrier and the first piece
    assert any(ins[1] in ("s_cbranch_scc0", "s_cbranch_scc1") for ins in body[barrier:dma[0]])
    # and no lane masking in the loop: the issue is wave-uniform
    assert not [ins for ins in body if ins[1].startswith("s_cbranch_exec") or "saveexec" in ins[1]]
    # the fragment reads of the period's start stand in front of the MFMAs, and none behind the last one
    reads_front = sum(1 for ins in body[barrier:first_mfma] if ins[1] == "ds_read_b128")
    last_mfma = max(i for i, ins in enumerate(body) if ins[1].startswith("v_mfma"))
    reads_back = sum(1 for ins in body[last_mfma:] if ins[1] == "ds_read_b128")
    assert reads_front >= 14 and reads_back == 0, (reads_front, reads_back)
    # the only counted wait of the body: this wave's pieces of k-tile kt, in front of the barrier (the next six may fly)
    waits = [(i, ins[2]) for i, ins in enumerate(body) if ins[1] == "s_waitcnt" and "vmcnt" in ins[2]]
    assert [w for _, w in waits] == ["vmcnt(6)"], waits
    assert waits[0][0] < barrier


def test_library_build_reads_no_clock(kernel):
    assert not [ins for ins in kernel if ins[1] in ("s_memtime", "s_memrealtime")]
