// The k-loop schedule of split_pingpong_kernel (gemm_split_bf16.hip) as data: who meets which barrier, who issues which
// k-tile into which stage, which vmcnt is waited for where, and which stage is read in which phase.
//
// The eight waves of a block are four SIMD pairs (w, w + 4).  Waves 0-3 are role X, waves 4-7 role Y, and the two roles
// run permanently ONE BARRIER APART: a k-tile is two phases, each closed by a barrier,
//   load phase:  [Y: issue the twelve LDS-DMA pieces of k-tile kt + 2]  read the phase's head fragments of stage kt % 3
//                [Y: counted vmcnt that retires k-tile kt + 1]
//   MFMA phase:  the 96 MFMAs of k-tile kt, the other A fragments read between them; all reads retired at its end
// and Y meets one barrier more in front of the loop, X one more behind it.  Numbering the spans between barriers
// ("intervals", interval i lies behind the i-th barrier a wave has met, counted from 0):
//   X: load(kt) in interval 2 kt,      MFMA(kt) in interval 2 kt + 1
//   Y: load(kt) in interval 2 kt + 1,  MFMA(kt) in interval 2 kt + 2
// so X's MFMAs run beside Y's load phase and Y's beside X's next load phase, and nobody meets a barrier with the matrix
// pipe empty.  The hazards, in these terms (tests/split_schedule_driver.cpp replays them for small and large KT):
//   RAW  k-tile kt + 1 is retired by Y's vmcnt in interval 2 kt + 1; X first reads it in interval 2 kt + 2, Y in
//        2 kt + 3: behind the issuers' wait AND a barrier the reader has met after it.  (k-tile 0: the prologue's wait.)
//   WAR  k-tile kt + 2 goes into the stage of k-tile kt - 1, whose last reads are X's in interval 2 kt - 1 and Y's in
//        interval 2 kt (retired before the barrier that closes it); the issue is in interval 2 kt + 1.
//   vmcnt  every wait retires exactly the oldest k-tile in flight: twelve pieces per younger k-tile may still fly.
//
// constexpr, no HIP: the kernel takes its counts and stage numbers from here, and walk() is the same program as a list
// of events for the CPU check.
#pragma once

namespace eg {
namespace split_sched {

constexpr int STAGES = 3;
constexpr int WAVES = 8;
constexpr int PIECES = 12;  // LDS-DMA pieces a Y wave issues per k-tile: its own six and its SIMD partner's six
constexpr int X = 0, Y = 1;  // (ints: the kernel keeps the role in a scalar register)

constexpr int role_of(int wave) { return (wave >> 2) & 1; }
constexpr int stage_of(int kt) { return kt % STAGES; }

// In front of the loop: Y issues k-tiles 0 .. n - 1 and waits until k-tile 0 has landed; every wave meets barrier S; Y
// meets one more (the stagger).  Behind the loop X meets one more, so that every wave has met 2 + 2 KT.
constexpr int prologue_tiles(int role, int KT) { return role != Y ? 0 : KT < STAGES ? KT : STAGES; }
constexpr int prologue_vmcnt(int KT) { return (prologue_tiles(Y, KT) - 1) * PIECES; }
constexpr int barriers_before_loop(int role) { return role == Y ? 2 : 1; }
constexpr int barriers_after_loop(int role) { return role == X ? 1 : 0; }

// The load phase of k-tile kt.
constexpr bool load_issues(int role, int kt, int KT) { return role == Y && kt >= 1 && kt + 2 < KT; }
constexpr int load_issue_tile(int kt) { return kt + 2; }
constexpr bool load_waits(int role) { return role == Y; }
constexpr int load_vmcnt(int kt, int KT) { return kt + 2 < KT ? PIECES : 0; }

// The program of one wave, in order.  V has issue(kt, stage), wait(vmcnt), barrier(), read(kt, stage) and mfma(kt).  A
// phase's read() stands for the ds_reads it issues AND for the head fragments still live in it: the load phase's reads
// are consumed by the MFMA phase, whose own reads are retired (lgkmcnt(0)) in front of its closing barrier.
template <class V>
constexpr void walk(int role, int KT, V& v) {
  for (int t = 0; t < prologue_tiles(role, KT); ++t) v.issue(t, stage_of(t));
  if (prologue_tiles(role, KT)) v.wait(prologue_vmcnt(KT));
  for (int b = 0; b < barriers_before_loop(role); ++b) v.barrier();
  for (int kt = 0; kt < KT; ++kt) {
    if (load_issues(role, kt, KT)) v.issue(load_issue_tile(kt), stage_of(load_issue_tile(kt)));
    v.read(kt, stage_of(kt));
    if (load_waits(role)) v.wait(load_vmcnt(kt, KT));
    v.barrier();
    v.read(kt, stage_of(kt));
    v.mfma(kt);
    v.barrier();
  }
  for (int b = 0; b < barriers_after_loop(role); ++b) v.barrier();
}

}  // namespace split_sched
}  // namespace eg
