// Replays the k-loop schedule of split_pingpong_kernel (exprgrad_amd/csrc/kernels/split_schedule.hpp) for the eight waves
// of a block, barrier generation by barrier generation, and checks the hazards the kernel relies on.  No HIP.
//
// A wave's program is the header's walk() as a list of events; an event's interval is the number of barriers the wave
// has met in front of it.  All waves meet every barrier together, so events of two waves are ordered exactly when
// their intervals differ.  Usage: split_schedule_driver KT...   prints "PASS KT=..." per KT and "ALL PASS".
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <string>
#include <vector>

#include "../exprgrad_amd/csrc/kernels/split_schedule.hpp"

namespace ss = eg::split_sched;

enum Kind { ISSUE, WAIT, BARRIER, READ, MFMA };
struct Event {
  Kind kind;
  int kt, stage, n;  // ISSUE / READ: k-tile and stage; WAIT: vmcnt; MFMA: k-tile
  int interval;
};
using Program = std::vector<Event>;

struct Recorder {
  Program p;
  int gen = 0;
  void issue(int kt, int stage) { p.push_back({ISSUE, kt, stage, 0, gen}); }
  void wait(int n) { p.push_back({WAIT, 0, 0, n, gen}); }
  void barrier() { p.push_back({BARRIER, 0, 0, 0, gen++}); }
  void read(int kt, int stage) { p.push_back({READ, kt, stage, 0, gen}); }
  void mfma(int kt) { p.push_back({MFMA, kt, 0, 0, gen}); }
};

static void renumber(Program& p) {
  int gen = 0;
  for (Event& e : p) {
    e.interval = gen;
    if (e.kind == BARRIER) ++gen;
  }
}

// "" when the eight programs are a correct schedule for KT k-tiles, else what is wrong.
static std::string check(const std::vector<Program>& w, int KT) {
  char buf[256];
  auto fail = [&](const char* what, int wave, int kt) {
    snprintf(buf, sizeof buf, "%s (wave %d, k-tile %d)", what, wave, kt);
    return std::string(buf);
  };
  // every wave meets the same number of barriers
  std::vector<int> barriers(ss::WAVES, 0);
  for (int i = 0; i < ss::WAVES; ++i)
    for (const Event& e : w[i]) barriers[i] += e.kind == BARRIER;
  for (int i = 1; i < ss::WAVES; ++i)
    if (barriers[i] != barriers[0]) return fail("barrier counts differ", i, -1);
  if (barriers[0] != 2 + 2 * KT) return fail("not 2 + 2 KT barriers", 0, -1);

  // per issuer: where each k-tile is issued and which wait retires it (vmcnt(N): all but the N youngest pieces have landed)
  std::vector<std::vector<int>> issued(ss::WAVES, std::vector<int>(KT, -1)), retired(ss::WAVES, std::vector<int>(KT, -1));
  std::vector<int> issuers;
  for (int i = 0; i < ss::WAVES; ++i) {
    std::deque<int> flying;  // k-tiles in flight, oldest first, PIECES each
    for (const Event& e : w[i]) {
      if (e.kind == ISSUE) {
        if (e.kt < 0 || e.kt >= KT || issued[i][e.kt] >= 0) return fail("k-tile issued twice or out of range", i, e.kt);
        if (e.stage != e.kt % ss::STAGES) return fail("issue into the wrong stage", i, e.kt);
        if (!flying.empty() && flying.back() + 1 != e.kt) return fail("issues out of order", i, e.kt);
        issued[i][e.kt] = e.interval;
        flying.push_back(e.kt);
      } else if (e.kind == WAIT) {
        // the count is exact: it retires the oldest k-tile in flight and nothing younger
        const int want = flying.empty() ? 0 : ((int)flying.size() - 1) * ss::PIECES;
        if (e.n != want) return fail("vmcnt is not the pieces that may still fly", i, flying.empty() ? -1 : flying.front());
        while ((int)flying.size() * ss::PIECES > e.n) {
          retired[i][flying.front()] = e.interval;
          flying.pop_front();
        }
      }
    }
    if (!flying.empty()) return fail("pieces in flight at the end", i, flying.front());
    if (issued[i][0] >= 0) issuers.push_back(i);
  }
  // the issuers are one wave of every SIMD pair (they load their partner's share), and each issues every k-tile
  if (issuers.size() != ss::WAVES / 2) return fail("not four issuers", -1, -1);
  for (int i : issuers) {
    if (ss::role_of(i) != ss::Y) return fail("an X wave issues", i, -1);
    for (int kt = 0; kt < KT; ++kt)
      if (issued[i][kt] < 0 || retired[i][kt] < 0) return fail("k-tile never issued or never waited for", i, kt);
  }

  // reads: ascending, once per phase and k-tile, from the right stage, behind the issuers' wait and a barrier
  std::vector<std::vector<int>> last_read(ss::WAVES, std::vector<int>(KT, -1));
  for (int i = 0; i < ss::WAVES; ++i) {
    int next_head = 0, next_rows = 0, next_mfma = 0;
    for (size_t k = 0; k < w[i].size(); ++k) {
      const Event& e = w[i][k];
      if (e.kind == MFMA) {
        if (e.kt != next_mfma++) return fail("MFMAs out of k order", i, e.kt);
        continue;
      }
      if (e.kind != READ) continue;
      if (e.kt < 0 || e.kt >= KT) return fail("read of a k-tile that does not exist", i, e.kt);
      if (e.stage != e.kt % ss::STAGES) return fail("read of the wrong stage", i, e.kt);
      int& next = last_read[i][e.kt] < 0 ? next_head : next_rows;
      if (e.kt != next++) return fail("reads out of order", i, e.kt);
      for (int y : issuers)
        if (!(retired[y][e.kt] < e.interval)) return fail("read not a barrier behind the wait that retires it", i, e.kt);
      last_read[i][e.kt] = e.interval;
    }
    if (next_head != KT || next_rows != KT || next_mfma != KT) return fail("a k-tile is not read once per phase", i, -1);
  }
  // no issue into a stage before a barrier that every reader met behind its last read of the k-tile it holds
  for (int y : issuers)
    for (int kt = ss::STAGES; kt < KT; ++kt)
      for (int i = 0; i < ss::WAVES; ++i)
        if (!(last_read[i][kt - ss::STAGES] < issued[y][kt])) return fail("issue over a stage still being read", i, kt);
  // SIMD partners never multiply in the same interval
  for (int i = 0; i < ss::WAVES / 2; ++i)
    for (const Event& a : w[i])
      if (a.kind == MFMA)
        for (const Event& b : w[i + 4])
          if (b.kind == MFMA && b.interval == a.interval) return fail("partners multiply in the same interval", i, a.kt);
  return "";
}

static std::vector<Program> programs(int KT) {
  std::vector<Program> w(ss::WAVES);
  for (int i = 0; i < ss::WAVES; ++i) {
    Recorder r;
    ss::walk(ss::role_of(i), KT, r);
    w[i] = r.p;
  }
  return w;
}

// The checker must be able to fail: three broken variants of the schedule have to be caught.
static bool mutants_are_caught(int KT) {
  bool ok = true;
  {  // a Y wave without its stagger barrier
    auto w = programs(KT);
    for (size_t k = 0; k < w[5].size(); ++k)
      if (w[5][k].kind == BARRIER) {
        w[5].erase(w[5].begin() + k);
        break;
      }
    renumber(w[5]);
    ok &= !check(w, KT).empty();
  }
  if (KT > ss::STAGES) {  // k-tile 3 issued one phase early, into a stage the partner still multiplies from
    auto w = programs(KT);
    for (int i = 4; i < ss::WAVES; ++i)
      for (size_t k = 0; k < w[i].size(); ++k)
        if (w[i][k].kind == ISSUE && w[i][k].kt == ss::STAGES) {
          Event e = w[i][k];
          w[i].erase(w[i].begin() + k);
          size_t b = k;
          while (w[i][b - 1].kind != BARRIER) --b;
          w[i].insert(w[i].begin() + (b - 1), e);
          renumber(w[i]);
          break;
        }
    ok &= !check(w, KT).empty();
  }
  if (KT > 1) {  // the loop's first wait one k-tile too loose: k-tile 1 is read while it may still fly
    auto w = programs(KT);
    for (int i = 4; i < ss::WAVES; ++i) {
      int seen = 0;
      for (Event& e : w[i])
        if (e.kind == WAIT && seen++ == 1) e.n += ss::PIECES;
    }
    ok &= !check(w, KT).empty();
  }
  return ok;
}

int main(int argc, char** argv) {
  bool all = true;
  for (int a = 1; a < argc; ++a) {
    const int KT = atoi(argv[a]);
    const std::string why = check(programs(KT), KT);
    const bool caught = mutants_are_caught(KT);
    if (why.empty() && caught) {
      printf("PASS KT=%d barriers=%d\n", KT, 2 + 2 * KT);
    } else {
      printf("FAIL KT=%d %s\n", KT, why.empty() ? "a broken schedule was not caught" : why.c_str());
      all = false;
    }
  }
  puts(all && argc > 1 ? "ALL PASS" : "FAILED");
  return all && argc > 1 ? 0 : 1;
}
