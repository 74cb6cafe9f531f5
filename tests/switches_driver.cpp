// The switch accessors of csrc/switches.hpp held to their header, without a GPU: a host-only program linked against
// switches.cpp alone (tests/test_switches_cpu.py builds and runs it).
//
//   switches_driver rules      the flag rule, the tuning gate, text() lifetime, generation(); prints "ok" or what failed
//   switches_driver table      eg_switch_table, as the library prints it
//   switches_driver threads    8 readers against 1000 rounds of setenv + reload on the main thread
//   switches_driver time       ns per on() call: 10^7 calls, one thread, median of 5 runs
//
// The threads mode under the sanitizers (stand-alone, from the repository root; not part of the suite):
//   g++ -std=c++17 -O1 -g -fsanitize=thread -Iinclude -Iexprgrad_amd/csrc tests/switches_driver.cpp exprgrad_amd/csrc/switches.cpp -o switches_tsan -lpthread && ./switches_tsan threads
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iexprgrad_amd/csrc tests/switches_driver.cpp exprgrad_amd/csrc/switches.cpp -o switches_asan -lpthread && ./switches_asan threads
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "exprgrad_hip.h"
#include "switches.hpp"

using eg::Sw;
namespace sw = eg::sw;

namespace {

int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      printf("FAILED line %d: %s\n", __LINE__, #cond);                  \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

void set(const char* name, const char* value) {
  if (value) setenv(name, value, 1);
  else unsetenv(name);
  sw::reload();
}

// unset, "", "0", "01", "1", "yes" -> off, off, off, off, on, on
void flag_rule(Sw s, const char* name) {
  const char* values[] = {nullptr, "", "0", "01", "1", "yes"};
  const bool want[] = {false, false, false, false, true, true};
  for (int i = 0; i < 6; ++i) {
    set(name, values[i]);
    if (sw::on(s) != want[i]) {
      printf("FAILED: %s=%s reads %s\n", name, values[i] ? values[i] : "(unset)", want[i] ? "off" : "on");   // (the opposite of want)
      ++failures;
    }
  }
  set(name, nullptr);
}

int rules() {
  flag_rule(Sw::NO_GRAPH, "EG_NO_GRAPH");
  flag_rule(Sw::GEMM_NO_PAIR, "EG_GEMM_NO_PAIR");   // (read by presence before the one rule)
  // a tuning row: unset without EG_TUNING=1, set with it, across reloads in both directions
  setenv("EG_EPILOGUE_MIN_ELEMS", "7", 1);
  set("EG_TUNING", nullptr);
  CHECK(!sw::is_set(Sw::EPILOGUE_MIN_ELEMS) && sw::integer(Sw::EPILOGUE_MIN_ELEMS, 3) == 3);
  set("EG_TUNING", "1");
  CHECK(sw::is_set(Sw::EPILOGUE_MIN_ELEMS) && sw::integer(Sw::EPILOGUE_MIN_ELEMS, 3) == 7);
  set("EG_TUNING", "0");
  CHECK(!sw::is_set(Sw::EPILOGUE_MIN_ELEMS) && sw::integer(Sw::EPILOGUE_MIN_ELEMS, 3) == 3);
  set("EG_TUNING", "1");
  CHECK(sw::integer(Sw::EPILOGUE_MIN_ELEMS, 3) == 7);
  setenv("EG_STREAMK_MIN_RATIO", "2.5", 1);
  sw::reload();
  CHECK(sw::real(Sw::STREAMK_MIN_RATIO, 24.0) == 2.5);
  unsetenv("EG_STREAMK_MIN_RATIO");
  unsetenv("EG_EPILOGUE_MIN_ELEMS");
  set("EG_TUNING", nullptr);
  CHECK(sw::real(Sw::STREAMK_MIN_RATIO, 24.0) == 24.0);
  // a text() pointer outlives the reload that supersedes it, with the value it had
  set("EG_DUMP_CODE", "/first");
  const char* before = sw::text(Sw::DUMP_CODE);
  CHECK(before && strcmp(before, "/first") == 0);
  set("EG_DUMP_CODE", "/second/and/longer/than/any/small/string/buffer");
  CHECK(strcmp(before, "/first") == 0);
  CHECK(strcmp(sw::text(Sw::DUMP_CODE), "/second/and/longer/than/any/small/string/buffer") == 0);
  set("EG_DUMP_CODE", nullptr);
  CHECK(sw::text(Sw::DUMP_CODE) == nullptr && strcmp(before, "/first") == 0);
  // generation() grows by exactly one per reload, through either entry
  const unsigned g0 = sw::generation();
  sw::reload();
  CHECK(sw::generation() == g0 + 1);
  CHECK(eg_switches_reload() == EG_OK && sw::generation() == g0 + 2);
  CHECK(sw::generation() == g0 + 2);
  if (!failures) printf("ok\n");
  return failures ? 1 : 0;
}

int table() {
  const int64_t n = eg_switch_table(nullptr, 0);
  std::vector<char> buf((size_t)n + 1);
  if (eg_switch_table(buf.data(), buf.size()) != n) return 1;
  fputs(buf.data(), stdout);
  return 0;
}

// Only the main thread touches the environment; every value a reader sees is one of the two that were set.
int threads() {
  const char* two[2] = {"1", "0"};
  const char* dirs[2] = {"/tmp/eg_dump_a", "/tmp/eg_dump_b_with_a_name_longer_than_a_small_string"};
  const char* nums[2] = {"100", "200"};
  auto put = [&](int k) {
    setenv("EG_NO_GRAPH", two[k], 1);
    setenv("EG_DUMP_CODE", dirs[k], 1);
    setenv("EG_DP_REAGREE_STEPS", nums[k], 1);
    sw::reload();
  };
  put(0);
  const unsigned g0 = sw::generation();
  std::atomic<bool> stop{false};
  std::atomic<long> bad{0}, reads{0};
  std::vector<std::thread> readers;
  for (int t = 0; t < 8; ++t)
    readers.emplace_back([&] {
      unsigned last = g0;
      long n = 0;
      while (!stop.load(std::memory_order_relaxed)) {
        (void)sw::on(Sw::NO_GRAPH);   // (either value is one of the two)
        const char* d = sw::text(Sw::DUMP_CODE);
        if (!d || (strcmp(d, dirs[0]) != 0 && strcmp(d, dirs[1]) != 0)) ++bad;
        const long v = sw::integer(Sw::DP_REAGREE_STEPS, -1);
        if (v != 100 && v != 200) ++bad;
        const unsigned g = sw::generation();
        if (g < last || g > g0 + 1000) ++bad;
        last = g;
        ++n;
      }
      reads += n;
    });
  for (int round = 1; round <= 1000; ++round) put(round & 1);
  stop = true;
  for (auto& r : readers) r.join();
  const bool ok = bad == 0 && sw::generation() == g0 + 1000;
  printf("%s: %ld reads by 8 threads against 1000 reloads, %ld bad\n", ok ? "ok" : "FAILED", reads.load(), bad.load());
  return ok ? 0 : 1;
}

int time_lookups() {
  setenv("EG_NO_GRAPH", "1", 1);
  sw::reload();
  const long calls = 10000000;
  double ns[5];
  long sink = 0;
  for (double& r : ns) {
    const auto t0 = std::chrono::steady_clock::now();
    for (long i = 0; i < calls; ++i) {
      sink += sw::on(Sw::NO_GRAPH);
      asm volatile("" ::: "memory");   // (each call loads the snapshot again, as separate library calls do)
    }
    r = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / calls;
  }
  std::sort(ns, ns + 5);
  printf("on(): %.2f ns per call (median of 5 runs of %ld calls; min %.2f, max %.2f; %ld on)\n", ns[2], calls, ns[0], ns[4], sink / 5);
  return sink == 5 * calls ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "rules") return rules();
  if (mode == "table") return table();
  if (mode == "threads") return threads();
  if (mode == "time") return time_lookups();
  fprintf(stderr, "usage: switches_driver rules | table | threads | time\n");
  return 2;
}
