// The environment switches the library honours: loading the list of switches.hpp into snapshots, and its C ABI.
#include "switches.hpp"

#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>

#include "exprgrad_hip.h"

namespace {

struct Row {
  const char* name;
  const char* cls;
  const char* purpose;
};
#define EG_SW_ROW(id, name, cls, kind, purpose) {name, cls, purpose},
const Row kSwitches[] = {EG_SWITCHES(EG_SW_ROW)};
#undef EG_SW_ROW
constexpr int kCount = (int)eg::Sw::kCount;

// A snapshot with the strings its pointers point into.
struct Loaded : eg::sw::Snapshot {
  std::string storage[kCount];
  const Loaded* older;  // the retired snapshots: never freed, readers may still hold pointers into them
};
std::mutex g_mu;  // the first load and reload() only

const eg::sw::Snapshot* load_locked() {
  const Loaded* older = static_cast<const Loaded*>(eg::sw::g_snapshot.load(std::memory_order_relaxed));
  Loaded* s = new Loaded;
  const char* t = getenv("EG_TUNING");
  const bool tuning = t && t[0] && t[0] != '0';
  for (int i = 0; i < kCount; ++i) {
    const char* e = getenv(kSwitches[i].name);
    if (e && !tuning && strcmp(kSwitches[i].cls, "tuning") == 0) e = nullptr;
    if (e) s->storage[i] = e;
    s->value[i] = e ? s->storage[i].c_str() : nullptr;
  }
  s->generation = older ? older->generation + 1 : 1;
  s->older = older;
  eg::sw::g_snapshot.store(s, std::memory_order_release);
  return s;
}

}  // namespace

namespace eg {
namespace sw {

std::atomic<const Snapshot*> g_snapshot{nullptr};

const Snapshot* first_load() {
  std::lock_guard<std::mutex> lock(g_mu);
  const Snapshot* s = g_snapshot.load(std::memory_order_acquire);
  return s ? s : load_locked();
}

void reload() {
  std::lock_guard<std::mutex> lock(g_mu);
  load_locked();
}

}  // namespace sw
}  // namespace eg

extern "C" {

int eg_switches_reload(void) {
  eg::sw::reload();
  return EG_OK;
}

// "<name>\t<class>\t<purpose>\n" per switch; returns the length needed (without the terminator), copies at most cap - 1.
int64_t eg_switch_table(char* buf, size_t cap) {
  std::string s;
  for (int i = 0; i < kCount; ++i) s += std::string(kSwitches[i].name) + "\t" + kSwitches[i].cls + "\t" + kSwitches[i].purpose + "\n";
  if (buf && cap > 0) {
    const size_t n = s.size() < cap - 1 ? s.size() : cap - 1;
    memcpy(buf, s.data(), n);
    buf[n] = 0;
  }
  return (int64_t)s.size();
}

}  // extern "C"
