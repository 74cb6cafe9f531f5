#include "error.hpp"

#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "exprgrad_hip.h"

namespace eg {
static thread_local std::string g_error;

void set_error(const char* fmt, ...) {
  char stack[2048];
  va_list ap;
  va_start(ap, fmt);
  int n = vsnprintf(stack, sizeof(stack), fmt, ap);
  va_end(ap);
  if (n < (int)sizeof(stack)) {
    g_error.assign(stack, n < 0 ? 0 : n);
    return;
  }
  std::vector<char> heap(n + 1);
  va_start(ap, fmt);
  vsnprintf(heap.data(), heap.size(), fmt, ap);
  va_end(ap);
  g_error.assign(heap.data(), n);
}
void clear_error() { g_error.clear(); }
}  // namespace eg

extern "C" const char* eg_last_error(void) { return eg::g_error.c_str(); }
