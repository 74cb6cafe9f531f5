// The thread-local error text behind eg_last_error().  No HIP header: the kernel-description layer (host/kd.cpp,
// codegen.cpp, match.cpp, epilogue.cpp, the row-fusion units) reports through here and compiles with a plain C++ compiler.
#pragma once

namespace eg {

void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
void clear_error();

}  // namespace eg
