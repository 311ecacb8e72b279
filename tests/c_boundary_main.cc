// Stand-alone host check of amber_amd/csrc/hip/c_boundary.h (tests/test_c_boundary.py builds and runs it; no HIP, no library).
// Guarded(name, f) over callables that return a code, throw std::bad_alloc, std::system_error, another std::exception and an int: the code
// and the text of amber_hip_last_error() for each.  Then std::bad_alloc once more while the global operator new fails, so that the handler's
// own message cannot be formed: the handler neither throws nor terminates, the code stands and the message is empty.
// Prints the number of cases and of failures; exit status 0 only if there is none.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "c_boundary.h"

namespace {
bool g_new_fails = false;
void* Allocate(std::size_t n) {
  if (g_new_fails) throw std::bad_alloc();
  if (void* p = std::malloc(n ? n : 1)) return p;
  throw std::bad_alloc();
}
}  // namespace
void* operator new(std::size_t n) { return Allocate(n); }
void* operator new[](std::size_t n) { return Allocate(n); }
void operator delete(void* p) noexcept { std::free(p); }
void operator delete[](void* p) noexcept { std::free(p); }
void operator delete(void* p, std::size_t) noexcept { std::free(p); }
void operator delete[](void* p, std::size_t) noexcept { std::free(p); }

namespace {
int g_cases = 0, g_failures = 0;
void Expect(const char* what, int code, int want_code, const char* want_message) {
  ++g_cases;
  if (code == want_code && std::strcmp(amber_hip_last_error(), want_message) == 0) return;
  ++g_failures;
  std::printf("FAILED %s: code %d (want %d), message \"%s\" (want \"%s\")\n", what, code, want_code, amber_hip_last_error(), want_message);
}
}  // namespace

int main() {
  const char* name = "amber_hip_pt_some_entry_point";                // longer than a std::string keeps without an allocation
  Expect("ok", Guarded(name, []() -> int { return AMBER_OK; }), AMBER_OK, "");
  Expect("a code", Guarded(name, []() -> int { return Fail(AMBER_EINVAL, "null handle"); }), AMBER_EINVAL, "null handle");
  Expect("bad_alloc", Guarded(name, []() -> int { throw std::bad_alloc(); }), AMBER_ENOMEM, "amber_hip_pt_some_entry_point: out of host memory");
  const std::system_error no_thread(std::make_error_code(std::errc::resource_unavailable_try_again), "std::async");
  const std::string want_system = std::string(name) + ": " + no_thread.what();
  Expect("system_error", Guarded(name, [&]() -> int { throw no_thread; }), AMBER_ENOMEM, want_system.c_str());
  Expect("runtime_error", Guarded(name, []() -> int { throw std::runtime_error("vector::_M_range_check"); }), AMBER_EHIP,
         "amber_hip_pt_some_entry_point: vector::_M_range_check");
  Fail(AMBER_EINVAL, "a message from an earlier call");
  Expect("int", Guarded(name, []() -> int { throw 42; }), AMBER_EHIP, "");
  // out of memory for good: the handler's message needs an allocation (the error string owns none), and operator new fails while it runs
  std::string().swap(g_last_error);
  const int code = Guarded(name, []() -> int { g_new_fails = true; throw std::bad_alloc(); });
  g_new_fails = false;
  Expect("bad_alloc, then no memory for the message", code, AMBER_ENOMEM, "");
  std::printf("cases %d, failures %d\n", g_cases, g_failures);
  return g_failures == 0 ? 0 : 1;
}
