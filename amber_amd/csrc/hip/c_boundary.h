// c_boundary.h -- the rule of the C ABI (include/amber_hip.h, amber_hip_lab.h), host only: NO EXCEPTION CROSSES AN extern "C" FUNCTION.
// The library's messages are std::strings and its hosts grow std::vectors, so nearly every entry point can throw std::bad_alloc; thrown through
// extern "C" into a C or ctypes caller that is std::terminate.  Every entry point that can allocate or form a string therefore runs its body
// under Guarded(name, f):
//   what f returns                      -> that code (f has set the message with Fail / HIP_TRY)
//   std::bad_alloc                      -> AMBER_ENOMEM, "<name>: out of host memory"
//   std::system_error                   -> AMBER_ENOMEM, "<name>: " + what()   (create: the reference BVH's build could not start its thread)
//   any other std::exception            -> AMBER_EHIP,   "<name>: " + what()
//   anything else                       -> AMBER_EHIP,   no message
// A handler's message is a std::string too: it is formed inside a try of its own, and left empty if that throws.  No handler throws.
// Needs the error codes only -- no HIP -- so that tests/c_boundary_main.cc checks it as a stand-alone host program; HIP_TRY is a macro and
// names the HIP runtime only where it is used.  AMBER_TRY is its counterpart for the library's own int-returning calls.
#pragma once

#include <exception>
#include <new>
#include <string>
#include <system_error>

#include "../../../include/amber_hip.h"

namespace {

thread_local std::string g_last_error;

int Fail(int code, const std::string& msg) { g_last_error = msg; return code; }
#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return Fail(AMBER_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));                  \
  } while (0)
// The same for a call of the library's own that has set the message: its code, unless it is AMBER_OK, is what the caller returns
#define AMBER_TRY(expr)                                                                            \
  do {                                                                                             \
    const int rc_ = (expr);                                                                        \
    if (rc_ != AMBER_OK) return rc_;                                                               \
  } while (0)

int FailCaught(int code, const char* name, const char* what) noexcept {   // a handler's message, "<name>: <what>"
  try { g_last_error = std::string(name) + ": " + what; } catch (...) { g_last_error.clear(); }
  return code;
}
template <typename F>
int Guarded(const char* name, F&& f) noexcept {
  try { return f(); }
  catch (const std::bad_alloc&) { return FailCaught(AMBER_ENOMEM, name, "out of host memory"); }
  catch (const std::system_error& e) { return FailCaught(AMBER_ENOMEM, name, e.what()); }
  catch (const std::exception& e) { return FailCaught(AMBER_EHIP, name, e.what()); }
  catch (...) { g_last_error.clear(); return AMBER_EHIP; }
}

}  // namespace

extern "C" const char* amber_hip_last_error(void) { return g_last_error.c_str(); }
