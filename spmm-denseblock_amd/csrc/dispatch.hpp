// dispatch.hpp — host-side helpers of the kernel launchers (csr_kernels.hip,
// bsr_kernels.hip): run-time values to template arguments, TUNING-build overrides, and the
// timing pair around a launcher's body. Which instantiation an argument tuple reaches is
// pinned by tests/test_dispatch_trace.py (csrc/dispatch_trace.hpp).
#pragma once

#include <cstdlib>
#include <type_traits>
#include <utility>

#include "context.hpp"

namespace spmm {

// f(std::true_type / std::false_type ...) for the given bools: `c()` is a constant in f.
template <typename F>
void with_bools(F&& f) { f(); }
template <typename F, typename... B>
void with_bools(F&& f, bool b, B... rest) {
  if (b) with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

// f(std::integral_constant<int, Vi>{}) for the Vi equal to v; false if there is none.
template <int... V, typename F>
bool with_int(int v, F&& f) {
  return ((v == V ? (f(std::integral_constant<int, V>{}), true) : false) || ...);
}

// A TUNING build (make TUNING=1)? `if constexpr (kTuning)` keeps the kernels only an
// override can reach out of a release library.
#ifdef SPMM_TUNING
constexpr bool kTuning = true;
#else
constexpr bool kTuning = false;
#endif

// An integer a TUNING build reads from the environment, once per use site.
// A release build compiles the name out: no environment setting changes a product there
// (tests/test_abi.py looks for the names in the library).
#ifdef SPMM_TUNING
#define tuning_env_int(NAME, DFLT)                \
  ([] {                                           \
    static const int v = [] {                     \
      const char* e = getenv(NAME);               \
      return e ? atoi(e) : (DFLT);                \
    }();                                          \
    return v;                                     \
  }())
#else
#define tuning_env_int(NAME, DFLT) (DFLT)
#endif

// f(std::integral_constant<int, D>{}), D the value a release build derives at compile
// time. A TUNING build, where an override may have replaced it, takes v among V... at run
// time instead (with_int), so only that build instantiates f for every V.
template <int D, int... V, typename F>
void with_tuned_int(int v, F&& f) {
  if constexpr (kTuning) with_int<V...>(v, f);
  else f(std::integral_constant<int, D>{});
}

// The timing pair around a launcher's body, closed on every path. A body that fails
// returns its own status; else the launches' error, read after the stop event is recorded.
template <typename F>
spmm_status_t timed(spmm_context* ctx, F&& body) {
  const int slot = timing_begin(ctx);
  const spmm_status_t st = body();
  timing_end(ctx, slot);
  return st != SPMM_STATUS_SUCCESS ? st : from_hip(hipGetLastError());
}

}  // namespace spmm
