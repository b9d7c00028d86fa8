// dispatch_trace.hpp — host-only trace of which kernel instantiation a launcher reaches.
//
// Included by csr_kernels.hip and bsr_kernels.hip after their other includes, under
// -DSPMM_DISPATCH_TRACE only (make bin/dispatch_trace, --offload-host-only objects in
// build/trace/; the shipped objects never see it). Every hipLaunchKernelGGL becomes one
// line of text, handed to spmm_trace::emit, instead of a launch:
//   <mangled KTag<kernel>> g=<x>,<y>,<z> b=<x> <arg> <arg> ...
// The tag's mangled name holds the kernel's own symbol with its template arguments as the
// compiler resolved them, however the launch site spelled them. Arguments are converted to
// the kernel's parameter types first, as the launch would, and printed by value (integers,
// bools, floats), as null / ptr (pointers; no device memory is touched) or as obj (structs).
// drivers/dispatch_trace.cpp walks the launchers over an argument grid;
// tests/test_dispatch_trace.py compares the output with tests/golden/dispatch_trace.txt.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>
#include <tuple>
#include <type_traits>
#include <typeinfo>
#include <utility>

#include "kernel_tag.hpp"

namespace spmm_trace {

// One finished line (no newline). Defined by the program that links the traced objects.
void emit(const std::string& line);

template <typename P>
void print_arg(std::string& s, const P& v) {
  if constexpr (std::is_pointer_v<P>) s += v ? " ptr" : " null";
  else if constexpr (std::is_same_v<P, bool>) s += v ? " true" : " false";
  else if constexpr (std::is_integral_v<P>) s += " " + std::to_string((long long)v);
  else if constexpr (std::is_floating_point_v<P>) {
    char buf[32];
    std::snprintf(buf, sizeof buf, " %g", (double)v);
    s += buf;
  } else s += " obj";
}

// (a launch may leave trailing defaulted parameters out: those are not printed)
template <typename... P, typename... A, size_t... I>
void print_args(std::string& s, void (*)(P...), std::index_sequence<I...>, const A&... a) {
  static_assert(sizeof...(A) <= sizeof...(P), "more arguments than kernel parameters");
  (print_arg<std::tuple_element_t<I, std::tuple<P...>>>(s, a), ...);
}

template <auto K, typename... A>
void trace_launch(dim3 grid, dim3 block, const A&... a) {
  std::string s = typeid(KTag<K>).name();
  s += " g=" + std::to_string(grid.x) + "," + std::to_string(grid.y) + "," +
       std::to_string(grid.z) + " b=" + std::to_string(block.x);
  print_args(s, K, std::index_sequence_for<A...>{}, a...);
  emit(s);
}

}  // namespace spmm_trace

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(K, G, B, SH, ST, ...) \
  ::spmm_trace::trace_launch<K>(dim3(G), dim3(B), ##__VA_ARGS__)
// no device here: the probe paths go on past their memset, and a launcher's status does not
// depend on whether the machine has one
#define hipMemsetAsync(...) hipSuccess
#define hipGetLastError() hipSuccess
