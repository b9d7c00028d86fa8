// kernel_tag.hpp — a kernel instantiation as a type, whose mangled name holds the kernel's
// own symbol with its template arguments as the compiler resolved them, however the launch
// site spelled them. typeid(KTag<K>).name() is the identifier of a launch in both the
// host-only dispatch trace (dispatch_trace.hpp) and a handle's launch record
// (launch_record.hpp); tests/kernel_keys.py maps it onto the .amdhsa_kernel symbol.
#pragma once

namespace spmm_trace {

template <auto K>
struct KTag {};

}  // namespace spmm_trace
