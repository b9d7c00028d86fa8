// launch_record.hpp — the one way a kernel is launched: SPMM_LAUNCH(ctx, kernel, grid, block,
// shared, args...) queues the kernel on the handle's stream and, when the handle's launch
// record is on (spmm_set_launch_record), first appends the kernel's identifier to it.
//
// The identifier is typeid(KTag<kernel>).name() (kernel_tag.hpp), a static string: recording
// is host-side, allocates nothing per launch beyond the list's own growth, and costs one test
// of a flag when it is off. It records what was queued, so it also works while the stream is
// capturing. The list is appended to without a lock: like the handle's stream and buffers it
// belongs to the one host thread that drives the handle (context.hpp). The launch itself is
// hipLaunchKernelGGL as before, so the device code does not depend on this header, and the
// host-only dispatch trace (dispatch_trace.hpp, which turns hipLaunchKernelGGL into a line
// of text) sees every launch through it.
#pragma once

#include <hip/hip_runtime.h>

#include <typeinfo>

#include "context.hpp"
#include "kernel_tag.hpp"

namespace spmm {

template <auto K>
inline const char* launch_id() {
  return typeid(spmm_trace::KTag<K>).name();
}
// (the identifier apart from the launch: for a kernel chosen at run time as a pointer)
inline void note_launch(spmm_context* ctx, const char* id) {
  if (ctx->record) ctx->launches.push_back(id);
}
template <auto K>
inline void note_launch(spmm_context* ctx) {
  note_launch(ctx, launch_id<K>());
}

}  // namespace spmm

#define SPMM_LAUNCH(CTX, K, G, B, SH, ...)                             \
  do {                                                                 \
    ::spmm::note_launch<K>(CTX);                                       \
    hipLaunchKernelGGL(K, G, B, SH, (CTX)->stream, ##__VA_ARGS__);     \
  } while (0)
