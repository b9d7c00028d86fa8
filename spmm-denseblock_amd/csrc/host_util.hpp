// host_util.hpp — shared host-side helpers of libspmm_hip.so (threads, CSR validation).
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <exception>
#include <thread>
#include <vector>

namespace spmm_host {

// Worker count: OMP_NUM_THREADS if set, else the hardware threads, capped at 32.
inline int num_threads() {
  unsigned t = std::thread::hardware_concurrency();
  if (const char* e = std::getenv("OMP_NUM_THREADS")) t = (unsigned)std::max(1, std::atoi(e));
  return (int)std::max(1u, std::min(t, 32u));
}

// Runs f(t) for t in [0, nt) on nt threads (inline when nt <= 1). What a worker or the
// start of a thread throws (an allocation failure) is rethrown here once every started
// worker is joined: nothing escapes on a worker thread, which would be std::terminate.
template <typename F>
void run_workers(int nt, F f) {
  if (nt <= 1) {
    if (nt == 1) f(0);
    return;
  }
  std::vector<std::exception_ptr> err((size_t)nt);
  std::vector<std::thread> th;
  th.reserve((size_t)nt);
  std::exception_ptr start_err;
  try {
    for (int t = 0; t < nt; ++t)
      th.emplace_back([&err, &f, t] {
        try {
          f(t);
        } catch (...) {
          err[(size_t)t] = std::current_exception();
        }
      });
  } catch (...) {
    start_err = std::current_exception();
  }
  for (auto& x : th) x.join();
  if (start_err) std::rethrow_exception(start_err);
  for (auto& e : err)
    if (e) std::rethrow_exception(e);
}

// Runs f(lo, hi) over [0, n) in contiguous chunks on worker threads.
template <typename F>
void parallel_for(int64_t n, F f) {
  const int nt = (int)std::min<int64_t>(num_threads(), std::max<int64_t>(1, n / 4096));
  if (nt <= 1) {
    f((int64_t)0, n);
    return;
  }
  run_workers(nt, [&](int t) { f(n * t / nt, n * (t + 1) / nt); });
}

// A 0-based CSR pattern of n rows: rowptr[0] == 0, no decreasing row pointer, every
// column in [0, ncols). n == 0 is valid whatever the pointers are.
inline bool valid_csr(int n, const int* rowptr, const int* colind, int64_t ncols) {
  if (n < 0 || (n > 0 && !rowptr)) return false;
  if (n == 0) return true;
  if (rowptr[0] != 0) return false;
  for (int i = 0; i < n; ++i)
    if (rowptr[i + 1] < rowptr[i]) return false;
  if (rowptr[n] > 0 && !colind) return false;
  std::atomic<bool> ok{true};
  parallel_for(rowptr[n], [&](int64_t lo, int64_t hi) {
    for (int64_t j = lo; j < hi; ++j)
      if (colind[j] < 0 || colind[j] >= ncols) {
        ok = false;
        return;
      }
  });
  return ok.load();
}

}  // namespace spmm_host
