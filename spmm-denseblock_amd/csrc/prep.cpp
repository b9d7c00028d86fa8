// prep.cpp — host-side preprocessing: csr2bsr, bsr2csr, nnzb, row partition.
//
// north_star keeps format conversion as CPU-side preprocessing; these replace
// the GPU cuSPARSE conversions of the reference drivers:
//   cusparseXcsr2bsrNnz + cusparseScsr2bsr   run_bsrmm.cu:116-142, csr2bsr.cu:176-192
//   cusparseSbsr2csr                         bsr2csr.cu:177-188
//   calculateNnzb                            utility.cc:47-69
// and the CPU block extraction of divide_matrix (divide.cu:52-127) at
// density -> 0. Index arrays are bit-exact with the oracle (tests/test_prep.py).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <atomic>
#include <thread>
#include <vector>

#include "host_util.hpp"
#include "softmax_rule.hpp"

#include "spmm_hip.h"

namespace {

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// Collects the sorted distinct block columns of block row `br`.
// `mark` has nb entries, all -1 on entry and on exit.
// Returns false on a column index outside [0, nb*bs).
bool block_cols(int br, int bs, int m, const int* rowptr, const int* colind, int base,
                std::vector<int>& mark, std::vector<int>& out) {
  out.clear();
  const int r0 = br * bs, r1 = std::min(m, r0 + bs);
  const int nb = (int)mark.size();
  for (int r = r0; r < r1; ++r) {
    for (int j = rowptr[r] - base; j < rowptr[r + 1] - base; ++j) {
      const int c = colind[j] - base;
      if (c < 0 || c / bs >= nb) {
        for (int bc : out) mark[bc] = -1;
        return false;
      }
      const int bc = c / bs;
      if (mark[bc] < 0) {
        mark[bc] = 0;
        out.push_back(bc);
      }
    }
  }
  for (int bc : out) mark[bc] = -1;
  std::sort(out.begin(), out.end());
  return true;
}

}  // namespace

extern "C" {

// Block rows are independent: counts and fills run on worker threads (each
// with its own marker array), the prefix sums in between are sequential.
spmm_status_t spmm_xcsr2bsr_nnz(spmm_direction_t dir, int m, int n, const int* csrRowPtr,
                                const int* csrColInd, int blockDim, int* bsrRowPtr,
                                int* nnzbTotal) try {
  if (dir != SPMM_DIRECTION_ROW && dir != SPMM_DIRECTION_COLUMN) return SPMM_STATUS_INVALID_VALUE;
  if (m < 0 || n < 0 || blockDim <= 0) return SPMM_STATUS_INVALID_VALUE;
  if (!csrRowPtr || !bsrRowPtr || !nnzbTotal) return SPMM_STATUS_INVALID_VALUE;
  const int mb = ceil_div(m, blockDim), nb = ceil_div(n, blockDim);
  if (m > 0 && csrRowPtr[m] - csrRowPtr[0] > 0 && !csrColInd) return SPMM_STATUS_INVALID_VALUE;
  const int base = m > 0 ? csrRowPtr[0] : 0;
  std::vector<int> cnt(mb);
  std::atomic<bool> ok{true};
  spmm_host::parallel_for(mb, [&](int64_t lo, int64_t hi) {
    std::vector<int> mark(std::max(nb, 1), -1), cols;
    for (int64_t br = lo; br < hi && ok; ++br) {
      if (!block_cols((int)br, blockDim, m, csrRowPtr, csrColInd, base, mark, cols)) ok = false;
      cnt[br] = (int)cols.size();
    }
  });
  if (!ok) return SPMM_STATUS_INVALID_VALUE;
  bsrRowPtr[0] = 0;
  long long acc = 0;
  for (int br = 0; br < mb; ++br) {
    acc += cnt[br];
    if (acc > INT32_MAX) return SPMM_STATUS_INVALID_VALUE;
    bsrRowPtr[br + 1] = (int)acc;
  }
  *nnzbTotal = (int)acc;
  return SPMM_STATUS_SUCCESS;
} catch (...) {  // no exception leaves the C ABI
  return SPMM_STATUS_ALLOC_FAILED;
}

spmm_status_t spmm_scsr2bsr(spmm_direction_t dir, int m, int n, const float* csrVal,
                            const int* csrRowPtr, const int* csrColInd, int blockDim,
                            const int* bsrRowPtr, float* bsrVal, int* bsrColInd) try {
  if (dir != SPMM_DIRECTION_ROW && dir != SPMM_DIRECTION_COLUMN) return SPMM_STATUS_INVALID_VALUE;
  if (m < 0 || n < 0 || blockDim <= 0) return SPMM_STATUS_INVALID_VALUE;
  if (!csrRowPtr || !bsrRowPtr) return SPMM_STATUS_INVALID_VALUE;
  const int bs = blockDim;
  const int mb = ceil_div(m, bs), nb = ceil_div(n, bs);
  const int nnzb = bsrRowPtr[mb];
  if (nnzb > 0 && (!bsrVal || !bsrColInd || !csrColInd || !csrVal))
    return SPMM_STATUS_INVALID_VALUE;
  const int base = m > 0 ? csrRowPtr[0] : 0;
  const size_t bs2 = (size_t)bs * bs;
  std::atomic<bool> ok{true};
  spmm_host::parallel_for(mb, [&](int64_t lo, int64_t hi) {
    std::vector<int> mark(std::max(nb, 1), -1), cols;
    for (int64_t br = lo; br < hi && ok; ++br) {
      if (!block_cols((int)br, bs, m, csrRowPtr, csrColInd, base, mark, cols)) {
        ok = false;
        return;
      }
      const int k0 = bsrRowPtr[br];
      if (bsrRowPtr[br + 1] - k0 != (int)cols.size()) {
        ok = false;
        return;
      }
      for (size_t t = 0; t < cols.size(); ++t) {
        bsrColInd[k0 + t] = cols[t];
        mark[cols[t]] = k0 + (int)t;
      }
      std::memset(bsrVal + (size_t)k0 * bs2, 0, cols.size() * bs2 * sizeof(float));
      const int r0 = (int)br * bs, r1 = std::min(m, r0 + bs);
      for (int r = r0; r < r1; ++r) {
        const int rr = r - r0;
        for (int j = csrRowPtr[r] - base; j < csrRowPtr[r + 1] - base; ++j) {
          const int c = csrColInd[j] - base;
          const int k = mark[c / bs], cc = c % bs;
          const size_t off = (size_t)k * bs2 + (dir == SPMM_DIRECTION_ROW
                                                    ? (size_t)rr * bs + cc
                                                    : (size_t)cc * bs + rr);
          bsrVal[off] += csrVal[j];  // duplicates summed, in CSR order
        }
      }
      for (int bc : cols) mark[bc] = -1;
    }
  });
  return ok ? SPMM_STATUS_SUCCESS : SPMM_STATUS_INVALID_VALUE;
} catch (...) {  // no exception leaves the C ABI
  return SPMM_STATUS_ALLOC_FAILED;
}

spmm_status_t spmm_sbsr2csr(spmm_direction_t dir, int mb, int nb, const float* bsrVal,
                            const int* bsrRowPtr, const int* bsrColInd, int blockDim,
                            float* csrVal, int* csrRowPtr, int* csrColInd) try {
  if (dir != SPMM_DIRECTION_ROW && dir != SPMM_DIRECTION_COLUMN) return SPMM_STATUS_INVALID_VALUE;
  if (mb < 0 || nb < 0 || blockDim <= 0) return SPMM_STATUS_INVALID_VALUE;
  if (!bsrRowPtr || !csrRowPtr) return SPMM_STATUS_INVALID_VALUE;
  const int bs = blockDim;
  const size_t bs2 = (size_t)bs * bs;
  const int base = mb > 0 ? bsrRowPtr[0] : 0;
  if (mb > 0 && bsrRowPtr[mb] - base > 0 && (!bsrVal || !bsrColInd || !csrVal || !csrColInd))
    return SPMM_STATUS_INVALID_VALUE;
  long long pos = 0;
  csrRowPtr[0] = 0;
  for (int br = 0; br < mb; ++br) {
    const int k0 = bsrRowPtr[br] - base, k1 = bsrRowPtr[br + 1] - base;
    for (int rr = 0; rr < bs; ++rr) {
      for (int k = k0; k < k1; ++k) {
        const long long cb = (long long)(bsrColInd[k] - base) * bs;
        const float* blk = bsrVal + (size_t)k * bs2;
        for (int c = 0; c < bs; ++c) {
          csrColInd[pos] = (int)(cb + c);
          csrVal[pos] = dir == SPMM_DIRECTION_ROW ? blk[(size_t)rr * bs + c]
                                                  : blk[(size_t)c * bs + rr];
          ++pos;
        }
      }
      if (pos > INT32_MAX) return SPMM_STATUS_INVALID_VALUE;
      csrRowPtr[(size_t)br * bs + rr + 1] = (int)pos;
    }
  }
  (void)nb;
  return SPMM_STATUS_SUCCESS;
} catch (...) {  // no exception leaves the C ABI
  return SPMM_STATUS_ALLOC_FAILED;
}

int64_t spmm_calculate_nnzb(int n, const int* csrRowPtr, const int* csrColInd, int blockDim) try {
  if (n < 0 || blockDim <= 0 || !csrRowPtr) return -1;
  const int mb = ceil_div(n, blockDim);
  const int base = n > 0 ? csrRowPtr[0] : 0;
  int maxc = 0;
  // (n == 0: no entries whatever csrRowPtr[0] is, a base-1 pointer included)
  for (int j = 0; n > 0 && j < csrRowPtr[n] - base; ++j) maxc = std::max(maxc, csrColInd[j] - base);
  const int nb = std::max(ceil_div(n, blockDim), maxc / blockDim + 1);
  std::vector<int> mark(std::max(nb, 1), -1), cols;
  int64_t total = 0;
  for (int br = 0; br < mb; ++br) {
    if (!block_cols(br, blockDim, n, csrRowPtr, csrColInd, base, mark, cols)) return -1;
    total += (int64_t)cols.size();
  }
  return total;
} catch (...) {  // no exception leaves the C ABI
  return -1;
}

spmm_status_t spmm_csr_partition_rows(int m, const int* csrRowPtr, int nparts, int* bounds) try {
  if (m < 0 || nparts <= 0 || !csrRowPtr || !bounds) return SPMM_STATUS_INVALID_VALUE;
  // Cost of the prefix [0, i) = nnz before row i + i (one unit per row for
  // its output write), monotone in i: cut at equal cost quantiles.
  const long long base = csrRowPtr[0];
  const long long total = (long long)csrRowPtr[m] - base + m;
  bounds[0] = 0;
  for (int p = 1; p < nparts; ++p) {
    const long long target = (total * p) / nparts;
    int lo = bounds[p - 1], hi = m;
    while (lo < hi) {  // first i with cost(i) >= target
      const int mid = lo + (hi - lo) / 2;
      const long long cost = (long long)csrRowPtr[mid] - base + mid;
      if (cost < target) lo = mid + 1; else hi = mid;
    }
    bounds[p] = lo;
  }
  bounds[nparts] = m;
  return SPMM_STATUS_SUCCESS;
} catch (...) {  // no exception leaves the C ABI
  return SPMM_STATUS_ALLOC_FAILED;
}

// CSR -> CSC: the stable counting sort of the CSR positions by column (no reference
// counterpart; the device form, spmm_csr2csc_dev, is compared against this one). The
// column counts are integer atomics (order-independent), the column pointer a sequential
// prefix sum; the fill gives every worker a range of columns holding about nnz / workers
// entries, and each worker walks all entries in CSR order and places those of its own
// columns, so the order inside a column is the CSR order whatever the worker count.
spmm_status_t spmm_csr2csc(int m, int n, int nnz, const void* csrVal, const int* csrRowPtr,
                           const int* csrColInd, int valueBytes, spmm_index_base_t baseA,
                           spmm_index_base_t baseC, void* cscVal, int* cscColPtr,
                           int* cscRowInd, int* perm) try {
  if (m < 0 || n < 0 || nnz < 0) return SPMM_STATUS_INVALID_VALUE;
  if (valueBytes != 0 && valueBytes != 2 && valueBytes != 4 && valueBytes != 8)
    return SPMM_STATUS_INVALID_VALUE;
  if ((baseA != SPMM_INDEX_BASE_ZERO && baseA != SPMM_INDEX_BASE_ONE) ||
      (baseC != SPMM_INDEX_BASE_ZERO && baseC != SPMM_INDEX_BASE_ONE))
    return SPMM_STATUS_INVALID_VALUE;
  if (!csrRowPtr || !cscColPtr) return SPMM_STATUS_INVALID_VALUE;
  if (nnz > 0 && (!csrColInd || !cscRowInd || (valueBytes > 0 && (!csrVal || !cscVal))))
    return SPMM_STATUS_INVALID_VALUE;
  const int ba = (int)baseA, bc = (int)baseC;
  const int64_t p0 = (int64_t)csrRowPtr[0] - ba;
  if (p0 < 0 || (int64_t)csrRowPtr[m] - csrRowPtr[0] != nnz) return SPMM_STATUS_INVALID_VALUE;
  std::atomic<bool> ok{true};
  spmm_host::parallel_for(m, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r)
      if (csrRowPtr[r + 1] < csrRowPtr[r]) ok = false;
  });
  if (!ok) return SPMM_STATUS_INVALID_VALUE;
  std::vector<int> cnt((size_t)n + 1, 0);  // cnt[c + 1]: entries of column c, then cursors
  spmm_host::parallel_for(nnz, [&](int64_t lo, int64_t hi) {
    for (int64_t i = lo; i < hi; ++i) {
      const int c = csrColInd[p0 + i] - ba;
      if (c < 0 || c >= n) {
        ok = false;
        return;
      }
      __atomic_fetch_add(&cnt[(size_t)c + 1], 1, __ATOMIC_RELAXED);
    }
  });
  if (!ok) return SPMM_STATUS_INVALID_VALUE;
  cscColPtr[0] = bc;
  int64_t acc = 0;
  for (int c = 0; c < n; ++c) {
    const int here = cnt[(size_t)c + 1];
    cnt[(size_t)c + 1] = (int)acc;  // cursor of column c (cnt[0] stays unused)
    acc += here;
    cscColPtr[c + 1] = (int)(acc + bc);
  }
  if (nnz == 0) return SPMM_STATUS_SUCCESS;
  const int nt = (int)std::min<int64_t>(spmm_host::num_threads(), std::max<int64_t>(1, nnz / 65536));
  // worker t owns the columns [cut[t], cut[t + 1]): cuts at equal shares of the entries
  std::vector<int> cut((size_t)nt + 1, n);
  cut[0] = 0;
  for (int t = 1; t < nt; ++t) {
    const int64_t target = (int64_t)nnz * t / nt + bc;
    cut[t] = (int)(std::lower_bound(cscColPtr, cscColPtr + n, (int)target) - cscColPtr);
  }
  auto fill = [&](int clo, int chi) {
    for (int r = 0; r < m; ++r)
      for (int64_t p = (int64_t)csrRowPtr[r] - ba; p < (int64_t)csrRowPtr[r + 1] - ba; ++p) {
        const int c = csrColInd[p] - ba;
        if (c < clo || c >= chi) continue;
        const size_t dst = (size_t)cnt[(size_t)c + 1]++;
        cscRowInd[dst] = r + bc;
        if (perm) perm[dst] = (int)p;
        if (valueBytes)
          std::memcpy(static_cast<char*>(cscVal) + dst * valueBytes,
                      static_cast<const char*>(csrVal) + (size_t)p * valueBytes, valueBytes);
      }
  };
  spmm_host::run_workers(nt, [&](int t) {
    if (cut[t] < cut[t + 1]) fill(cut[t], cut[t + 1]);
  });
  return SPMM_STATUS_SUCCESS;
} catch (...) {  // no exception leaves the C ABI
  return SPMM_STATUS_ALLOC_FAILED;
}

}  // extern "C"

namespace {

// The dot of the sampled product's rule (include/spmm_hip.h): chain l of
// G sums the columns c with (c / 4) mod G == l in ascending c by fp32 FMA from +0, and
// the chains fold pairwise over adjacent lanes, level by level (the butterfly
// acc_l + acc_(l xor s), s = 1, 2, ..., G / 2).
inline int sddmm_group_lanes(int n) {
  const int chunks = (n + 3) / 4;
  int g = 1;
  while (g < chunks && g < 64) g <<= 1;
  return g;
}

inline float sddmm_dot(const float* x, const float* y, int n, int G) {
  float acc[64];
  for (int l = 0; l < G; ++l) {
    float a = 0.f;
    for (int c0 = 4 * l; c0 < n; c0 += 4 * G)
      for (int c = c0; c < std::min(c0 + 4, n); ++c) a = __builtin_fmaf(x[c], y[c], a);
    acc[l] = a;
  }
  for (int w = G; w > 1; w >>= 1)
    for (int l = 0; l < w / 2; ++l) acc[l] = acc[2 * l] + acc[2 * l + 1];
  return acc[0];
}

}  // namespace

extern "C" {

// The sampled dense-dense product on the host: the written rule in executable form (the
// device entry, spmm_sddmm_csr_f32, equals it bit for bit). Workers take equal shares of
// the positions; an output depends on its own two rows alone, so the worker count
// cannot change a bit.
spmm_status_t spmm_sddmm_csr_host_f32(int m, int n, int k, int nnz, float alpha,
                                      const int* csrRowPtr, const int* csrColInd,
                                      spmm_index_base_t base, const float* X, int ldx,
                                      const float* Y, int ldy, float beta, float* outVal) try {
  if (m < 0 || n < 0 || k < 0 || nnz < 0) return SPMM_STATUS_INVALID_VALUE;
  if (base != SPMM_INDEX_BASE_ZERO && base != SPMM_INDEX_BASE_ONE)
    return SPMM_STATUS_INVALID_VALUE;
  if (ldx < n || ldy < n) return SPMM_STATUS_INVALID_VALUE;
  if (nnz > 0 && (!csrRowPtr || !csrColInd || !outVal || (n > 0 && (!X || !Y))))
    return SPMM_STATUS_INVALID_VALUE;
  if (m == 0 || nnz == 0) return SPMM_STATUS_SUCCESS;
  const int ba = (int)base;
  const int64_t p0 = (int64_t)csrRowPtr[0] - ba, p1 = (int64_t)csrRowPtr[m] - ba;
  if (p0 < 0 || p1 < p0 || p1 > nnz) return SPMM_STATUS_INVALID_VALUE;
  std::atomic<bool> ok{true};
  spmm_host::parallel_for(m, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r)
      if (csrRowPtr[r + 1] < csrRowPtr[r]) ok = false;
  });
  spmm_host::parallel_for(p1 - p0, [&](int64_t lo, int64_t hi) {
    for (int64_t p = p0 + lo; p < p0 + hi; ++p)
      if (csrColInd[p] - ba < 0 || csrColInd[p] - ba >= k) ok = false;
  });
  if (!ok) return SPMM_STATUS_INVALID_VALUE;
  const int G = sddmm_group_lanes(n);
  spmm_host::parallel_for(p1 - p0, [&](int64_t lo, int64_t hi) {
    if (lo >= hi) return;
    // the row of the share's first position: the last row that starts at or before it
    int r = (int)(std::upper_bound(csrRowPtr, csrRowPtr + m, (int)(p0 + lo + ba)) - csrRowPtr) - 1;
    for (int64_t p = p0 + lo; p < p0 + hi; ++p) {
      while (p >= (int64_t)csrRowPtr[r + 1] - ba) ++r;
      const float d = sddmm_dot(X + (int64_t)r * ldx, Y + (int64_t)(csrColInd[p] - ba) * ldy, n, G);
      outVal[p] = beta == 0.f ? alpha * d : __builtin_fmaf(beta, outVal[p], alpha * d);
    }
  });
  return SPMM_STATUS_SUCCESS;
} catch (...) {  // no exception leaves the C ABI
  return SPMM_STATUS_ALLOC_FAILED;
}

}  // extern "C"

namespace {

// The SUM of the edge softmax's rule (include/spmm_hip.h) over a row of L
// positions: pieces of 1024 positions from the row's start; in a piece chain c of 64 takes
// the positions = c (mod 64) in ascending order from +0 (term(acc, q) appends position q),
// the chains fold pairwise over adjacent chains, level by level (the butterfly
// acc_l + acc_(l xor s), s = 1, 2, ..., 32), and the piece sums are added in ascending
// order.
template <typename Term>
inline float softmax_row_sum(int64_t L, Term term) {
  constexpr int C = spmm_rule::kSoftmaxChains, P = spmm_rule::kSoftmaxPiece;
  float s = 0.f;
  for (int64_t q0 = 0; q0 < L; q0 += P) {
    float acc[C];
    for (int c = 0; c < C; ++c) {
      float a = 0.f;
      for (int64_t q = q0 + c; q < std::min<int64_t>(q0 + P, L); q += C) a = term(a, q);
      acc[c] = a;
    }
    for (int w = C; w > 1; w >>= 1)
      for (int l = 0; l < w / 2; ++l) acc[l] = acc[2 * l] + acc[2 * l + 1];
    s += acc[0];
  }
  return s;
}

// The checks the two host forms share (the order of spmm_sddmm_csr_host_f32's); *done:
// nothing to do.
spmm_status_t softmax_host_check(int m, int nnz, const int* rp, spmm_index_base_t base,
                                 bool null_ptr, bool* done) {
  *done = true;
  if (m < 0 || nnz < 0) return SPMM_STATUS_INVALID_VALUE;
  if (base != SPMM_INDEX_BASE_ZERO && base != SPMM_INDEX_BASE_ONE)
    return SPMM_STATUS_INVALID_VALUE;
  if (nnz > 0 && (!rp || null_ptr)) return SPMM_STATUS_INVALID_VALUE;
  if (m == 0 || nnz == 0) return SPMM_STATUS_SUCCESS;
  const int ba = (int)base;
  const int64_t p0 = (int64_t)rp[0] - ba, p1 = (int64_t)rp[m] - ba;
  if (p0 < 0 || p1 < p0 || p1 > nnz) return SPMM_STATUS_INVALID_VALUE;
  std::atomic<bool> ok{true};
  spmm_host::parallel_for(m, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r)
      if (rp[r + 1] < rp[r]) ok = false;
  });
  if (!ok) return SPMM_STATUS_INVALID_VALUE;
  *done = false;
  return SPMM_STATUS_SUCCESS;
}

}  // namespace

extern "C" {

// The edge softmax and its backward on the host: the written rule in executable form (the
// device entries equal them bit for bit). Workers take equal shares of the rows; an output
// depends on its own row alone, so the worker count cannot change a bit. y may be x, gx
// may be g: a row's inputs are read completely before its first output is written, except
// the position's own.
spmm_status_t spmm_edge_softmax_csr_host_f32(int m, int nnz, const int* csrRowPtr,
                                             spmm_index_base_t base, const float* x, float* y) try {
  bool done;
  const spmm_status_t st = softmax_host_check(m, nnz, csrRowPtr, base, !x || !y, &done);
  if (done) return st;
  const int ba = (int)base;
  spmm_host::parallel_for(m, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r) {
      const int64_t a = (int64_t)csrRowPtr[r] - ba, L = (int64_t)csrRowPtr[r + 1] - ba - a;
      const float* xr = x + a;
      float mx = -__builtin_inff();
      for (int64_t q = 0; q < L; ++q) mx = __builtin_fmaxf(mx, xr[q]);
      const float s = softmax_row_sum(L, [&](float acc, int64_t q) {
        return acc + spmm_rule::softmax_exp(xr[q] - mx);
      });
      for (int64_t q = 0; q < L; ++q) y[a + q] = spmm_rule::softmax_exp(xr[q] - mx) / s;
    }
  });
  return SPMM_STATUS_SUCCESS;
} catch (...) {  // no exception leaves the C ABI
  return SPMM_STATUS_ALLOC_FAILED;
}

spmm_status_t spmm_edge_softmax_bwd_csr_host_f32(int m, int nnz, const int* csrRowPtr,
                                                 spmm_index_base_t base, const float* y,
                                                 const float* g, float* gx) try {
  bool done;
  const spmm_status_t st = softmax_host_check(m, nnz, csrRowPtr, base, !y || !g || !gx, &done);
  if (done) return st;
  const int ba = (int)base;
  spmm_host::parallel_for(m, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r) {
      const int64_t a = (int64_t)csrRowPtr[r] - ba, L = (int64_t)csrRowPtr[r + 1] - ba - a;
      const float* yr = y + a;
      const float* gr = g + a;
      const float d = softmax_row_sum(L, [&](float acc, int64_t q) {
        return __builtin_fmaf(yr[q], gr[q], acc);
      });
      for (int64_t q = 0; q < L; ++q) {
        const float diff = gr[q] - d;
        gx[a + q] = yr[q] * diff;
      }
    }
  });
  return SPMM_STATUS_SUCCESS;
} catch (...) {  // no exception leaves the C ABI
  return SPMM_STATUS_ALLOC_FAILED;
}

// The three ops over `heads` heads (include/spmm_hip.h): per-edge values
// [nnz, heads], per-node features with head h in the columns [h d, (h + 1) d); per head the
// rule of the single-head form above, so heads = 1 is that form bit for bit.
spmm_status_t spmm_sddmm_csr_heads_host_f32(int m, int d, int k, int nnz, int heads, float alpha,
                                            const int* csrRowPtr, const int* csrColInd,
                                            spmm_index_base_t base, const float* X, int ldx,
                                            const float* Y, int ldy, float beta,
                                            float* outVal) try {
  if (m < 0 || d < 0 || k < 0 || nnz < 0 || heads < 1) return SPMM_STATUS_INVALID_VALUE;
  if (base != SPMM_INDEX_BASE_ZERO && base != SPMM_INDEX_BASE_ONE)
    return SPMM_STATUS_INVALID_VALUE;
  if (ldx < (int64_t)heads * d || ldy < (int64_t)heads * d) return SPMM_STATUS_INVALID_VALUE;
  if (nnz > 0 && (!csrRowPtr || !csrColInd || !outVal || (d > 0 && (!X || !Y))))
    return SPMM_STATUS_INVALID_VALUE;
  if (m == 0 || nnz == 0) return SPMM_STATUS_SUCCESS;
  if ((int64_t)nnz * heads > INT32_MAX || d > 1024) return SPMM_STATUS_NOT_SUPPORTED;
  const int ba = (int)base;
  const int64_t p0 = (int64_t)csrRowPtr[0] - ba, p1 = (int64_t)csrRowPtr[m] - ba;
  if (p0 < 0 || p1 < p0 || p1 > nnz) return SPMM_STATUS_INVALID_VALUE;
  std::atomic<bool> ok{true};
  spmm_host::parallel_for(m, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r)
      if (csrRowPtr[r + 1] < csrRowPtr[r]) ok = false;
  });
  spmm_host::parallel_for(p1 - p0, [&](int64_t lo, int64_t hi) {
    for (int64_t p = p0 + lo; p < p0 + hi; ++p)
      if (csrColInd[p] - ba < 0 || csrColInd[p] - ba >= k) ok = false;
  });
  if (!ok) return SPMM_STATUS_INVALID_VALUE;
  const int G = sddmm_group_lanes(d);
  spmm_host::parallel_for(p1 - p0, [&](int64_t lo, int64_t hi) {
    if (lo >= hi) return;
    int r = (int)(std::upper_bound(csrRowPtr, csrRowPtr + m, (int)(p0 + lo + ba)) - csrRowPtr) - 1;
    for (int64_t p = p0 + lo; p < p0 + hi; ++p) {
      while (p >= (int64_t)csrRowPtr[r + 1] - ba) ++r;
      const float* xr = X + (int64_t)r * ldx;
      const float* yr = Y + (int64_t)(csrColInd[p] - ba) * ldy;
      for (int h = 0; h < heads; ++h) {
        const float dot = sddmm_dot(xr + (int64_t)h * d, yr + (int64_t)h * d, d, G);
        float& o = outVal[p * heads + h];
        o = beta == 0.f ? alpha * dot : __builtin_fmaf(beta, o, alpha * dot);
      }
    }
  });
  return SPMM_STATUS_SUCCESS;
} catch (...) {  // no exception leaves the C ABI
  return SPMM_STATUS_ALLOC_FAILED;
}

spmm_status_t spmm_edge_softmax_csr_heads_host_f32(int m, int nnz, int heads,
                                                   const int* csrRowPtr, spmm_index_base_t base,
                                                   const float* x, float* y) try {
  if (heads < 1) return SPMM_STATUS_INVALID_VALUE;
  bool done;
  const spmm_status_t st = softmax_host_check(m, nnz, csrRowPtr, base, !x || !y, &done);
  if (done) return st;
  if ((int64_t)nnz * heads > INT32_MAX) return SPMM_STATUS_NOT_SUPPORTED;
  const int ba = (int)base;
  spmm_host::parallel_for(m, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r) {
      const int64_t a = (int64_t)csrRowPtr[r] - ba, L = (int64_t)csrRowPtr[r + 1] - ba - a;
      for (int h = 0; h < heads; ++h) {
        const float* xr = x + a * heads + h;
        float mx = -__builtin_inff();
        for (int64_t q = 0; q < L; ++q) mx = __builtin_fmaxf(mx, xr[q * heads]);
        const float s = softmax_row_sum(L, [&](float acc, int64_t q) {
          return acc + spmm_rule::softmax_exp(xr[q * heads] - mx);
        });
        for (int64_t q = 0; q < L; ++q)
          y[(a + q) * heads + h] = spmm_rule::softmax_exp(xr[q * heads] - mx) / s;
      }
    }
  });
  return SPMM_STATUS_SUCCESS;
} catch (...) {  // no exception leaves the C ABI
  return SPMM_STATUS_ALLOC_FAILED;
}

spmm_status_t spmm_edge_softmax_bwd_csr_heads_host_f32(int m, int nnz, int heads,
                                                       const int* csrRowPtr,
                                                       spmm_index_base_t base, const float* y,
                                                       const float* g, float* gx) try {
  if (heads < 1) return SPMM_STATUS_INVALID_VALUE;
  bool done;
  const spmm_status_t st = softmax_host_check(m, nnz, csrRowPtr, base, !y || !g || !gx, &done);
  if (done) return st;
  if ((int64_t)nnz * heads > INT32_MAX) return SPMM_STATUS_NOT_SUPPORTED;
  const int ba = (int)base;
  spmm_host::parallel_for(m, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r) {
      const int64_t a = (int64_t)csrRowPtr[r] - ba, L = (int64_t)csrRowPtr[r + 1] - ba - a;
      for (int h = 0; h < heads; ++h) {
        const float* yr = y + a * heads + h;
        const float* gr = g + a * heads + h;
        const float dsum = softmax_row_sum(L, [&](float acc, int64_t q) {
          return __builtin_fmaf(yr[q * heads], gr[q * heads], acc);
        });
        for (int64_t q = 0; q < L; ++q) {
          const float diff = gr[q * heads] - dsum;
          gx[(a + q) * heads + h] = yr[q * heads] * diff;
        }
      }
    }
  });
  return SPMM_STATUS_SUCCESS;
} catch (...) {  // no exception leaves the C ABI
  return SPMM_STATUS_ALLOC_FAILED;
}

// The product's piece rule on the host: a row of L nonzeros is cut into
// pieces of max(128, ceil(L / 64)) nonzeros from its start, each a sequential chain
// fma(val, b, acc) from +0, the pieces added left to right from -0 (an empty row is +0).
spmm_status_t spmm_csrmm_heads_host_f32(int m, int d, int k, int nnz, int heads, float alpha,
                                        const int* csrRowPtr, const int* csrColInd,
                                        const float* csrVal, spmm_index_base_t base,
                                        const float* B, int ldb, float beta, float* C,
                                        int ldc) try {
  if (m < 0 || d < 0 || k < 0 || nnz < 0 || heads < 1) return SPMM_STATUS_INVALID_VALUE;
  if (base != SPMM_INDEX_BASE_ZERO && base != SPMM_INDEX_BASE_ONE)
    return SPMM_STATUS_INVALID_VALUE;
  if (m == 0 || d == 0) return SPMM_STATUS_SUCCESS;
  if (!csrRowPtr || !C || (k > 0 && !B) || (nnz > 0 && (!csrColInd || !csrVal)))
    return SPMM_STATUS_INVALID_VALUE;
  if (ldb < (int64_t)heads * d || ldc < (int64_t)heads * d) return SPMM_STATUS_INVALID_VALUE;
  if ((int64_t)nnz * heads > INT32_MAX) return SPMM_STATUS_NOT_SUPPORTED;
  const int ba = (int)base;
  const int64_t p0 = (int64_t)csrRowPtr[0] - ba, p1 = (int64_t)csrRowPtr[m] - ba;
  if (p0 < 0 || p1 < p0 || p1 > nnz) return SPMM_STATUS_INVALID_VALUE;
  std::atomic<bool> ok{true};
  spmm_host::parallel_for(m, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r)
      if (csrRowPtr[r + 1] < csrRowPtr[r]) ok = false;
  });
  spmm_host::parallel_for(p1 - p0, [&](int64_t lo, int64_t hi) {
    for (int64_t p = p0 + lo; p < p0 + hi; ++p)
      if (csrColInd[p] - ba < 0 || csrColInd[p] - ba >= k) ok = false;
  });
  if (!ok) return SPMM_STATUS_INVALID_VALUE;
  spmm_host::parallel_for(m, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r) {
      const int64_t a = (int64_t)csrRowPtr[r] - ba, b = (int64_t)csrRowPtr[r + 1] - ba;
      const int64_t T = std::max<int64_t>(128, (b - a + 63) / 64);
      for (int h = 0; h < heads; ++h)
        for (int c = h * d; c < (h + 1) * d; ++c) {
          volatile float x = b > a ? -0.f : 0.f;  // no reassociation of the piece sums
          for (int64_t s = a; s < b; s += T) {
            float acc = 0.f;
            for (int64_t p = s; p < std::min(s + T, b); ++p)
              acc = __builtin_fmaf(csrVal[p * heads + h],
                                   B[(int64_t)(csrColInd[p] - ba) * ldb + c], acc);
            x = x + acc;
          }
          float& o = C[r * ldc + c];
          const float xs = x;
          o = beta == 0.f ? alpha * xs : __builtin_fmaf(beta, o, alpha * xs);
        }
    }
  });
  return SPMM_STATUS_SUCCESS;
} catch (...) {  // no exception leaves the C ABI
  return SPMM_STATUS_ALLOC_FAILED;
}

// The max / min reducers of the CSR product and their backward on the host:
// the written rules in executable form; the device entries equal them bit for bit. Workers
// take equal shares of the rows; an output depends on its own row alone.
//
// Forward: the terms of a row are walked in ascending position; a term takes over when the
// holder is not a NaN and the term is a NaN or strictly greater (less) under the IEEE
// comparison, so the winner is the lowest NaN position if there is one and otherwise the
// lowest position of the greatest (least) term. C holds the winner's own bits.
spmm_status_t spmm_csrmm_reduce_host_f32(spmm_reduce_t op, int m, int n, int k, int nnz,
                                         const int* csrRowPtr, const int* csrColInd,
                                         const float* csrVal, spmm_index_base_t base,
                                         const float* B, int ldb, float* C, int ldc, int* arg,
                                         int ldarg) try {
  if (m < 0 || n < 0 || k < 0 || nnz < 0) return SPMM_STATUS_INVALID_VALUE;
  if (op != SPMM_REDUCE_MAX && op != SPMM_REDUCE_MIN) return SPMM_STATUS_INVALID_VALUE;
  if (base != SPMM_INDEX_BASE_ZERO && base != SPMM_INDEX_BASE_ONE)
    return SPMM_STATUS_INVALID_VALUE;
  if (m == 0 || n == 0) return SPMM_STATUS_SUCCESS;
  if (!csrRowPtr || !C || (k > 0 && !B) || (nnz > 0 && !csrColInd))
    return SPMM_STATUS_INVALID_VALUE;
  if (ldb < n || ldc < n || (arg && ldarg < n)) return SPMM_STATUS_INVALID_VALUE;
  const int ba = (int)base;
  const int64_t p0 = (int64_t)csrRowPtr[0] - ba, p1 = (int64_t)csrRowPtr[m] - ba;
  if (p0 < 0 || p1 < p0 || p1 > nnz) return SPMM_STATUS_INVALID_VALUE;
  std::atomic<bool> ok{true};
  spmm_host::parallel_for(m, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r)
      if (csrRowPtr[r + 1] < csrRowPtr[r]) ok = false;
  });
  spmm_host::parallel_for(p1 - p0, [&](int64_t lo, int64_t hi) {
    for (int64_t p = p0 + lo; p < p0 + hi; ++p)
      if (csrColInd[p] - ba < 0 || csrColInd[p] - ba >= k) ok = false;
  });
  if (!ok) return SPMM_STATUS_INVALID_VALUE;
  const bool mn = op == SPMM_REDUCE_MIN;
  spmm_host::parallel_for(m, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r) {
      const int64_t a = (int64_t)csrRowPtr[r] - ba, b = (int64_t)csrRowPtr[r + 1] - ba;
      float* cr = C + r * ldc;
      int* wr = arg ? arg + r * ldarg : nullptr;
      if (a == b)
        for (int c = 0; c < n; ++c) {
          cr[c] = 0.f;
          if (wr) wr[c] = -1;
        }
      for (int64_t p = a; p < b; ++p) {
        const float* br = B + (int64_t)(csrColInd[p] - ba) * ldb;
        for (int c = 0; c < n; ++c) {
          float t = br[c];
          if (csrVal) {
            volatile float prod = csrVal[p] * br[c];  // one rounding, nothing fused
            t = prod;
          }
          const float v = cr[c];
          const bool better = mn ? !(t >= v) : !(t <= v);
          if (p == a || (v == v && better)) {
            cr[c] = t;
            if (wr) wr[c] = (int)p;
          }
        }
      }
    }
  });
  return SPMM_STATUS_SUCCESS;
} catch (...) {  // no exception leaves the C ABI
  return SPMM_STATUS_ALLOC_FAILED;
}

// Backward: row c of A^T, positions [ta, tb), column j: the selected positions
// (arg[i, j] == perm[q], i = tColInd[q] - base) enter fma(v, dC[i, j], acc) chains under the
// product's piece rule counted over all positions: pieces of max(128, ceil(L / 64)), each
// from +0, added left to right from -0; an empty row is +0. arg is compared, never used as
// an index.
spmm_status_t spmm_csrmm_reduce_bwd_host_f32(int k, int n, int m, int nnz, const int* tRowPtr,
                                             const int* tColInd, const int* perm,
                                             const float* csrVal, spmm_index_base_t base,
                                             const float* dC, int lddc, const int* arg,
                                             int ldarg, float* dB, int lddb) try {
  if (k < 0 || n < 0 || m < 0 || nnz < 0) return SPMM_STATUS_INVALID_VALUE;
  if (base != SPMM_INDEX_BASE_ZERO && base != SPMM_INDEX_BASE_ONE)
    return SPMM_STATUS_INVALID_VALUE;
  if (k == 0 || n == 0) return SPMM_STATUS_SUCCESS;
  if (!tRowPtr || !dB || (nnz > 0 && (!tColInd || !perm || !dC || !arg)))
    return SPMM_STATUS_INVALID_VALUE;
  if (lddc < n || ldarg < n || lddb < n) return SPMM_STATUS_INVALID_VALUE;
  const int ba = (int)base;
  const int64_t p0 = (int64_t)tRowPtr[0] - ba, p1 = (int64_t)tRowPtr[k] - ba;
  if (p0 < 0 || p1 < p0 || p1 > nnz) return SPMM_STATUS_INVALID_VALUE;
  std::atomic<bool> ok{true};
  spmm_host::parallel_for(k, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r)
      if (tRowPtr[r + 1] < tRowPtr[r]) ok = false;
  });
  spmm_host::parallel_for(p1 - p0, [&](int64_t lo, int64_t hi) {
    for (int64_t q = p0 + lo; q < p0 + hi; ++q)
      if (tColInd[q] - ba < 0 || tColInd[q] - ba >= m || perm[q] < 0 || perm[q] >= nnz)
        ok = false;
  });
  if (!ok) return SPMM_STATUS_INVALID_VALUE;
  spmm_host::parallel_for(k, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r) {
      const int64_t a = (int64_t)tRowPtr[r] - ba, b = (int64_t)tRowPtr[r + 1] - ba;
      const int64_t T = std::max<int64_t>(128, (b - a + 63) / 64);
      for (int c = 0; c < n; ++c) {
        volatile float x = b > a ? -0.f : 0.f;  // no reassociation of the piece sums
        for (int64_t s = a; s < b; s += T) {
          float acc = 0.f;
          for (int64_t q = s; q < std::min(s + T, b); ++q) {
            const int64_t i = tColInd[q] - ba;
            if (arg[i * ldarg + c] != perm[q]) continue;
            acc = __builtin_fmaf(csrVal ? csrVal[perm[q]] : 1.f, dC[i * lddc + c], acc);
          }
          x = x + acc;
        }
        dB[r * lddb + c] = x;
      }
    }
  });
  return SPMM_STATUS_SUCCESS;
} catch (...) {  // no exception leaves the C ABI
  return SPMM_STATUS_ALLOC_FAILED;
}

}  // extern "C"

// ----------------------------------------------------------------------------
// The fp16 / bf16-feature forms of the multi-head sampled product and product (DESIGN.md
// §4k): the rule is the fp32 form's on the widened operands, and that is how it is stated.
// ----------------------------------------------------------------------------
namespace {

// binary16 -> binary32, exact (subnormals included); a NaN comes out quiet, as from the
// hardware's conversion.
inline float widen_f16(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, f = h & 0x3ffu;
  uint32_t u;
  if (e == 0) {
    float v = (float)f * 0x1p-24f;  // f 2^-24: exact
    std::memcpy(&u, &v, 4);
    u |= sign;
  } else if (e == 31) {
    u = sign | 0x7f800000u | (f ? 0x400000u | (f << 13) : 0u);
  } else {
    u = sign | ((e + 112u) << 23) | (f << 13);
  }
  float x;
  std::memcpy(&x, &u, 4);
  return x;
}

// bfloat16 -> binary32: the pattern is the upper half.
inline float widen_bf16(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float x;
  std::memcpy(&x, &u, 4);
  return x;
}

// The first w columns of `rows` rows with leading dimension ld (>= w), widened, at the
// same ld; what lies between the rows is left zero and never read.
std::vector<float> widened(const uint16_t* a, int64_t rows, int64_t ld, int64_t w, bool bf16) {
  std::vector<float> out(rows > 0 && w > 0 ? (size_t)((rows - 1) * ld + w) : 0, 0.f);
  spmm_host::parallel_for(rows, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r)
      for (int64_t c = 0; c < w; ++c)
        out[r * ld + c] = bf16 ? widen_bf16(a[r * ld + c]) : widen_f16(a[r * ld + c]);
  });
  return out;
}

// The fp32 host form's checks up to the point where it reads X and Y (its order), then the
// fp32 host form itself on the widened X and Y: the rest of its checks are its own.
spmm_status_t sddmm_heads_host_half(bool bf16, int m, int d, int k, int nnz, int heads,
                                    float alpha, const int* rp, const int* ci,
                                    spmm_index_base_t base, const uint16_t* X, int ldx,
                                    const uint16_t* Y, int ldy, float beta, float* outVal) {
  if (m < 0 || d < 0 || k < 0 || nnz < 0 || heads < 1) return SPMM_STATUS_INVALID_VALUE;
  if (base != SPMM_INDEX_BASE_ZERO && base != SPMM_INDEX_BASE_ONE)
    return SPMM_STATUS_INVALID_VALUE;
  if (ldx < (int64_t)heads * d || ldy < (int64_t)heads * d) return SPMM_STATUS_INVALID_VALUE;
  if (nnz > 0 && (!rp || !ci || !outVal || (d > 0 && (!X || !Y))))
    return SPMM_STATUS_INVALID_VALUE;
  if (m == 0 || nnz == 0) return SPMM_STATUS_SUCCESS;
  if ((int64_t)nnz * heads > INT32_MAX || d > 1024) return SPMM_STATUS_NOT_SUPPORTED;
  const std::vector<float> Xf = widened(X, m, ldx, (int64_t)heads * d, bf16);
  const std::vector<float> Yf = widened(Y, k, ldy, (int64_t)heads * d, bf16);
  // (d == 0: both copies are empty, and the fp32 form reads neither)
  return spmm_sddmm_csr_heads_host_f32(m, d, k, nnz, heads, alpha, rp, ci, base, Xf.data(), ldx,
                                       Yf.data(), ldy, beta, outVal);
}

spmm_status_t csrmm_heads_host_half(bool bf16, int m, int d, int k, int nnz, int heads,
                                    float alpha, const int* rp, const int* ci, const float* val,
                                    spmm_index_base_t base, const uint16_t* B, int ldb, float beta,
                                    float* C, int ldc) {
  if (m < 0 || d < 0 || k < 0 || nnz < 0 || heads < 1) return SPMM_STATUS_INVALID_VALUE;
  if (base != SPMM_INDEX_BASE_ZERO && base != SPMM_INDEX_BASE_ONE)
    return SPMM_STATUS_INVALID_VALUE;
  if (m == 0 || d == 0) return SPMM_STATUS_SUCCESS;
  if (!rp || !C || (k > 0 && !B) || (nnz > 0 && (!ci || !val))) return SPMM_STATUS_INVALID_VALUE;
  if (ldb < (int64_t)heads * d || ldc < (int64_t)heads * d) return SPMM_STATUS_INVALID_VALUE;
  if ((int64_t)nnz * heads > INT32_MAX) return SPMM_STATUS_NOT_SUPPORTED;
  const std::vector<float> Bf = widened(B, k, ldb, (int64_t)heads * d, bf16);
  // k == 0: B may be null and Bf is empty; the fp32 form then refuses any column index
  return spmm_csrmm_heads_host_f32(m, d, k, nnz, heads, alpha, rp, ci, val, base,
                                   k > 0 ? Bf.data() : nullptr, ldb, beta, C, ldc);
}

}  // namespace

extern "C" {

spmm_status_t spmm_sddmm_csr_heads_host_f16(int m, int d, int k, int nnz, int heads, float alpha,
                                            const int* csrRowPtr, const int* csrColInd,
                                            spmm_index_base_t base, const uint16_t* X, int ldx,
                                            const uint16_t* Y, int ldy, float beta,
                                            float* outVal) try {
  return sddmm_heads_host_half(false, m, d, k, nnz, heads, alpha, csrRowPtr, csrColInd, base, X,
                               ldx, Y, ldy, beta, outVal);
} catch (...) {  // no exception leaves the C ABI
  return SPMM_STATUS_ALLOC_FAILED;
}

spmm_status_t spmm_sddmm_csr_heads_host_bf16(int m, int d, int k, int nnz, int heads, float alpha,
                                             const int* csrRowPtr, const int* csrColInd,
                                             spmm_index_base_t base, const uint16_t* X, int ldx,
                                             const uint16_t* Y, int ldy, float beta,
                                             float* outVal) try {
  return sddmm_heads_host_half(true, m, d, k, nnz, heads, alpha, csrRowPtr, csrColInd, base, X,
                               ldx, Y, ldy, beta, outVal);
} catch (...) {  // no exception leaves the C ABI
  return SPMM_STATUS_ALLOC_FAILED;
}

spmm_status_t spmm_csrmm_heads_host_f16(int m, int d, int k, int nnz, int heads, float alpha,
                                        const int* csrRowPtr, const int* csrColInd,
                                        const float* csrVal, spmm_index_base_t base,
                                        const uint16_t* B, int ldb, float beta, float* C,
                                        int ldc) try {
  return csrmm_heads_host_half(false, m, d, k, nnz, heads, alpha, csrRowPtr, csrColInd, csrVal,
                               base, B, ldb, beta, C, ldc);
} catch (...) {  // no exception leaves the C ABI
  return SPMM_STATUS_ALLOC_FAILED;
}

spmm_status_t spmm_csrmm_heads_host_bf16(int m, int d, int k, int nnz, int heads, float alpha,
                                         const int* csrRowPtr, const int* csrColInd,
                                         const float* csrVal, spmm_index_base_t base,
                                         const uint16_t* B, int ldb, float beta, float* C,
                                         int ldc) try {
  return csrmm_heads_host_half(true, m, d, k, nnz, heads, alpha, csrRowPtr, csrColInd, csrVal,
                               base, B, ldb, beta, C, ldc);
} catch (...) {  // no exception leaves the C ABI
  return SPMM_STATUS_ALLOC_FAILED;
}

}  // extern "C"

// ----------------------------------------------------------------------------
// divide_matrix (divide.cu:52-127) with values.
// ----------------------------------------------------------------------------
namespace {

// Per block row: entry counts per block column (over the block row's rows),
// and the admitted block columns in ascending order. `cnt` has nb entries,
// zero on entry and on exit; `touched` lists the columns with a count.
struct DivideScratch {
  std::vector<int> cnt, touched, slot;
  explicit DivideScratch(int nb) : cnt(std::max(nb, 1), 0), slot(std::max(nb, 1), -1) {}
};

// Returns false on an out-of-range column. Fills `adm` with the admitted
// block columns (ascending).
bool divide_block_row(int br, int bs, int n, int nb, const int* rowptr, const int* colind,
                      int base, float density, DivideScratch& s, std::vector<int>& adm) {
  adm.clear();
  s.touched.clear();
  const int r0 = br * bs, r1 = std::min(n, r0 + bs);
  for (int r = r0; r < r1; ++r)
    for (int j = rowptr[r] - base; j < rowptr[r + 1] - base; ++j) {
      const int c = colind[j] - base;
      if (c < 0 || c / bs >= nb) {
        for (int t : s.touched) s.cnt[t] = 0;
        return false;
      }
      if (s.cnt[c / bs]++ == 0) s.touched.push_back(c / bs);
    }
  const double bnum = (double)bs * bs;
  if (density <= 0.f) {
    // 0 >= 0: every block column is admitted, empty ones included (divide.cu:91).
    for (int bc = 0; bc < nb; ++bc) adm.push_back(bc);
  } else {
    for (int bc : s.touched)
      if ((float)(s.cnt[bc] / bnum) >= density) adm.push_back(bc);
    std::sort(adm.begin(), adm.end());
  }
  for (int t : s.touched) s.cnt[t] = 0;
  return true;
}

}  // namespace

extern "C" {

spmm_status_t spmm_divide_nnz(int n, const int* rowPtr, const int* colInd, int blockDim,
                              float density, int* csrRowPtr, int* bsrRowPtr, int* csrNnz,
                              int* nnzb) try {
  if (n < 0 || blockDim <= 0) return SPMM_STATUS_INVALID_VALUE;
  if (!rowPtr || !csrRowPtr || !bsrRowPtr || !csrNnz || !nnzb) return SPMM_STATUS_INVALID_VALUE;
  const int bs = blockDim, nb = ceil_div(n, bs), mb = nb;
  const int base = n > 0 ? rowPtr[0] : 0;
  if (n > 0 && rowPtr[n] - base > 0 && !colInd) return SPMM_STATUS_INVALID_VALUE;
  // Per block row (worker threads): admitted blocks, and per CSR row the
  // entries left to the remainder (stored in csrRowPtr[r + 1], summed below).
  std::vector<int> nb_row(mb);
  std::atomic<bool> ok{true};
  spmm_host::parallel_for(mb, [&](int64_t lo, int64_t hi) {
    DivideScratch s(nb);
    std::vector<int> adm;
    for (int64_t br = lo; br < hi && ok; ++br) {
      if (!divide_block_row((int)br, bs, n, nb, rowPtr, colInd, base, density, s, adm)) {
        ok = false;
        return;
      }
      nb_row[br] = (int)adm.size();
      for (int bc : adm) s.slot[bc] = 1;
      const int r0 = (int)br * bs, r1 = std::min(n, r0 + bs);
      for (int r = r0; r < r1; ++r) {
        int c = 0;
        for (int j = rowPtr[r] - base; j < rowPtr[r + 1] - base; ++j)
          if (s.slot[(colInd[j] - base) / bs] < 0) ++c;
        csrRowPtr[r + 1] = c;
      }
      for (int bc : adm) s.slot[bc] = -1;
    }
  });
  if (!ok) return SPMM_STATUS_INVALID_VALUE;
  long long nb_acc = 0, c_acc = 0;
  csrRowPtr[0] = 0;
  bsrRowPtr[0] = 0;
  for (int r = 0; r < n; ++r) {
    c_acc += csrRowPtr[r + 1];
    if (c_acc > INT32_MAX) return SPMM_STATUS_INVALID_VALUE;
    csrRowPtr[r + 1] = (int)c_acc;
  }
  for (int br = 0; br < mb; ++br) {
    nb_acc += nb_row[br];
    if (nb_acc > INT32_MAX) return SPMM_STATUS_INVALID_VALUE;
    bsrRowPtr[br + 1] = (int)nb_acc;
  }
  *csrNnz = (int)c_acc;
  *nnzb = (int)nb_acc;
  return SPMM_STATUS_SUCCESS;
} catch (...) {  // no exception leaves the C ABI
  return SPMM_STATUS_ALLOC_FAILED;
}

spmm_status_t spmm_sdivide(int n, const int* rowPtr, const int* colInd, const float* val,
                           int blockDim, float density, const int* csrRowPtr,
                           const int* bsrRowPtr, int* csrColInd, float* csrVal, int* bsrColInd,
                           float* bsrVal) try {
  if (n < 0 || blockDim <= 0) return SPMM_STATUS_INVALID_VALUE;
  if (!rowPtr || !csrRowPtr || !bsrRowPtr) return SPMM_STATUS_INVALID_VALUE;
  const int bs = blockDim, nb = ceil_div(n, bs), mb = nb;
  const int base = n > 0 ? rowPtr[0] : 0;
  if (n > 0 && rowPtr[n] - base > 0 && (!colInd || !val)) return SPMM_STATUS_INVALID_VALUE;
  if ((csrRowPtr[n] > 0 && (!csrColInd || !csrVal)) ||
      (bsrRowPtr[mb] > 0 && (!bsrColInd || !bsrVal)))
    return SPMM_STATUS_INVALID_VALUE;
  const size_t bs2 = (size_t)bs * bs;
  std::atomic<bool> ok{true};
  spmm_host::parallel_for(mb, [&](int64_t lo, int64_t hi) {
    DivideScratch s(nb);
    std::vector<int> adm;
    for (int64_t br = lo; br < hi && ok; ++br) {
      if (!divide_block_row((int)br, bs, n, nb, rowPtr, colInd, base, density, s, adm)) {
        ok = false;
        return;
      }
      const int k0 = bsrRowPtr[br];
      if (bsrRowPtr[br + 1] - k0 != (int)adm.size()) {
        ok = false;
        return;
      }
      for (size_t t = 0; t < adm.size(); ++t) {
        bsrColInd[k0 + t] = adm[t];
        s.slot[adm[t]] = k0 + (int)t;
      }
      if (!adm.empty())
        std::memset(bsrVal + (size_t)k0 * bs2, 0, adm.size() * bs2 * sizeof(float));
      const int r0 = (int)br * bs, r1 = std::min(n, r0 + bs);
      for (int r = r0; r < r1; ++r) {
        int pos = csrRowPtr[r];
        for (int j = rowPtr[r] - base; j < rowPtr[r + 1] - base; ++j) {
          const int c = colInd[j] - base;
          const int k = s.slot[c / bs];
          if (k < 0) {
            csrColInd[pos] = c;
            csrVal[pos] = val[j];
            ++pos;
          } else {
            bsrVal[(size_t)k * bs2 + (size_t)(r - r0) * bs + c % bs] += val[j];
          }
        }
        if (pos != csrRowPtr[r + 1]) ok = false;
      }
      for (int bc : adm) s.slot[bc] = -1;
    }
  });
  return ok ? SPMM_STATUS_SUCCESS : SPMM_STATUS_INVALID_VALUE;
} catch (...) {  // no exception leaves the C ABI
  return SPMM_STATUS_ALLOC_FAILED;
}

spmm_status_t spmm_hybrid_plan(int n, const int* rowPtr, const int* colInd, int blockDim, int K,
                               int valueBytes, double bsrBytesPerSec, double csrBytesPerSec,
                               float* density, int64_t* nnzb, int64_t* csrNnz,
                               double* estSeconds) try {
  if (n < 0 || blockDim <= 0 || K <= 0 || valueBytes <= 0 || !rowPtr || !density)
    return SPMM_STATUS_INVALID_VALUE;
  const int bs = blockDim, nb = ceil_div(n, bs);
  const int64_t bs2 = (int64_t)bs * bs;
  const int base = n > 0 ? rowPtr[0] : 0;
  if (n > 0 && rowPtr[n] - base > 0 && !colInd) return SPMM_STATUS_INVALID_VALUE;
  const double bw_b = bsrBytesPerSec > 0 ? bsrBytesPerSec : 7.0e12;
  const double bw_c = csrBytesPerSec > 0 ? csrBytesPerSec : 7.5e12;
  // hist[c] = number of blocks holding c entries (c = 1 .. bs^2; duplicates
  // counted, as divide_matrix counts them).
  const int nt = spmm_host::num_threads();
  std::vector<std::vector<int64_t>> hist(nt, std::vector<int64_t>(bs2 + 1, 0));
  std::atomic<bool> ok{true};
  spmm_host::run_workers(nt, [&](int t) {
    DivideScratch s(nb);
    auto& h = hist[t];
    for (int br = (int)((int64_t)nb * t / nt); br < (int)((int64_t)nb * (t + 1) / nt); ++br) {
      s.touched.clear();
      const int r0 = br * bs, r1 = std::min(n, r0 + bs);
      for (int r = r0; r < r1; ++r)
        for (int j = rowPtr[r] - base; j < rowPtr[r + 1] - base; ++j) {
          const int c = colInd[j] - base;
          if (c < 0 || c / bs >= nb) {
            ok = false;
            for (int x : s.touched) s.cnt[x] = 0;
            return;
          }
          if (s.cnt[c / bs]++ == 0) s.touched.push_back(c / bs);
        }
      for (int x : s.touched) {
        ++h[std::min<int64_t>(s.cnt[x], bs2)];
        s.cnt[x] = 0;
      }
    }
  });
  if (!ok) return SPMM_STATUS_INVALID_VALUE;
  for (int t = 1; t < nt; ++t)
    for (int64_t c = 0; c <= bs2; ++c) hist[0][c] += hist[t][c];
  const auto& h = hist[0];
  const double tb = ((double)valueBytes * (bs2 + (double)bs * K) + 4.0) / bw_b;
  const double tn = (8.0 + 4.0 * K) / bw_c;
  // T = bs^2 + 1 (all CSR) first; lowering T moves the blocks of fill T - 1
  // from the CSR side to the BSR side.
  int64_t total_nnz = 0;
  for (int64_t c = 1; c <= bs2; ++c) total_nnz += c * h[c];
  double cost = total_nnz * tn, best = cost;
  int64_t bestT = bs2 + 1, blocks = 0, rem = total_nnz, best_blocks = 0, best_rem = rem;
  for (int64_t T = bs2; T >= 1; --T) {
    cost += h[T] * (tb - T * tn);
    blocks += h[T];
    rem -= T * h[T];
    if (cost < best) {
      best = cost;
      bestT = T;
      best_blocks = blocks;
      best_rem = rem;
    }
  }
  *density = (float)((double)bestT / (double)bs2);
  if (nnzb) *nnzb = best_blocks;
  if (csrNnz) *csrNnz = best_rem;
  if (estSeconds) *estSeconds = best;
  return SPMM_STATUS_SUCCESS;
} catch (...) {  // no exception leaves the C ABI
  return SPMM_STATUS_ALLOC_FAILED;
}

}  // extern "C"

