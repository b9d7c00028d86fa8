// heads_half_kernels.hip — the multi-head sampled product and CSR product on fp16 and bf16
// per-node features: spmm_sddmm_csr_heads_f16 / _bf16 and
// spmm_csrmm_heads_f16 / _bf16. Edge values, alpha, beta, outVal and C stay fp32.
//
// The kernel text is heads_impl.hpp's, the one heads_kernels.hip instantiates for float:
// the features are widened as they are loaded (binary16 by a conversion, bfloat16 by a
// 16-bit shift of the pattern; both exact, subnormals included) and everything behind the
// loads is the fp32 rule, so the bits are those of the _f32 entries on the widened
// operands: §4h's G(d) chains and butterfly, §3c's pieces at every d. A column's owner lane
// depends on the column index alone; a chunk of four columns is 8 bytes instead of 16.
//   Sampled product: one 8-byte load per chunk when d % 4 == 0, X and Y are 8-byte aligned
//   and ldx % 4 == ldy % 4 == 0, else one 2-byte load per column. d == 0 reads no features
//   and is the fp32 file's fill kernel (api.cpp).
//   Product: VEC in {4, 2, 1} columns per lane as 8 / 4 / 2-byte loads of B; VEC divides d,
//   keeps B's loads and C's fp32 stores aligned and is narrowed so that a tile is not
//   mostly idle (csrmm_heads_vec).
// No workspace, no atomics, one launch per call on the handle's stream.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "context.hpp"
#include "heads_impl.hpp"
#include "launch_record.hpp"

namespace {

// the 16-bit patterns of the C ABI as the storage type the kernels are instantiated for
template <typename T>
const T* as(const uint16_t* p) {
  return reinterpret_cast<const T*>(p);
}

}  // namespace

namespace spmm {

spmm_status_t launch_sddmm_heads_half(spmm_context* ctx, bool bf16, int m, int d, int nnz,
                                      int heads, const int* rowptr, const int* colind, int base,
                                      const uint16_t* X, int ldx, const uint16_t* Y, int ldy,
                                      float alpha, float beta, float* out) {
  if (bf16)
    return launch_sddmm_heads_of<bf16_t>(ctx, m, d, nnz, heads, rowptr, colind, base,
                                         as<bf16_t>(X), ldx, as<bf16_t>(Y), ldy, alpha, beta, out);
  return launch_sddmm_heads_of<f16_t>(ctx, m, d, nnz, heads, rowptr, colind, base, as<f16_t>(X),
                                      ldx, as<f16_t>(Y), ldy, alpha, beta, out);
}

spmm_status_t launch_csrmm_heads_half(spmm_context* ctx, bool bf16, int m, int d, int nnz,
                                      int heads, const int* rowptr, const int* colind,
                                      const float* val, int base, const uint16_t* B, int ldb,
                                      float alpha, float beta, float* C, int ldc) {
  if (bf16)
    return launch_csrmm_heads_of<bf16_t>(ctx, m, d, nnz, heads, rowptr, colind, val, base,
                                         as<bf16_t>(B), ldb, alpha, beta, C, ldc);
  return launch_csrmm_heads_of<f16_t>(ctx, m, d, nnz, heads, rowptr, colind, val, base,
                                      as<f16_t>(B), ldb, alpha, beta, C, ldc);
}

}  // namespace spmm
