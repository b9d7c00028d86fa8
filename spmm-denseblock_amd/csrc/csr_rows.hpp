// csr_rows.hpp — what the graph kernels over CSR rows share: the sampled product
// (sddmm_kernels.hip), the edge softmax (softmax_kernels.hip, softmax_impl.hpp), their
// multi-head and fp16 / bf16 forms (heads_kernels.hip, heads_half_kernels.hip,
// heads_impl.hpp) and the max / min reducers (reduce_kernels.hip). Four groups:
//   wave primitives  the DPP moves, the two butterflies (group_fold, fold) and settle;
//   the CSR walk     which rows a wave owns (wave_rows), how a position is clamped when the
//                    row pointer is bad (row_pos), the workgroup's long rows
//                    (for_long_rows), the sampled product's share of positions
//                    (wave_share, find_row) and its epilogue;
//   column loads     the widening of fp16 / bf16 and the sampled products' chunk of four;
//   launch side      a kernel picked at run time and its launch, the merge-path grid and
//                    the lanes per row or position.
// They decide which lane sums what in which order, that is the bits of every entry above,
// so each exists once, here. Everything is in the including file's anonymous namespace.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "context.hpp"
#include "launch_record.hpp"

namespace {

// ------------------------------------------------------------------ wave primitives
constexpr int kWave = 64;
constexpr int kWG = 256;
constexpr int kWavesPerWG = kWG / kWave;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

template <int CTRL>
__device__ __forceinline__ float dpp(float x) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, false));
}

// x of lane (l xor S). Every lane of the wave must be active.
template <int S>
__device__ __forceinline__ float from_xor(float x) {
  if constexpr (S == 1) return dpp<0xB1>(x);        // quad_perm:[1,0,3,2]
  else if constexpr (S == 2) return dpp<0x4E>(x);   // quad_perm:[2,3,0,1]
  else if constexpr (S == 8) return dpp<0x128>(x);  // row_ror:8, l - 8 mod 16 == l xor 8
  else return __shfl_xor(x, S);
}

// The butterfly over the G lanes of a group, complete in every lane (addition and max
// commute, so both sides of a pair hold the same bits).
template <int G, bool MAX, int S = 1>
__device__ __forceinline__ float group_fold(float x) {
  if constexpr (S < G) {
    const float o = from_xor<S>(x);
    return group_fold<G, MAX, 2 * S>(MAX ? fmaxf(x, o) : x + o);
  } else {
    return x;
  }
}

// x from lane (l - N) mod 16 of the same 16-lane row (DPP row_ror:N).
template <int N>
__device__ __forceinline__ float dpp_ror(float x) {
  return dpp<0x120 + N>(x);
}

// The butterfly sum of the G chains of a lane group, complete in the group's last lane
// (lane % G == G - 1): after the rotations by 1, 2, ..., s / 2 a lane whose low bits are
// all ones holds (its half) + (the other half), each half summed the same way, which is
// acc_l + acc_(l xor s) at every level. Every lane of the wave must be active.
template <int G>
__device__ __forceinline__ float fold(float x) {
  if constexpr (G >= 2) x += dpp_ror<1>(x);
  if constexpr (G >= 4) x += dpp_ror<2>(x);
  if constexpr (G >= 8) x += dpp_ror<4>(x);
  if constexpr (G >= 16) x += dpp_ror<8>(x);
  if constexpr (G >= 32) x += __shfl_xor(x, 16);
  if constexpr (G >= 64) x += __shfl_xor(x, 32);
  return x;
}

// Waits for a pending load into `x` right here (the rare reload path), so that the
// common path that merges with it after the branch does not inherit a full wait.
template <typename T>
__device__ __forceinline__ void settle(T& x) {
  asm volatile("" : "+v"(x));
}

// ------------------------------------------------------------------ the CSR walk
// Position rowptr[r] - base, clamped to what the value arrays hold.
__device__ __forceinline__ long long row_pos(const int* __restrict__ rowptr, int r, int base,
                                             int nnz) {
  return min(max((long long)rowptr[r] - base, 0ll), (long long)nnz);
}

// The first row in [0, m] whose merge-path coordinate r + row_pos(r) reaches t.
__device__ __forceinline__ int first_row(const int* __restrict__ rowptr, int m, int base, int nnz,
                                         long long t) {
  int lo = 0, hi = m;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (mid + row_pos(rowptr, mid, base, nnz) >= t) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// Wave w's rows [r0, r1): those whose merge-path coordinate lies in its equal share of
// the rows + positions of the pattern.
struct Rows {
  int r0, r1;
};
__device__ __forceinline__ Rows wave_rows(const int* __restrict__ rowptr, int m, int base,
                                          int nnz, int wave) {
  const long long p0 = row_pos(rowptr, 0, base, nnz);
  const long long items = (long long)m + max(row_pos(rowptr, m, base, nnz) - p0, 0ll);
  const long long nwaves = (long long)gridDim.x * kWavesPerWG;
  const long long per = (items + nwaves - 1) / nwaves;
  const long long w = (long long)blockIdx.x * kWavesPerWG + wave;
  return {first_row(rowptr, m, base, nnz, p0 + min(w * per, items)),
          first_row(rowptr, m, base, nnz, p0 + min((w + 1) * per, items))};
}

// The workgroup's rows [R0, R1) of length above `limit`, one after the other, each handed
// to f(row, a, b) by every thread (workgroup-uniform arguments). s_mask: 2 kWavesPerWG words.
template <typename F>
__device__ __forceinline__ void for_long_rows(const int* __restrict__ rowptr, int m, int base,
                                              int nnz, int R0, int R1, long long limit,
                                              unsigned* s_mask, F f) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int rb = R0; rb < R1; rb += kWG) {  // workgroup-uniform
    const int r = min(rb + tid, m - 1);
    const long long len = row_pos(rowptr, r + 1, base, nnz) - row_pos(rowptr, r, base, nnz);
    const unsigned long long mk = __ballot(rb + tid < R1 && len > limit);
    if (lane == 0) {
      s_mask[2 * wave] = (unsigned)mk;
      s_mask[2 * wave + 1] = (unsigned)(mk >> 32);
    }
    __syncthreads();
    for (int w = 0; w < 2 * kWavesPerWG; ++w) {
      unsigned bits = __builtin_amdgcn_readfirstlane((int)s_mask[w]);
      while (bits) {
        const int row = rb + 32 * w + __builtin_ctz(bits);
        bits &= bits - 1;
        f(row, row_pos(rowptr, row, base, nnz), row_pos(rowptr, row + 1, base, nnz));
      }
    }
    __syncthreads();
  }
}

// The sampled product's positions of the pattern, clamped to what csrColInd / outVal hold
// (nnz is an int, so a position fits 32 bits, and a position plus a few steps fits an
// unsigned: a share ends at b <= INT_MAX and the last batch reaches at most
// PD * S + 63 < 2^10 positions past it; every such sum in the kernels is an unsigned and is
// clamped to b - 1 as one; held at rowptr[m] - base = INT_MAX by
// tests/test_gpu_far_positions.py), and wave w's share [a, b): whole steps of S positions.
// (sddmm_heads_kernel computes the same share over virtual positions with its own text,
// heads_impl.hpp says why.)
struct Share {
  unsigned a, b;
};
__device__ __forceinline__ Share wave_share(const int* __restrict__ rowptr, int m, int base,
                                            int nnz, int S) {
  const long long w = (long long)blockIdx.x * kWavesPerWG +
                      __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long nwaves = (long long)gridDim.x * kWavesPerWG;
  const long long p0 = max((long long)rowptr[0] - base, 0ll);
  const long long p1 = min((long long)rowptr[m] - base, (long long)nnz);
  if (p1 <= p0) return {0u, 0u};
  const long long steps = (p1 - p0 + S - 1) / S;
  const long long per = (steps + nwaves - 1) / nwaves;
  const long long a = p0 + min(w * per, steps) * S;
  return {(unsigned)min(a, p1), (unsigned)min(a + per * S, p1)};
}

// The row of position p (the last row that starts at or before it), in [0, m - 1].
__device__ __forceinline__ int find_row(const int* __restrict__ rowptr, int m, int base,
                                        long long p) {
  int lo = 0, hi = m - 1;
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if ((long long)rowptr[mid] - base <= p) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ float epilogue(float d, float alpha, float beta, const float* op) {
  return beta == 0.f ? alpha * d : __builtin_fmaf(beta, *op, alpha * d);
}

// ------------------------------------------------------------------ column loads
// Builtin types, so that a kernel's template arguments stay literals and builtin types in
// its symbol (tests/kernel_keys.py reads them): bf16_t is the bit pattern of a bfloat16.
using f16_t = _Float16;
using bf16_t = unsigned short;

// One element, and the two elements of a packed pair (little endian: the lower half is
// the lower column). binary16 goes through the conversion (v_cvt_f32_f16), bfloat16 is the
// upper half of the binary32 with the same value: a 16-bit shift, or a mask for the upper
// element of a pair. Both are exact for every finite value, subnormals included, keep
// the sign of zero and of infinity, and keep a NaN a NaN.
__device__ __forceinline__ float widen(float x) { return x; }
__device__ __forceinline__ float widen(f16_t x) { return (float)x; }
__device__ __forceinline__ float widen(bf16_t x) {
  return __builtin_bit_cast(float, (unsigned)x << 16);
}
template <typename T>
__device__ __forceinline__ float widen_lo(unsigned w) {
  if constexpr (std::is_same_v<T, f16_t>)
    return (float)__builtin_bit_cast(f16_t, (unsigned short)(w & 0xffffu));
  else
    return __builtin_bit_cast(float, w << 16);
}
template <typename T>
__device__ __forceinline__ float widen_hi(unsigned w) {
  if constexpr (std::is_same_v<T, f16_t>)
    return (float)__builtin_bit_cast(f16_t, (unsigned short)(w >> 16));
  else
    return __builtin_bit_cast(float, w & 0xffff0000u);
}

// Columns c0 .. c0 + 3 of a row (of a head's slice) of n > 0 columns, widened, without a
// branch, so that the loads of several steps stay in flight together. VEC (n % 4 == 0,
// bases aligned to four elements, ld % 4 == 0: a chunk is whole or empty): one load of four
// elements (a dwordx4 of floats, a dwordx2 of 16-bit elements), an empty chunk reading the
// row's last one instead. Otherwise one load per column, a column from n on reading column
// n - 1 instead. What is read in place of a missing column is never summed (chain4).
// FULL: n is a multiple of 4 G, so every lane's chunks are whole and nothing is clamped.
template <typename T, bool VEC, bool FULL>
__device__ __forceinline__ f32x4 load4(const T* __restrict__ row, int c0, int n) {
  if constexpr (VEC && std::is_same_v<T, float>) {
    return *reinterpret_cast<const f32x4*>(row + (FULL ? c0 : min(c0, n - 4)));
  } else if constexpr (VEC) {
    const u32x2 t = *reinterpret_cast<const u32x2*>(row + (FULL ? c0 : min(c0, n - 4)));
    return f32x4{widen_lo<T>(t[0]), widen_hi<T>(t[0]), widen_lo<T>(t[1]), widen_hi<T>(t[1])};
  } else {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = widen(row[FULL ? c0 + e : min(c0 + e, n - 1)]);
    return v;
  }
}

template <bool FULL>
__device__ __forceinline__ float chain4(float acc, const f32x4& x, const f32x4& y, int c0, int n) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (FULL || c0 + e < n) acc = __builtin_fmaf(x[e], y[e], acc);
  return acc;
}

// ------------------------------------------------------------------ launch side
// A kernel chosen at run time, with its launch-record identifier (launch_record.hpp).
template <typename K>
struct Picked {
  K fn;
  const char* id;
};
template <auto K>
Picked<decltype(K)> picked() {
  return {K, spmm::launch_id<K>()};
}

// The one launch of a picked kernel on the handle's stream: its timing slot, its launch
// record, and the launch's own status.
template <typename K, typename... Args>
spmm_status_t launch_picked(spmm_context* ctx, const Picked<K>& kern, dim3 grid, dim3 block,
                            Args... args) {
  const int slot = spmm::timing_begin(ctx);
  spmm::note_launch(ctx, kern.id);
  hipLaunchKernelGGL(kern.fn, grid, block, 0, ctx->stream, args...);
  spmm::timing_end(ctx, slot);
  return spmm::from_hip(hipGetLastError());
}

// waves for `items` merge-path items at `per` items a wave, at most 32 waves per CU;
// spmm_set_csr_waves_per_cu sets the wave count itself (at least one item each)
inline unsigned merge_grid(const spmm_context* ctx, long long items, long long per) {
  const long long waves =
      ctx->csr_waves_per_cu > 0
          ? std::min<long long>((long long)ctx->num_cus * ctx->csr_waves_per_cu, items)
          : std::min<long long>((items + per - 1) / per, (long long)ctx->num_cus * 32);
  return (unsigned)((std::max<long long>(waves, 1) + kWavesPerWG - 1) / kWavesPerWG);
}

inline bool aligned(const void* p, uintptr_t bytes) {
  return reinterpret_cast<uintptr_t>(p) % bytes == 0;
}

// the edge softmax's lanes per short row, from the mean row length (m > 0)
inline int softmax_group_lanes(int m, int nnz) {
  const long long mean = ((long long)nnz + m - 1) / m;
  return mean <= 8 ? 4 : mean <= 48 ? 16 : 64;
}

// the sampled product's lanes per position: G(d) = min(64, max(1, pow2ceil(ceil(d / 4))))
inline int sddmm_group_lanes(int d) {
  const int chunks = (d + 3) / 4;
  int g = 1;
  while (g < chunks && g < kWave) g <<= 1;
  return g;
}

}  // namespace
