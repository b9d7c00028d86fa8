// softmax_impl.hpp — the parts of the edge softmax and of its backward that
// edge_softmax_kernel (softmax_kernels.hip) and edge_softmax_heads_kernel (heads_kernels.hip)
// share: a term of a chain, the output at a position and a long row by the workgroup.
//
// The kernels differ in where position q of a row lies from the row's first element: at q
// in the single-head arrays, at q * heads in the [nnz, heads] ones. That is the policy
// `at`, Unit or Strided, so that each kernel compiles to the text it had written out.
//
// The short row's lane-group body (the max, the 64 / G chains of a lane, the folds, the tree
// and the write-back) stays written out in both kernels. As one function of `at` it reorders
// the instructions of 11 of the 12 kernels (no more registers past the allocation unit, at
// most two more instructions), and measured against the parent build the multi-head
// backward came out slower than the parent's own spread allows
// (profiles/csr_rows/heads_short_row/). Everything is in the including file's anonymous
// namespace.
#pragma once

#include "csr_rows.hpp"
#include "softmax_rule.hpp"

namespace {

using spmm_rule::softmax_exp;

constexpr int kPiece = spmm_rule::kSoftmaxPiece;
constexpr int kRound = 32;  // pieces whose sums meet in LDS at one barrier
// merge-path items (rows + positions) a wave is given when the grid is not capped
constexpr int kSoftmaxItemsPerWave = 2048;

// The element offset of in-row position q.
struct Unit {
  __device__ __forceinline__ unsigned operator()(unsigned q) const { return q; }
};
struct Strided {
  size_t heads;
  __device__ __forceinline__ size_t operator()(unsigned q) const { return q * heads; }
};

// One term of a chain at element e: the forward's e = EXP(x - mx) added, the backward's
// fma(y, g, acc).
template <bool BWD, typename I>
__device__ __forceinline__ float chain(float acc, const float* u, const float* v, I e, float mx) {
  if constexpr (BWD) return __builtin_fmaf(u[e], v[e], acc);
  else return acc + softmax_exp(u[e] - mx);
}

// The output at element e from the row's s (the forward's sum, the backward's d).
template <bool BWD, typename I>
__device__ __forceinline__ float result(const float* u, const float* v, I e, float mx, float s) {
  if constexpr (BWD) {
    const float diff = v[e] - s;
    return u[e] * diff;
  } else {
    return softmax_exp(u[e] - mx) / s;
  }
}

// A row of L > kPiece positions by the whole workgroup (every thread calls it with the
// same arguments). sums: kRound floats of LDS.
template <bool BWD, typename At>
__device__ void long_row(const float* u, const float* v, float* o, unsigned L, At at,
                         float* sums) {
  const unsigned tid = threadIdx.x, lane = tid & (kWave - 1);
  const unsigned wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
  float mx = -__builtin_inff();
  if constexpr (!BWD) {
    for (unsigned q = tid; q < L; q += kWG) mx = fmaxf(mx, u[at(q)]);
    mx = group_fold<kWave, true>(mx);
    if (lane == 0) sums[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(sums[0], sums[1]), fmaxf(sums[2], sums[3]));
    __syncthreads();
  }
  const unsigned npieces = (L + kPiece - 1) / kPiece;
  float s = 0.f;
  for (unsigned P0 = 0; P0 < npieces; P0 += kRound) {
    const unsigned cnt = min((unsigned)kRound, npieces - P0);
    for (unsigned P = wave; P < cnt; P += kWavesPerWG) {  // wave-uniform
      const unsigned q0 = (P0 + P) * kPiece + lane;
      float acc = 0.f;
#pragma unroll 4
      for (int i = 0; i < kPiece / kWave; ++i) {
        const unsigned q = q0 + i * kWave;
        if (q < L) acc = chain<BWD>(acc, u, v, at(q), mx);
      }
      acc = group_fold<kWave, false>(acc);
      if (lane == 0) sums[P] = acc;
    }
    __syncthreads();
    for (unsigned i = 0; i < cnt; ++i) s += sums[i];
    __syncthreads();
  }
  for (unsigned q = tid; q < L; q += kWG) o[at(q)] = result<BWD>(u, v, at(q), mx, s);
}

}  // namespace
