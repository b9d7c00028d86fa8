// heads_kernels.hip — the three ops of a graph attention layer over `heads` heads in one
// launch each: spmm_sddmm_csr_heads_f32, spmm_edge_softmax_csr_heads_f32 /
// _bwd_csr_heads_f32 and spmm_csrmm_heads_f32. No reference counterpart.
//
// Layouts: per-edge values are [nnz, heads] (element (p, h) at p * heads + h), per-node
// features are row-major [rows, ld] with head h in the columns [h d, (h + 1) d).
//
// The contract is per head the written rule of the single-head entry: §4h's chains and
// butterfly with G(d) lanes (sampled product), §4i's EXP, pieces of 1024, 64 chains and
// butterfly (edge softmax and its backward), §3c's pieces of max(128, ceil(L / 64))
// nonzeros added left to right from -0 (product). Heads never mix, and the bits do not
// depend on heads, the grid, ld or the operands' alignment.
//
//   Sampled product: sddmm_kernel's scheme (sddmm_kernels.hip) over the virtual positions
//   q = p * heads + h, G(d) lanes per q, h fastest across the lane groups of a step, so
//   that the groups of a step read adjacent slices of one Y row.
//   Edge softmax: edge_softmax_kernel's two phases (softmax_kernels.hip) over the virtual
//   rows v = r * heads + h with element stride heads: adjacent lane groups take adjacent
//   heads of one row, and a long row is done head after head by its workgroup.
//   Product: a lane owns VEC adjacent columns of one head in a tile of 64 VEC columns
//   (blockIdx.y), the column index is wave-uniform (v_readlane of a coalesced index load),
//   the B row is one coalesced load and the value is the lane's own val[p, h]; 8 nonzeros
//   are in flight. Waves take equal shares of the merge path of rows and nonzeros and own
//   the rows that start in it: a one-piece row is summed by its wave, a longer one by the
//   owning workgroup, pieces round-robin over its waves, piece sums meeting in LDS behind
//   a barrier and added in piece order. A hub row costs its own length over one workgroup.
// No workspace, no atomics, no polling; every loop is bounded by m or nnz; positions are
// clamped to [0, nnz] and rows to [0, m). The text of the sampled product and of the product
// is heads_impl.hpp's, shared with the fp16 / bf16 forms (heads_half_kernels.hip) and
// instantiated here for float; the body of a softmax row is softmax_impl.hpp's, shared with
// the single-head kernel, and this file holds the loop over virtual rows around it. The
// helpers of all of them (the walk, the folds, the launch) are csr_rows.hpp's.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "context.hpp"
#include "heads_impl.hpp"
#include "launch_record.hpp"
#include "softmax_impl.hpp"

namespace {

// ------------------------------------------------------------------ sampled product
// (sddmm_heads_kernel<float, G, VEC>: heads_impl.hpp)
// d == 0: every dot is +0.
__global__ __launch_bounds__(kWG) void sddmm_heads_zero_kernel(int m, int nnz, int heads,
                                                               const int* __restrict__ rowptr,
                                                               int base, float alpha, float beta,
                                                               float* out) {
  const long long q0 = max((long long)rowptr[0] - base, 0ll) * heads;
  const long long q1 = min((long long)rowptr[m] - base, (long long)nnz) * heads;
  for (long long q = q0 + (long long)blockIdx.x * kWG + threadIdx.x; q < q1;
       q += (long long)gridDim.x * kWG)
    out[q] = epilogue(0.f, alpha, beta, out + q);
}

// ------------------------------------------------------------------ edge softmax
// (chain, result and long_row: softmax_impl.hpp, at element stride heads)
// BWD false: u = x, v unused, o = y.  BWD true: u = y, v = g, o = gx. All [nnz, heads].
template <int G, bool BWD>
__global__ __launch_bounds__(kWG) void edge_softmax_heads_kernel(int m, int nnz, int heads,
                                                                 const int* __restrict__ rowptr,
                                                                 int base, const float* u,
                                                                 const float* v, float* o) {
  constexpr int NB = kWave / G;  // virtual rows of a batch, and chains of a lane
  __shared__ int s_rows[2];
  __shared__ unsigned s_mask[2 * kWavesPerWG];
  __shared__ float s_sums[kRound];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sub = lane & (G - 1), grp = lane / G;
  const Strided at{(size_t)heads};

  const Rows wr = wave_rows(rowptr, m, base, nnz, wave);
  if (tid == 0) s_rows[0] = wr.r0;
  if (tid == kWG - 1) s_rows[1] = wr.r1;

  // short rows: the virtual rows v = r * heads + h of the wave's rows, h fastest
  const long long v0 = (long long)wr.r0 * heads, v1 = (long long)wr.r1 * heads;
  for (long long vb = v0; vb < v1; vb += NB) {  // wave-uniform
    const long long vr = min(vb + grp, v1 - 1);
    const int r = (int)(vr / heads);
    const int h = (int)(vr - (long long)r * heads);
    const long long a = row_pos(rowptr, r, base, nnz);
    const long long len = row_pos(rowptr, r + 1, base, nnz) - a;
    const unsigned L = vb + grp < v1 && len > 0 && len <= kPiece ? (unsigned)len : 0u;
    const size_t off = (size_t)a * at.heads + h;
    const float* ur = u + off;
    const float* vp = v + off;
    float* orow = o + off;
    // (edge_softmax_kernel's lane-group body at stride heads: softmax_impl.hpp says why
    // the two are not one function)
    float mx = -__builtin_inff();
    if constexpr (!BWD) {
      for (unsigned q = sub; q < L; q += G) mx = fmaxf(mx, ur[at(q)]);
      mx = group_fold<G, true>(mx);
    }
    float acc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[j] = 0.f;
    for (unsigned q0 = 0; q0 < L; q0 += kWave) {
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const unsigned q = q0 + G * j + sub;
        if (q < L) acc[j] = chain<BWD>(acc[j], ur, vp, at(q), mx);
      }
    }
    // chains G j .. G j + G - 1 across the lanes, then the tree over j in registers
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[j] = group_fold<G, false>(acc[j]);
#pragma unroll
    for (int wd = NB; wd > 1; wd >>= 1)
#pragma unroll
      for (int j = 0; j < wd / 2; ++j) acc[j] = acc[2 * j] + acc[2 * j + 1];
    const float s = acc[0];
    for (unsigned q = sub; q < L; q += G) orow[at(q)] = result<BWD>(ur, vp, at(q), mx, s);
  }

  // long rows of the workgroup's range, each head by all four waves
  __syncthreads();
  for_long_rows(rowptr, m, base, nnz, s_rows[0], s_rows[1], kPiece, s_mask,
                [&](int, long long a, long long b) {
                  for (int h = 0; h < heads; ++h) {
                    const size_t off = (size_t)a * at.heads + h;
                    long_row<BWD>(u + off, v + off, o + off, (unsigned)(b - a), at, s_sums);
                  }
                });
}

// ------------------------------------------------------------------ product
// (csrmm_heads_kernel<float, VEC>: heads_impl.hpp)

// ------------------------------------------------------------------ launchers' choice
using SoftmaxKernel = void (*)(int, int, int, const int*, int, const float*, const float*, float*);
template <bool BWD>
Picked<SoftmaxKernel> pick_softmax(int G) {
  if (G == 4) return picked<edge_softmax_heads_kernel<4, BWD>>();
  if (G == 16) return picked<edge_softmax_heads_kernel<16, BWD>>();
  return picked<edge_softmax_heads_kernel<64, BWD>>();
}

}  // namespace

namespace spmm {

spmm_status_t launch_sddmm_heads(spmm_context* ctx, int m, int d, int nnz, int heads,
                                 const int* rowptr, const int* colind, int base, const float* X,
                                 int ldx, const float* Y, int ldy, float alpha, float beta,
                                 float* out) {
  if (d == 0) {
    const long long vnnz = (long long)nnz * heads;
    const unsigned zgrid = (unsigned)std::min<long long>((vnnz + kWG - 1) / kWG, 65536);
    const int zslot = timing_begin(ctx);
    SPMM_LAUNCH(ctx, sddmm_heads_zero_kernel, dim3(zgrid), dim3(kWG), 0, m, nnz, heads, rowptr,
                base, alpha, beta, out);
    timing_end(ctx, zslot);
    return from_hip(hipGetLastError());
  }
  return launch_sddmm_heads_of<float>(ctx, m, d, nnz, heads, rowptr, colind, base, X, ldx, Y, ldy,
                                      alpha, beta, out);
}

spmm_status_t launch_edge_softmax_heads(spmm_context* ctx, bool bwd, int m, int nnz, int heads,
                                        const int* rowptr, int base, const float* u,
                                        const float* v, float* o) {
  const int G = softmax_group_lanes(m, nnz);
  // the share is the kernel's own, from the row pointer's count; a wave's items carry
  // heads elements each
  const unsigned grid = merge_grid(ctx, (long long)m + nnz,
                                   std::max<long long>(kSoftmaxItemsPerWave / heads, 64));
  return launch_picked(ctx, bwd ? pick_softmax<true>(G) : pick_softmax<false>(G), dim3(grid),
                       dim3(kWG), m, nnz, heads, rowptr, base, u, v, o);
}

spmm_status_t launch_csrmm_heads(spmm_context* ctx, int m, int d, int nnz, int heads,
                                 const int* rowptr, const int* colind, const float* val, int base,
                                 const float* B, int ldb, float alpha, float beta, float* C,
                                 int ldc) {
  return launch_csrmm_heads_of<float>(ctx, m, d, nnz, heads, rowptr, colind, val, base, B, ldb,
                                      alpha, beta, C, ldc);
}

}  // namespace spmm
