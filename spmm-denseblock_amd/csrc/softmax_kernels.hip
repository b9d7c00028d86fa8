// softmax_kernels.hip — softmax over the positions of every CSR row (spmm_edge_softmax_csr_f32:
// DGL's edge_softmax, the attention weights of a graph layer from its edge logits) and its
// backward (spmm_edge_softmax_bwd_csr_f32). No reference counterpart.
//
// The rule, a function of the row's own values alone:
//   forward   mx = max of x over the row, e[p] = EXP(x[p] - mx) (softmax_rule.hpp),
//             s = SUM(e), y[p] = e[p] / s;
//   backward  d = SUM(y[p] * g[p]) with chains acc = fma(y[p], g[p], acc),
//             gx[p] = y[p] * (g[p] - d), the difference and the product rounded apart.
//   SUM: the row is cut into pieces of 1024 positions from its start; in a piece chain c of
//   64 takes the positions = c (mod 64) in ascending order from +0, the chains fold in the
//   butterfly acc_l + acc_(l xor s), s = 1, 2, ..., 32, and the piece sums are added one after
//   the other in ascending order.
//
// One kernel, two phases. A wave takes an equal share of the merge path of rows and
// positions and owns the rows that start in it (two bisections of the row pointer).
//   Short rows (at most one piece): lane groups of G lanes take a row each, G chosen on the
//   host from the mean row length. Lane l of a group holds the chains l, l + G, ... of its
//   row in 64 / G accumulators, which fold across the group's lanes and then in registers:
//   the same tree. Three passes over the row (max, sum, quotient), the second and third
//   from cache. Groups of a wave run rows of different lengths; the folds come after the
//   loops, where every lane is active again.
//   Long rows are left out there and done by the whole workgroup that owns them, one after
//   the other: waves take the pieces of a round of 32 round-robin, the piece sums meet in
//   LDS behind a barrier and every thread adds them in piece order. A hub row costs its
//   own length spread over 256 lanes; nobody waits for another workgroup.
// No workspace, no atomics, no polling; every loop is bounded by m or nnz. Positions are
// clamped to [0, nnz] and rows to [0, m), so that a bad row pointer reads nothing out of
// bounds. y may be x and gx may be g: a position is read and written by one lane, and the
// row's reads of the earlier passes are complete (fold or barrier) before its first store.
// The row walk is csr_rows.hpp's; a chain's term, the output at a position and the long row
// are softmax_impl.hpp's, shared with the multi-head kernel (heads_kernels.hip).
#include <hip/hip_runtime.h>

#include "context.hpp"
#include "csr_rows.hpp"
#include "softmax_impl.hpp"

namespace {

// BWD false: u = x, v unused, o = y.  BWD true: u = y, v = g, o = gx.
template <int G, bool BWD>
__global__ __launch_bounds__(kWG) void edge_softmax_kernel(int m, int nnz,
                                                           const int* __restrict__ rowptr,
                                                           int base, const float* u,
                                                           const float* v, float* o) {
  constexpr int NB = kWave / G;  // rows of a batch, and chains of a lane
  __shared__ int s_rows[2];
  __shared__ unsigned s_mask[2 * kWavesPerWG];
  __shared__ float s_sums[kRound];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sub = lane & (G - 1), grp = lane / G;

  const Rows wr = wave_rows(rowptr, m, base, nnz, wave);
  if (tid == 0) s_rows[0] = wr.r0;
  if (tid == kWG - 1) s_rows[1] = wr.r1;

  // short rows: a lane group takes a row
  for (int rb = wr.r0; rb < wr.r1; rb += NB) {  // wave-uniform
    const int r = min(rb + grp, m - 1);
    const long long a = row_pos(rowptr, r, base, nnz);
    const long long len = row_pos(rowptr, r + 1, base, nnz) - a;
    const unsigned L = rb + grp < wr.r1 && len > 0 && len <= kPiece ? (unsigned)len : 0u;
    const float* ur = u + a;
    const float* vr = v + a;
    float* orow = o + a;
    float mx = -__builtin_inff();
    if constexpr (!BWD) {
      for (unsigned q = sub; q < L; q += G) mx = fmaxf(mx, ur[q]);
      mx = group_fold<G, true>(mx);
    }
    float acc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[j] = 0.f;
    for (unsigned q0 = 0; q0 < L; q0 += kWave) {
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const unsigned q = q0 + G * j + sub;
        if (q < L) acc[j] = chain<BWD>(acc[j], ur, vr, q, mx);
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
    for (unsigned q = sub; q < L; q += G) orow[q] = result<BWD>(ur, vr, q, mx, s);
  }

  // long rows of the workgroup's range, each by all four waves: for_long_rows' walk
  // (csr_rows.hpp), written out here, since through the function every instantiation grows
  // by 11 instructions (it takes the wave index anew) and two of them measured slower
  // (profiles/csr_rows/edge_softmax_for_long_rows/)
  __syncthreads();
  const int R0 = s_rows[0], R1 = s_rows[1];
  for (int rb = R0; rb < R1; rb += kWG) {  // workgroup-uniform
    const int r = min(rb + tid, m - 1);
    const long long len = row_pos(rowptr, r + 1, base, nnz) - row_pos(rowptr, r, base, nnz);
    const unsigned long long mk = __ballot(rb + tid < R1 && len > kPiece);
    if (lane == 0) {
      s_mask[2 * wave] = (unsigned)mk;
      s_mask[2 * wave + 1] = (unsigned)(mk >> 32);
    }
    __syncthreads();
    for (int h = 0; h < 2 * kWavesPerWG; ++h) {
      unsigned bits = __builtin_amdgcn_readfirstlane((int)s_mask[h]);
      while (bits) {
        const int row = rb + 32 * h + __builtin_ctz(bits);
        bits &= bits - 1;
        const long long a = row_pos(rowptr, row, base, nnz);
        const long long b = row_pos(rowptr, row + 1, base, nnz);
        long_row<BWD>(u + a, v + a, o + a, (unsigned)(b - a), Unit{}, s_sums);
      }
    }
    __syncthreads();
  }
}

using Kernel = void (*)(int, int, const int*, int, const float*, const float*, float*);
template <bool BWD>
Picked<Kernel> pick(int G) {
  if (G == 4) return picked<edge_softmax_kernel<4, BWD>>();
  if (G == 16) return picked<edge_softmax_kernel<16, BWD>>();
  return picked<edge_softmax_kernel<64, BWD>>();
}

}  // namespace

namespace spmm {

spmm_status_t launch_edge_softmax(spmm_context* ctx, bool bwd, int m, int nnz, const int* rowptr,
                                  int base, const float* u, const float* v, float* o) {
  const int G = softmax_group_lanes(m, nnz);
  // the share is computed in the kernel from the row pointer's own count; the grid's size
  // cannot reach the output (a row's bits are the row's)
  const unsigned grid = merge_grid(ctx, (long long)m + nnz, kSoftmaxItemsPerWave);
  return launch_picked(ctx, bwd ? pick<true>(G) : pick<false>(G), dim3(grid), dim3(kWG), m, nnz,
                       rowptr, base, u, v, o);
}

}  // namespace spmm
