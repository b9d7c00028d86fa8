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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "context.hpp"
#include "launch_record.hpp"
#include "softmax_rule.hpp"

namespace {

using spmm_rule::softmax_exp;

constexpr int kWave = 64;
constexpr int kWG = 256;
constexpr int kWavesPerWG = kWG / kWave;
constexpr int kPiece = spmm_rule::kSoftmaxPiece;
constexpr int kRound = 32;  // pieces whose sums meet in LDS at one barrier
// merge-path items (rows + positions) a wave is given when the grid is not capped
constexpr int kItemsPerWave = 2048;

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

// Position rowptr[r] - base, clamped to what x / y hold.
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

// One term of a chain: the forward's e = EXP(x - mx) added, the backward's fma(y, g, acc).
template <bool BWD>
__device__ __forceinline__ float chain(float acc, const float* u, const float* v, unsigned q,
                                       float mx) {
  if constexpr (BWD) return __builtin_fmaf(u[q], v[q], acc);
  else return acc + softmax_exp(u[q] - mx);
}

// The output at q from the row's s (the forward's sum, the backward's d).
template <bool BWD>
__device__ __forceinline__ float result(const float* u, const float* v, unsigned q, float mx,
                                        float s) {
  if constexpr (BWD) {
    const float diff = v[q] - s;
    return u[q] * diff;
  } else {
    return softmax_exp(u[q] - mx) / s;
  }
}

// A row of L > kPiece positions by the whole workgroup (every thread calls it with the
// same arguments). sums: kRound floats of LDS.
template <bool BWD>
__device__ void long_row(const float* u, const float* v, float* o, unsigned L, float* sums) {
  const unsigned tid = threadIdx.x, lane = tid & (kWave - 1);
  const unsigned wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
  float mx = -__builtin_inff();
  if constexpr (!BWD) {
    for (unsigned q = tid; q < L; q += kWG) mx = fmaxf(mx, u[q]);
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
        if (q < L) acc = chain<BWD>(acc, u, v, q, mx);
      }
      acc = group_fold<kWave, false>(acc);
      if (lane == 0) sums[P] = acc;
    }
    __syncthreads();
    for (unsigned i = 0; i < cnt; ++i) s += sums[i];
    __syncthreads();
  }
  for (unsigned q = tid; q < L; q += kWG) o[q] = result<BWD>(u, v, q, mx, s);
}

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

  // the wave's rows [wr0, wr1): those whose merge-path coordinate lies in its share
  const long long p0 = row_pos(rowptr, 0, base, nnz);
  const long long items = (long long)m + max(row_pos(rowptr, m, base, nnz) - p0, 0ll);
  const long long nwaves = (long long)gridDim.x * kWavesPerWG;
  const long long per = (items + nwaves - 1) / nwaves;
  const long long w = (long long)blockIdx.x * kWavesPerWG + wave;
  const int wr0 = first_row(rowptr, m, base, nnz, p0 + min(w * per, items));
  const int wr1 = first_row(rowptr, m, base, nnz, p0 + min((w + 1) * per, items));
  if (tid == 0) s_rows[0] = wr0;
  if (tid == kWG - 1) s_rows[1] = wr1;

  // short rows
  for (int rb = wr0; rb < wr1; rb += NB) {  // wave-uniform
    const int r = min(rb + grp, m - 1);
    const long long a = row_pos(rowptr, r, base, nnz);
    const long long len = row_pos(rowptr, r + 1, base, nnz) - a;
    const unsigned L = rb + grp < wr1 && len > 0 && len <= kPiece ? (unsigned)len : 0u;
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

  // long rows of the workgroup's range, each by all four waves
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
        long_row<BWD>(u + a, v + a, o + a, (unsigned)(b - a), s_sums);
      }
    }
    __syncthreads();
  }
}

// lanes per short row from the mean row length
inline int group_lanes(int m, int nnz) {
  const long long mean = ((long long)nnz + m - 1) / m;
  return mean <= 8 ? 4 : mean <= 48 ? 16 : 64;
}

using Kernel = void (*)(int, int, const int*, int, const float*, const float*, float*);
struct Picked {
  Kernel fn;
  const char* id;
};
template <auto K>
Picked picked() {
  return {K, spmm::launch_id<K>()};
}
template <bool BWD>
Picked pick(int G) {
  if (G == 4) return picked<edge_softmax_kernel<4, BWD>>();
  if (G == 16) return picked<edge_softmax_kernel<16, BWD>>();
  return picked<edge_softmax_kernel<64, BWD>>();
}

}  // namespace

namespace spmm {

spmm_status_t launch_edge_softmax(spmm_context* ctx, bool bwd, int m, int nnz, const int* rowptr,
                                  int base, const float* u, const float* v, float* o) {
  const Picked kern = bwd ? pick<true>(group_lanes(m, nnz)) : pick<false>(group_lanes(m, nnz));
  // the share is computed in the kernel from the row pointer's own count; the grid's size
  // cannot reach the output (a row's bits are the row's)
  const long long items = (long long)m + nnz;
  // kItemsPerWave items per wave up to 32 waves per CU; spmm_set_csr_waves_per_cu sets
  // the wave count itself (at least one item each)
  const long long waves =
      ctx->csr_waves_per_cu > 0
          ? std::min<long long>((long long)ctx->num_cus * ctx->csr_waves_per_cu, items)
          : std::min<long long>((items + kItemsPerWave - 1) / kItemsPerWave,
                                (long long)ctx->num_cus * 32);
  const unsigned grid = (unsigned)((waves + kWavesPerWG - 1) / kWavesPerWG);
  const int slot = timing_begin(ctx);
  spmm::note_launch(ctx, kern.id);
  hipLaunchKernelGGL(kern.fn, dim3(grid), dim3(kWG), 0, ctx->stream, m, nnz, rowptr, base, u, v,
                     o);
  timing_end(ctx, slot);
  return from_hip(hipGetLastError());
}

}  // namespace spmm
