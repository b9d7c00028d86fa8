// reduce_kernels.hip — the max / min reducers of the CSR product and their backward
// (DESIGN.md §4l): spmm_csrmm_reduce_f32 and spmm_csrmm_reduce_bwd_f32. No reference
// counterpart.
//
// Forward: C[i, j] = t_w and arg[i, j] = w, the winner w of row i's terms
// t_p = val[p] * B[col(p), j] (t_p = B[col(p), j] as stored without val): the lowest NaN
// position if there is one, otherwise the lowest position of the greatest (least) term.
// Ordered by (is-NaN, value, -position) the combine is a commutative monoid, so the bits
// do not depend on how a row is cut: the kernel keeps (value, position) per column and
// always combines a state of lower positions with one of higher positions, which needs no
// comparison of positions at all (an equal value never replaces the holder).
//   The mapping is the multi-head product's (heads_impl.hpp): a lane owns VEC adjacent
//   columns of a tile of 64 VEC columns (blockIdx.y), the column index is wave-uniform
//   (v_readlane of a coalesced index load), the B row is one coalesced load, 8 nonzeros are
//   in flight. Waves take equal shares of the merge path of rows and nonzeros and own the
//   rows that start in it: a row of up to 128 nonzeros is done by its wave, a longer one by
//   the owning workgroup, a quarter of the row per wave, the four states meeting in LDS
//   behind one barrier and combined in wave order.
// Backward: dB = the masked product over A^T: position q of row c of A^T takes part in
// column j when arg[i, j] == perm[q] (i = tColInd[q]); the association is §3c's piece rule
// counted over all positions, so the text is csrmm_heads_kernel's with the select in the
// chain. arg is compared and never used as an index.
// No workspace, no atomics, no polling; every loop is bounded by the row count or nnz;
// positions are clamped to [0, nnz] and rows to [0, m). The merge-path share, the long-row
// walk and the grid are csr_rows.hpp's; the vector loads and stores of a lane's columns
// (Cols) and the piece constants are heads_impl.hpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "context.hpp"
#include "csr_rows.hpp"
#include "heads_impl.hpp"
#include "launch_record.hpp"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));

template <int VEC>
struct Ints {
  int v[VEC];
};

template <int VEC>
__device__ __forceinline__ Ints<VEC> load_ints(const int* p) {
  Ints<VEC> c;
  if constexpr (VEC == 4) {
    const i32x4 t = *reinterpret_cast<const i32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) c.v[e] = t[e];
  } else if constexpr (VEC == 2) {
    const i32x2 t = *reinterpret_cast<const i32x2*>(p);
    c.v[0] = t[0];
    c.v[1] = t[1];
  } else {
    c.v[0] = *p;
  }
  return c;
}

template <int VEC>
__device__ __forceinline__ void store_ints(int* p, const Ints<VEC>& c) {
  if constexpr (VEC == 4) {
    *reinterpret_cast<i32x4*>(p) = i32x4{c.v[0], c.v[1], c.v[2], c.v[3]};
  } else if constexpr (VEC == 2) {
    *reinterpret_cast<i32x2*>(p) = i32x2{c.v[0], c.v[1]};
  } else {
    *p = c.v[0];
  }
}

// ------------------------------------------------------------------ forward
// The winner so far of a lane's VEC columns: its term and its position, p < 0 while no
// position has been seen (the value is then +0, an empty row's result).
template <int VEC>
struct Best {
  float v[VEC];
  int p[VEC];
};

template <int VEC>
__device__ __forceinline__ Best<VEC> no_best() {
  Best<VEC> x;
#pragma unroll
  for (int c = 0; c < VEC; ++c) {
    x.v[c] = 0.f;
    x.p[c] = -1;
  }
  return x;
}

// (t, p) after the holder (v, q), p above q or q < 0: it takes over an empty holder, and a
// holder that is not a NaN when t is a NaN or strictly better under the IEEE comparison
// (an unordered t fails t <= v and t >= v alike).
__device__ __forceinline__ void combine(float& v, int& q, float t, int p, bool mn) {
  const bool better = mn ? !(t >= v) : !(t <= v);
  const bool take = q < 0 || (v == v && better);
  v = take ? t : v;
  q = take ? p : q;
}

// The nonzeros [s, e) (0 <= s < e <= nnz) in ascending order into acc, by one wave with
// every lane active: piece_chain's walk (heads_impl.hpp). A nonzero from e on reads nonzero
// e - 1 again, which changes nothing: a term never replaces its equal, nor a NaN.
template <int VEC>
__device__ __forceinline__ void reduce_chain(Best<VEC>& acc, long long s, long long e,
                                             const int* __restrict__ colind,
                                             const float* __restrict__ val, int base,
                                             const float* __restrict__ Bc, long long ldb,
                                             int lane, bool mn) {
  for (long long c0 = s; c0 < e; c0 += kWave) {  // wave-uniform
    const int jv = colind[min(c0 + lane, e - 1)] - base;
    const int cnt = (int)min((long long)kWave, e - c0);
    for (int i0 = 0; i0 < cnt; i0 += kInFlight) {  // wave-uniform
      float a[kInFlight];
      Cols<VEC> bv[kInFlight];
#pragma unroll
      for (int t = 0; t < kInFlight; ++t) {
        const int i = min(i0 + t, cnt - 1);
        const int j = __builtin_amdgcn_readlane(jv, i);
        a[t] = val ? val[c0 + i] : 1.f;
        bv[t] = load_cols<float, VEC>(Bc + (long long)j * ldb);
      }
#pragma unroll
      for (int t = 0; t < kInFlight; ++t) {
        const int p = (int)c0 + min(i0 + t, cnt - 1);
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
          // one fp32 multiply, nothing to fuse with; without val the term is B's own bits
          const float term = val ? a[t] * bv[t].v[c] : bv[t].v[c];
          combine(acc.v[c], acc.p[c], term, p, mn);
        }
      }
    }
  }
}

template <int VEC>
__device__ __forceinline__ void store_best(float* Cp, int* argp, const Best<VEC>& x) {
  Cols<VEC> o;
  Ints<VEC> w;
#pragma unroll
  for (int c = 0; c < VEC; ++c) {
    o.v[c] = x.v[c];
    w.v[c] = x.p[c];
  }
  store_cols<VEC>(Cp, o);
  if (argp) store_ints<VEC>(argp, w);
}

// n columns in tiles of 64 VEC (blockIdx.y). A lane past the last column works on the last
// VEC columns again and stores nothing, so that every lane is active at the readlanes.
// mn: 0 max, 1 min. arg may be null.
template <int VEC>
__global__ __launch_bounds__(kWG) void csrmm_reduce_kernel(
    int m, int n, int nnz, int mn, const int* __restrict__ rowptr,
    const int* __restrict__ colind, const float* __restrict__ val, int base,
    const float* __restrict__ B, long long ldb, float* C, long long ldc, int* arg,
    long long ldarg) {
  __shared__ int s_rows[2];
  __shared__ unsigned s_mask[2 * kWavesPerWG];
  __shared__ float s_v[kWavesPerWG * VEC * kWave];
  __shared__ int s_p[kWavesPerWG * VEC * kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool is_min = mn != 0;
  const long long cw = (long long)blockIdx.y * (kWave * VEC) + (long long)lane * VEC;
  const bool mine = cw < n;
  const long long col = mine ? cw : (long long)n - VEC;
  const float* Bc = B + col;
  float* Cc = C + col;
  int* argc = arg ? arg + col : nullptr;

  const Rows wr = wave_rows(rowptr, m, base, nnz, wave);
  if (tid == 0) s_rows[0] = wr.r0;
  if (tid == kWG - 1) s_rows[1] = wr.r1;

  // rows of up to kCsrPiece nonzeros (and empty rows), one after the other by the wave
  for (int r = wr.r0; r < wr.r1; ++r) {  // wave-uniform
    const long long a = row_pos(rowptr, r, base, nnz);
    const long long L = row_pos(rowptr, r + 1, base, nnz) - a;
    if (L > kCsrPiece) continue;
    Best<VEC> x = no_best<VEC>();
    if (L > 0) reduce_chain<VEC>(x, a, a + L, colind, val, base, Bc, ldb, lane, is_min);
    if (mine) store_best<VEC>(Cc + (long long)r * ldc, argc ? argc + (long long)r * ldarg : nullptr, x);
  }

  // longer rows, each by the workgroup that owns it: wave w takes the w-th quarter, the
  // four states are combined in wave order, that is in ascending position
  __syncthreads();
  for_long_rows(rowptr, m, base, nnz, s_rows[0], s_rows[1], kCsrPiece, s_mask,
                [&](int row, long long a, long long b) {
                  const long long Q = (b - a + kWavesPerWG - 1) / kWavesPerWG;
                  const long long s = min(a + wave * Q, b), e = min(s + Q, b);
                  Best<VEC> part = no_best<VEC>();
                  if (s < e) reduce_chain<VEC>(part, s, e, colind, val, base, Bc, ldb, lane, is_min);
#pragma unroll
                  for (int c = 0; c < VEC; ++c) {
                    s_v[(wave * VEC + c) * kWave + lane] = part.v[c];
                    s_p[(wave * VEC + c) * kWave + lane] = part.p[c];
                  }
                  __syncthreads();
                  if (wave == 0) {
                    Best<VEC> x = no_best<VEC>();
                    for (int w = 0; w < kWavesPerWG; ++w)
#pragma unroll
                      for (int c = 0; c < VEC; ++c) {
                        const float t = s_v[(w * VEC + c) * kWave + lane];
                        const int p = s_p[(w * VEC + c) * kWave + lane];
                        if (p >= 0) combine(x.v[c], x.p[c], t, p, is_min);
                      }
                    if (mine)
                      store_best<VEC>(Cc + (long long)row * ldc,
                                      argc ? argc + (long long)row * ldarg : nullptr, x);
                  }
                  __syncthreads();
                });
}

// ------------------------------------------------------------------ backward
// The chain acc = sel ? fma(v, dC[i, c], acc) : acc from +0 over the positions [s, e) of
// A^T (0 <= s < e <= nnz), i = tcol[q] - base, sel = (arg[i, c] == perm[q]),
// v = val[perm[q]] or 1: piece_chain's walk with two gathers per position. The row and the
// permuted position are wave-uniform (readlanes of two coalesced loads); perm indexes val
// clamped to [0, nnz), and is compared as it is. A position from e on reads position e - 1
// instead and is dropped by a select.
template <int VEC>
__device__ __forceinline__ Cols<VEC> masked_chain(long long s, long long e,
                                                  const int* __restrict__ tcol,
                                                  const int* __restrict__ perm,
                                                  const float* __restrict__ val, int nnz,
                                                  int base, const float* __restrict__ Gc,
                                                  long long ldg, const int* __restrict__ argc,
                                                  long long ldarg, int lane) {
  Cols<VEC> acc;
#pragma unroll
  for (int c = 0; c < VEC; ++c) acc.v[c] = 0.f;
  for (long long c0 = s; c0 < e; c0 += kWave) {  // wave-uniform
    const long long ql = min(c0 + lane, e - 1);
    const int iv = tcol[ql] - base;
    const int pv = perm[ql];
    const int cnt = (int)min((long long)kWave, e - c0);
    for (int i0 = 0; i0 < cnt; i0 += kInFlight) {  // wave-uniform
      float a[kInFlight];
      int pq[kInFlight];
      Cols<VEC> g[kInFlight];
      Ints<VEC> w[kInFlight];
#pragma unroll
      for (int t = 0; t < kInFlight; ++t) {
        const int i = min(i0 + t, cnt - 1);
        const int r = __builtin_amdgcn_readlane(iv, i);
        pq[t] = __builtin_amdgcn_readlane(pv, i);
        a[t] = val ? val[min(max(pq[t], 0), nnz - 1)] : 1.f;
        g[t] = load_cols<float, VEC>(Gc + (long long)r * ldg);
        w[t] = load_ints<VEC>(argc + (long long)r * ldarg);
      }
#pragma unroll
      for (int t = 0; t < kInFlight; ++t)
        if (i0 + t < cnt) {
#pragma unroll
          for (int c = 0; c < VEC; ++c)
            acc.v[c] = w[t].v[c] == pq[t] ? __builtin_fmaf(a[t], g[t].v[c], acc.v[c]) : acc.v[c];
        }
    }
  }
  return acc;
}

// kt rows of A^T, n columns in tiles of 64 VEC (blockIdx.y); csrmm_heads_kernel's rows and
// pieces with alpha = 1, beta = 0.
template <int VEC>
__global__ __launch_bounds__(kWG) void csrmm_reduce_bwd_kernel(
    int kt, int n, int nnz, const int* __restrict__ trowptr, const int* __restrict__ tcol,
    const int* __restrict__ perm, const float* __restrict__ val, int base,
    const float* __restrict__ dC, long long lddc, const int* __restrict__ arg, long long ldarg,
    float* dB, long long lddb) {
  __shared__ int s_rows[2];
  __shared__ unsigned s_mask[2 * kWavesPerWG];
  __shared__ float s_sums[kCsrRound * VEC * kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long cw = (long long)blockIdx.y * (kWave * VEC) + (long long)lane * VEC;
  const bool mine = cw < n;
  const long long col = mine ? cw : (long long)n - VEC;
  const float* Gc = dC + col;
  const int* argc = arg + col;
  float* Dc = dB + col;

  const Rows wr = wave_rows(trowptr, kt, base, nnz, wave);
  if (tid == 0) s_rows[0] = wr.r0;
  if (tid == kWG - 1) s_rows[1] = wr.r1;

  // rows of one piece (and empty rows), one after the other by the wave
  for (int r = wr.r0; r < wr.r1; ++r) {  // wave-uniform
    const long long a = row_pos(trowptr, r, base, nnz);
    const long long L = row_pos(trowptr, r + 1, base, nnz) - a;
    if (L > kCsrPiece) continue;
    Cols<VEC> x;
    if (L > 0) {
      x = masked_chain<VEC>(a, a + L, tcol, perm, val, nnz, base, Gc, lddc, argc, ldarg, lane);
#pragma unroll
      for (int c = 0; c < VEC; ++c) x.v[c] = -0.f + x.v[c];
    } else {
#pragma unroll
      for (int c = 0; c < VEC; ++c) x.v[c] = 0.f;
    }
    if (mine) store_cols<VEC>(Dc + (long long)r * lddb, x);
  }

  // rows of several pieces, each by the workgroup that owns it: pieces round-robin over
  // the waves, kCsrRound piece sums per barrier, added in piece order from -0
  __syncthreads();
  for_long_rows(trowptr, kt, base, nnz, s_rows[0], s_rows[1], kCsrPiece, s_mask,
                [&](int row, long long a, long long b) {
                  const long long L = b - a;
                  const long long T_ = max((long long)kCsrPiece, (L + kCsrPieces - 1) / kCsrPieces);
                  const int npieces = (int)((L + T_ - 1) / T_);
                  Cols<VEC> x;
#pragma unroll
                  for (int c = 0; c < VEC; ++c) x.v[c] = -0.f;
                  for (int P0 = 0; P0 < npieces; P0 += kCsrRound) {
                    const int cnt = min(kCsrRound, npieces - P0);
                    for (int P = wave; P < cnt; P += kWavesPerWG) {  // wave-uniform
                      const long long s = a + (long long)(P0 + P) * T_;
                      const Cols<VEC> acc = masked_chain<VEC>(s, min(s + T_, b), tcol, perm, val,
                                                              nnz, base, Gc, lddc, argc, ldarg, lane);
#pragma unroll
                      for (int c = 0; c < VEC; ++c) s_sums[(P * VEC + c) * kWave + lane] = acc.v[c];
                    }
                    __syncthreads();
                    for (int P = 0; P < cnt; ++P)
#pragma unroll
                      for (int c = 0; c < VEC; ++c) x.v[c] = x.v[c] + s_sums[(P * VEC + c) * kWave + lane];
                    __syncthreads();
                  }
                  if (wave == 0 && mine) store_cols<VEC>(Dc + (long long)row * lddb, x);
                });
}

// The widest lane a launch may use: it divides n, keeps every vector load and store
// aligned (ptrs: the dense operands, each of 4-byte elements; lds: their leading
// dimensions) and leaves no tile mostly idle.
int reduce_vec(int n, std::initializer_list<const void*> ptrs, std::initializer_list<int> lds) {
  int vec = n > 128 ? 4 : n > 64 ? 2 : 1;
  auto fits = [&](int v) {
    if (n % v) return false;
    for (const void* p : ptrs)
      if (p && !aligned(p, 4 * v)) return false;
    for (int ld : lds)
      if (ld % v) return false;
    return true;
  };
  while (vec > 1 && !fits(vec)) vec >>= 1;
  return vec;
}

}  // namespace

namespace spmm {

spmm_status_t launch_csrmm_reduce(spmm_context* ctx, bool is_min, int m, int n, int nnz,
                                  const int* rowptr, const int* colind, const float* val,
                                  int base, const float* B, int ldb, float* C, int ldc, int* arg,
                                  int ldarg) {
  const int vec = reduce_vec(n, {B, C, arg}, {ldb, ldc, arg ? ldarg : 0});
  const long long ntiles = ((long long)n + kWave * vec - 1) / (kWave * vec);
  if (ntiles > 65535) return SPMM_STATUS_NOT_SUPPORTED;  // the grid's y extent
  const dim3 grid(merge_grid(ctx, (long long)m + nnz, kCsrItemsPerWave), (unsigned)ntiles);
  const int slot = timing_begin(ctx);
  auto go = [&](auto v) {
    constexpr int V = decltype(v)::value;
    SPMM_LAUNCH(ctx, csrmm_reduce_kernel<V>, grid, dim3(kWG), 0, m, n, nnz, (int)is_min, rowptr,
                colind, val, base, B, (long long)ldb, C, (long long)ldc, arg, (long long)ldarg);
  };
  if (vec == 4) go(std::integral_constant<int, 4>{});
  else if (vec == 2) go(std::integral_constant<int, 2>{});
  else go(std::integral_constant<int, 1>{});
  timing_end(ctx, slot);
  return from_hip(hipGetLastError());
}

spmm_status_t launch_csrmm_reduce_bwd(spmm_context* ctx, int kt, int n, int nnz,
                                      const int* trowptr, const int* tcol, const int* perm,
                                      const float* val, int base, const float* dC, int lddc,
                                      const int* arg, int ldarg, float* dB, int lddb) {
  const int vec = reduce_vec(n, {dC, arg, dB}, {lddc, ldarg, lddb});
  const long long ntiles = ((long long)n + kWave * vec - 1) / (kWave * vec);
  if (ntiles > 65535) return SPMM_STATUS_NOT_SUPPORTED;  // the grid's y extent
  const dim3 grid(merge_grid(ctx, (long long)kt + nnz, kCsrItemsPerWave), (unsigned)ntiles);
  const int slot = timing_begin(ctx);
  auto go = [&](auto v) {
    constexpr int V = decltype(v)::value;
    SPMM_LAUNCH(ctx, csrmm_reduce_bwd_kernel<V>, grid, dim3(kWG), 0, kt, n, nnz, trowptr, tcol,
                perm, val, base, dC, (long long)lddc, arg, (long long)ldarg, dB, (long long)lddb);
  };
  if (vec == 4) go(std::integral_constant<int, 4>{});
  else if (vec == 2) go(std::integral_constant<int, 2>{});
  else go(std::integral_constant<int, 1>{});
  timing_end(ctx, slot);
  return from_hip(hipGetLastError());
}

}  // namespace spmm
