// heads_impl.hpp — the kernel text of the multi-head sampled product and CSR product
// (DESIGN.md §4j, §4k), parameterised by the storage type T of the per-node features:
//   float      heads_kernels.hip       spmm_sddmm_csr_heads_f32 / spmm_csrmm_heads_f32
//   f16_t      heads_half_kernels.hip  ..._f16  (binary16, widened by a conversion)
//   bf16_t     heads_half_kernels.hip  ..._bf16 (bfloat16 bit patterns, widened by a shift)
// Only the multi-head text is here: sddmm_heads_kernel, the product's Cols / load_cols /
// store_cols, piece_chain and csrmm_heads_kernel, and their two launchers. The wave
// primitives, the CSR walk, the widening, the chunk loads and the launch side are
// csr_rows.hpp's, shared with the single-head files and the reducers.
//
// Three places depend on T: load4 (the sampled product's chunk of four columns), load_cols
// (the product's VEC columns of a lane) and the pointer arithmetic, which counts elements
// of T. Both widenings are exact, subnormals included, so everything behind the loads is
// the fp32 text: the walk, the unconditional clamped loads, the select that drops a batch's
// tail, the folds, the piece rounds in LDS, the -0 / +0 conventions and the epilogue. The
// bits are therefore those of the fp32 kernels on the widened operands, at every vector
// width and alignment.
//
// Everything is in the including file's anonymous namespace: a .hip file gets the kernels of
// the types whose launchers (launch_sddmm_heads_of<T>, launch_csrmm_heads_of<T>) it calls.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "context.hpp"
#include "csr_rows.hpp"

namespace {

// ------------------------------------------------------------------ sampled product
// G = G(d) lanes per virtual position q = p * heads + h; a lane holds up to NC chunks of
// four columns (NC > 1 only at G = 64: d up to 1024). nnz * heads fits an int (the entries
// refuse anything more), so a virtual position plus a few steps fits an unsigned: q0, q1 and
// the share's start are long long, a share ends at b <= INT_MAX, and the last batch reaches
// less than 2^10 virtual positions past it, as an unsigned clamped to b - 1 (held at
// nnz * heads = INT_MAX - (INT_MAX mod heads) by tests/test_gpu_far_positions.py).
// ldx, ldy count elements of T.
template <typename T, int G, bool VEC>
__global__ __launch_bounds__(kWG) void sddmm_heads_kernel(
    int m, int d, int nnz, int heads, const int* __restrict__ rowptr,
    const int* __restrict__ colind, int base, const T* __restrict__ X, long long ldx,
    const T* __restrict__ Y, long long ldy, float alpha, float beta, float* out) {
  constexpr int S = kWave / G;          // virtual positions per step
  constexpr int NC = G == 64 ? 4 : 1;   // chunks a lane can hold
  constexpr int PD = G == 64 ? 2 : 4;   // steps whose Y gathers are in flight
  const int lane = threadIdx.x & (kWave - 1);
  const int sub = lane & (G - 1), grp = lane / G;
  const int nc = G == 64 ? (d + 4 * G - 1) / (4 * G) : 1;  // chunks a lane does hold

  // the wave's share [a, b) of the virtual positions: whole steps of S. wave_share's text
  // with a factor heads, kept apart: as one function with the single-head kernels (their
  // early exit, or this one's) either their assembly or this kernel's changes.
  unsigned a, b;
  {
    const long long w = (long long)blockIdx.x * kWavesPerWG +
                        __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long nwaves = (long long)gridDim.x * kWavesPerWG;
    const long long q0 = max((long long)rowptr[0] - base, 0ll) * heads;
    const long long q1 = min((long long)rowptr[m] - base, (long long)nnz) * heads;
    if (q1 <= q0) return;
    const long long steps = (q1 - q0 + S - 1) / S;
    const long long per = (steps + nwaves - 1) / nwaves;
    const long long s0 = q0 + min(w * per, steps) * S;
    a = (unsigned)min(s0, q1);
    b = (unsigned)min(s0 + per * S, q1);
  }
  if (a >= b) return;
  int r = find_row(rowptr, m, base, min(a + grp, b - 1) / (unsigned)heads);
  long long re = (long long)rowptr[r + 1] - base;  // end of row r
  int rx = -1, hx = -1;                            // the (row, head) x[] holds
  f32x4 x[NC];
#pragma unroll
  for (int t = 0; t < NC; ++t) x[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // A step past the share's end (the last batch alone) repeats the share's last virtual
  // position: its loads stay in bounds and unconditional, and nothing is stored.
  const unsigned nsteps = (b - a + S - 1) / S;
  for (unsigned t0 = 0; t0 < nsteps; t0 += PD) {
    unsigned q[PD], p[PD];
    bool ok[PD];
    int j[PD], h[PD], ru[PD];
    f32x4 y[PD][NC];
#pragma unroll
    for (int u = 0; u < PD; ++u) {
      const unsigned qq = a + (t0 + u) * S + grp;
      ok[u] = qq < b;
      q[u] = min(qq, b - 1);
      p[u] = q[u] / (unsigned)heads;
      h[u] = (int)(q[u] - p[u] * (unsigned)heads);
      j[u] = colind[p[u]];
    }
#pragma unroll
    for (int u = 0; u < PD; ++u) {  // the rows: positions ascend with u
      while ((long long)p[u] >= re && r + 1 < m) {
        ++r;
        re = (long long)rowptr[r + 1] - base;
      }
      ru[u] = r;
    }
#pragma unroll
    for (int u = 0; u < PD; ++u) {
      const T* yp = Y + (long long)(j[u] - base) * ldy + (long long)h[u] * d;
#pragma unroll
      for (int t = 0; t < NC; ++t)
        if (t == 0 || t < nc) y[u][t] = load4<T, VEC, false>(yp, 4 * (sub + G * t), d);
    }
#pragma unroll
    for (int u = 0; u < PD; ++u) {
      if (t0 + u < nsteps) {  // wave-uniform: the fold below runs with every lane active
        if (ru[u] != rx || h[u] != hx) {
          rx = ru[u];
          hx = h[u];
          const T* xp = X + (long long)rx * ldx + (long long)hx * d;
#pragma unroll
          for (int t = 0; t < NC; ++t)
            if (t == 0 || t < nc) {
              x[t] = load4<T, VEC, false>(xp, 4 * (sub + G * t), d);
              settle(x[t]);
            }
        }
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < NC; ++t)
          if (t == 0 || t < nc) acc = chain4<false>(acc, x[t], y[u][t], 4 * (sub + G * t), d);
        const float dot = fold<G>(acc);
        if (ok[u] && sub == G - 1) out[q[u]] = epilogue(dot, alpha, beta, out + q[u]);
      }
    }
  }
}

// ------------------------------------------------------------------ product
constexpr int kCsrPiece = 128;   // the least piece length of §3c's rule
constexpr int kCsrPieces = 64;   // and the most pieces of a row
constexpr int kCsrRound = 16;    // pieces whose sums meet in LDS at one barrier
constexpr int kInFlight = 8;     // nonzeros whose gathers are in flight
constexpr int kCsrItemsPerWave = 512;

template <int VEC>
struct Cols {
  float v[VEC];
};

// VEC adjacent columns at p, widened: one load of 4 VEC bytes of floats, of 2 VEC bytes
// of 16-bit elements.
template <typename T, int VEC>
__device__ __forceinline__ Cols<VEC> load_cols(const T* p) {
  Cols<VEC> c;
  if constexpr (std::is_same_v<T, float>) {
    if constexpr (VEC == 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
      for (int e = 0; e < 4; ++e) c.v[e] = t[e];
    } else if constexpr (VEC == 2) {
      const float2 t = *reinterpret_cast<const float2*>(p);
      c.v[0] = t.x;
      c.v[1] = t.y;
    } else {
      c.v[0] = *p;
    }
  } else if constexpr (VEC == 4) {
    const u32x2 t = *reinterpret_cast<const u32x2*>(p);
    c.v[0] = widen_lo<T>(t[0]);
    c.v[1] = widen_hi<T>(t[0]);
    c.v[2] = widen_lo<T>(t[1]);
    c.v[3] = widen_hi<T>(t[1]);
  } else if constexpr (VEC == 2) {
    const unsigned t = *reinterpret_cast<const unsigned*>(p);
    c.v[0] = widen_lo<T>(t);
    c.v[1] = widen_hi<T>(t);
  } else {
    c.v[0] = widen(*p);
  }
  return c;
}

template <int VEC>
__device__ __forceinline__ void store_cols(float* p, const Cols<VEC>& c) {
  if constexpr (VEC == 4) {
    *reinterpret_cast<f32x4*>(p) = f32x4{c.v[0], c.v[1], c.v[2], c.v[3]};
  } else if constexpr (VEC == 2) {
    *reinterpret_cast<float2*>(p) = make_float2(c.v[0], c.v[1]);
  } else {
    *p = c.v[0];
  }
}

// The sequential chain acc = fma(val[p, h], B[col(p), c], acc) from +0 over the nonzeros
// [s, e) (0 <= s < e <= nnz), by one wave with every lane active: the column indices of
// 64 nonzeros are one coalesced load, a nonzero's index is then wave-uniform (readlane);
// the gathers of kInFlight nonzeros are issued together. A nonzero from e on reads
// nonzero e - 1 instead and is dropped by a select.
template <typename T, int VEC>
__device__ __forceinline__ Cols<VEC> piece_chain(long long s, long long e,
                                                 const int* __restrict__ colind,
                                                 const float* __restrict__ vh, long long heads,
                                                 int base, const T* __restrict__ Bc,
                                                 long long ldb, int lane) {
  Cols<VEC> acc;
#pragma unroll
  for (int c = 0; c < VEC; ++c) acc.v[c] = 0.f;
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
        a[t] = vh[(c0 + i) * heads];
        bv[t] = load_cols<T, VEC>(Bc + (long long)j * ldb);
      }
#pragma unroll
      for (int t = 0; t < kInFlight; ++t)
        if (i0 + t < cnt) {
#pragma unroll
          for (int c = 0; c < VEC; ++c) acc.v[c] = __builtin_fmaf(a[t], bv[t].v[c], acc.v[c]);
        }
    }
  }
  return acc;
}

// C[i, c] = epi(x) for the lane's columns.
template <int VEC>
__device__ __forceinline__ void store_row(float* Cp, const Cols<VEC>& x, float alpha, float beta) {
  Cols<VEC> o;
  if (beta == 0.f) {
#pragma unroll
    for (int c = 0; c < VEC; ++c) o.v[c] = alpha * x.v[c];
  } else {
    const Cols<VEC> old = load_cols<float, VEC>(Cp);
#pragma unroll
    for (int c = 0; c < VEC; ++c) o.v[c] = __builtin_fmaf(beta, old.v[c], alpha * x.v[c]);
  }
  store_cols<VEC>(Cp, o);
}

// W = heads * d columns in tiles of 64 VEC (blockIdx.y); VEC divides d, so a lane's
// columns belong to one head. A lane past the last column works on the last VEC columns
// again and stores nothing, so that every lane is active at the readlanes. ldb counts
// elements of T, ldc floats.
template <typename T, int VEC>
__global__ __launch_bounds__(kWG) void csrmm_heads_kernel(
    int m, int d, int nnz, int heads, const int* __restrict__ rowptr,
    const int* __restrict__ colind, const float* __restrict__ val, int base,
    const T* __restrict__ B, long long ldb, float alpha, float beta, float* C,
    long long ldc) {
  __shared__ int s_rows[2];
  __shared__ unsigned s_mask[2 * kWavesPerWG];
  __shared__ float s_sums[kCsrRound * VEC * kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long W = (long long)heads * d;
  const long long cw = (long long)blockIdx.y * (kWave * VEC) + (long long)lane * VEC;
  const bool mine = cw < W;
  const long long col = mine ? cw : W - VEC;
  const int h = (int)(col / d);
  const float* vh = val + h;
  const T* Bc = B + col;
  float* Cc = C + col;

  const Rows wr = wave_rows(rowptr, m, base, nnz, wave);
  if (tid == 0) s_rows[0] = wr.r0;
  if (tid == kWG - 1) s_rows[1] = wr.r1;

  // rows of one piece (and empty rows), one after the other by the wave
  for (int r = wr.r0; r < wr.r1; ++r) {  // wave-uniform
    const long long a = row_pos(rowptr, r, base, nnz);
    const long long L = row_pos(rowptr, r + 1, base, nnz) - a;
    if (L > kCsrPiece) continue;
    Cols<VEC> x;
    if (L > 0) {
      x = piece_chain<T, VEC>(a, a + L, colind, vh, heads, base, Bc, ldb, lane);
#pragma unroll
      for (int c = 0; c < VEC; ++c) x.v[c] = -0.f + x.v[c];
    } else {
#pragma unroll
      for (int c = 0; c < VEC; ++c) x.v[c] = 0.f;
    }
    if (mine) store_row<VEC>(Cc + (long long)r * ldc, x, alpha, beta);
  }

  // rows of several pieces, each by the workgroup that owns it: pieces round-robin over
  // the waves, kCsrRound piece sums per barrier, added in piece order from -0
  __syncthreads();
  for_long_rows(rowptr, m, base, nnz, s_rows[0], s_rows[1], kCsrPiece, s_mask,
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
                      const Cols<VEC> acc = piece_chain<T, VEC>(s, min(s + T_, b), colind, vh,
                                                                heads, base, Bc, ldb, lane);
#pragma unroll
                      for (int c = 0; c < VEC; ++c) s_sums[(P * VEC + c) * kWave + lane] = acc.v[c];
                    }
                    __syncthreads();
                    for (int P = 0; P < cnt; ++P)
#pragma unroll
                      for (int c = 0; c < VEC; ++c) x.v[c] = x.v[c] + s_sums[(P * VEC + c) * kWave + lane];
                    __syncthreads();
                  }
                  if (wave == 0 && mine) store_row<VEC>(Cc + (long long)row * ldc, x, alpha, beta);
                });
}

// ------------------------------------------------------------------ launchers' choice
template <typename T>
using SddmmKernel = void (*)(int, int, int, int, const int*, const int*, int, const T*, long long,
                             const T*, long long, float, float, float*);
template <typename T>
using CsrmmKernel = void (*)(int, int, int, int, const int*, const int*, const float*, int,
                             const T*, long long, float, float, float*, long long);

template <typename T, int G>
Picked<SddmmKernel<T>> pick_sddmm(bool vec) {
  return vec ? picked<sddmm_heads_kernel<T, G, true>>() : picked<sddmm_heads_kernel<T, G, false>>();
}
template <typename T>
Picked<CsrmmKernel<T>> pick_csrmm(int vec) {
  if (vec == 4) return picked<csrmm_heads_kernel<T, 4>>();
  if (vec == 2) return picked<csrmm_heads_kernel<T, 2>>();
  return picked<csrmm_heads_kernel<T, 1>>();
}

// The sampled product at d > 0.
template <typename T>
spmm_status_t launch_sddmm_heads_of(spmm_context* ctx, int m, int d, int nnz, int heads,
                                      const int* rowptr, const int* colind, int base, const T* X,
                                      int ldx, const T* Y, int ldy, float alpha, float beta,
                                      float* out) {
  const long long vnnz = (long long)nnz * heads;
  const int G = sddmm_group_lanes(d);
  // a chunk of four elements is one load: 16 bytes of floats, 8 of 16-bit elements
  const bool vec = d % 4 == 0 && aligned(X, 4 * sizeof(T)) && aligned(Y, 4 * sizeof(T)) &&
                   ldx % 4 == 0 && ldy % 4 == 0;
  const Picked<SddmmKernel<T>> kern = G == 1    ? pick_sddmm<T, 1>(vec)
                                      : G == 2  ? pick_sddmm<T, 2>(vec)
                                      : G == 4  ? pick_sddmm<T, 4>(vec)
                                      : G == 8  ? pick_sddmm<T, 8>(vec)
                                      : G == 16 ? pick_sddmm<T, 16>(vec)
                                      : G == 32 ? pick_sddmm<T, 32>(vec)
                                                : pick_sddmm<T, 64>(vec);
  // at least 32 steps of 64 / G virtual positions per wave, at most 128 waves per CU
  // (spmm_set_csr_waves_per_cu sets the wave count itself, at least one step each): the
  // share is computed in the kernel from the row pointer's own count
  const long long S = kWave / G;
  const long long steps = (vnnz + S - 1) / S;
  const long long waves =
      ctx->csr_waves_per_cu > 0
          ? std::min<long long>((long long)ctx->num_cus * ctx->csr_waves_per_cu, steps)
          : std::min<long long>(std::max<long long>((steps + 31) / 32, 1),
                                (long long)ctx->num_cus * 128);
  const unsigned grid = (unsigned)((waves + kWavesPerWG - 1) / kWavesPerWG);
  return launch_picked(ctx, kern, dim3(grid), dim3(kWG), m, d, nnz, heads, rowptr, colind, base,
                       X, (long long)ldx, Y, (long long)ldy, alpha, beta, out);
}

// The widest lane the product may launch: it divides d, keeps B's loads (sizeof(T) vec
// bytes) and C's stores (4 vec bytes) aligned and leaves no tile mostly idle.
template <typename T>
int csrmm_heads_vec(int d, int heads, const T* B, int ldb, const float* C, int ldc) {
  const long long W = (long long)heads * d;
  int vec = W > 128 ? 4 : W > 64 ? 2 : 1;
  while (vec > 1 && !(d % vec == 0 && ldb % vec == 0 && ldc % vec == 0 &&
                      aligned(B, sizeof(T) * vec) && aligned(C, 4 * vec)))
    vec >>= 1;
  return vec;
}

template <typename T>
spmm_status_t launch_csrmm_heads_of(spmm_context* ctx, int m, int d, int nnz, int heads,
                                      const int* rowptr, const int* colind, const float* val,
                                      int base, const T* B, int ldb, float alpha, float beta,
                                      float* C, int ldc) {
  const long long W = (long long)heads * d;
  const int vec = csrmm_heads_vec(d, heads, B, ldb, C, ldc);
  const long long ntiles = (W + kWave * vec - 1) / (kWave * vec);
  if (ntiles > 65535) return SPMM_STATUS_NOT_SUPPORTED;  // the grid's y extent
  const unsigned tiles = (unsigned)ntiles;
  const unsigned grid = merge_grid(ctx, (long long)m + nnz, kCsrItemsPerWave);
  return launch_picked(ctx, pick_csrmm<T>(vec), dim3(grid, tiles), dim3(kWG), m, d, nnz, heads,
                       rowptr, colind, val, base, B, (long long)ldb, alpha, beta, C,
                       (long long)ldc);
}

}  // namespace
