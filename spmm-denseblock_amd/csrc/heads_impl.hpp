// heads_impl.hpp — the kernel text of the multi-head sampled product and CSR product
// (DESIGN.md §4j, §4k), parameterised by the storage type T of the per-node features:
//   float      heads_kernels.hip       spmm_sddmm_csr_heads_f32 / spmm_csrmm_heads_f32
//   f16_t      heads_half_kernels.hip  ..._f16  (binary16, widened by a conversion)
//   bf16_t     heads_half_kernels.hip  ..._bf16 (bfloat16 bit patterns, widened by a shift)
// with the helpers the edge softmax kernels of heads_kernels.hip share with them.
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
#include "launch_record.hpp"

namespace {

// Builtin types, so that a kernel's template arguments stay literals and builtin types in
// its symbol (tests/kernel_keys.py reads them): bf16_t is the bit pattern of a bfloat16.
using f16_t = _Float16;
using bf16_t = unsigned short;

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

__device__ __forceinline__ float epilogue(float d, float alpha, float beta, const float* op) {
  return beta == 0.f ? alpha * d : __builtin_fmaf(beta, *op, alpha * d);
}

// ------------------------------------------------------------------ widening
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

// ------------------------------------------------------------------ sampled product
// x from lane (l - N) mod 16 of the same 16-lane row (DPP row_ror:N).
template <int N>
__device__ __forceinline__ float dpp_ror(float x) {
  return dpp<0x120 + N>(x);
}

// The butterfly sum of the G chains of a lane group, complete in the group's last lane
// (sddmm_kernels.hip's fold). Every lane of the wave must be active.
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

// Columns c0 .. c0 + 3 of a head's slice of d > 0 columns, widened, without a branch. VEC
// (d % 4 == 0, bases aligned to four elements, ld % 4 == 0: a chunk is whole or empty):
// one load of four elements (a dwordx4 of floats, a dwordx2 of 16-bit elements), an empty
// chunk reading the slice's last one. Otherwise one load per column, a column from d on
// reading column d - 1. What is read in place of a missing column is never summed.
template <typename T, bool VEC>
__device__ __forceinline__ f32x4 load4(const T* __restrict__ row, int c0, int d) {
  if constexpr (VEC && std::is_same_v<T, float>) {
    return *reinterpret_cast<const f32x4*>(row + min(c0, d - 4));
  } else if constexpr (VEC) {
    const u32x2 t = *reinterpret_cast<const u32x2*>(row + min(c0, d - 4));
    return f32x4{widen_lo<T>(t[0]), widen_hi<T>(t[0]), widen_lo<T>(t[1]), widen_hi<T>(t[1])};
  } else {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = widen(row[min(c0 + e, d - 1)]);
    return v;
  }
}

__device__ __forceinline__ float chain4(float acc, const f32x4& x, const f32x4& y, int c0, int d) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (c0 + e < d) acc = __builtin_fmaf(x[e], y[e], acc);
  return acc;
}

template <typename T>
__device__ __forceinline__ void settle(T& x) {
  asm volatile("" : "+v"(x));
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

  // the wave's share [a, b) of the virtual positions: whole steps of S
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
        if (t == 0 || t < nc) y[u][t] = load4<T, VEC>(yp, 4 * (sub + G * t), d);
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
              x[t] = load4<T, VEC>(xp, 4 * (sub + G * t), d);
              settle(x[t]);
            }
        }
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < NC; ++t)
          if (t == 0 || t < nc) acc = chain4(acc, x[t], y[u][t], 4 * (sub + G * t), d);
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
template <typename K>
struct Picked {
  K fn;
  const char* id;
};
template <auto K>
Picked<decltype(K)> picked() {
  return {K, spmm::launch_id<K>()};
}

template <typename T>
using SddmmKernel = void (*)(int, int, int, int, const int*, const int*, int, const T*, long long,
                             const T*, long long, float, float, float*);
template <typename T>
using CsrmmKernel = void (*)(int, int, int, int, const int*, const int*, const float*, int,
                             const T*, long long, float, float, float*, long long);

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
  using spmm::from_hip;
  const long long vnnz = (long long)nnz * heads;
  const int chunks = (d + 3) / 4;
  int G = 1;
  while (G < chunks && G < kWave) G <<= 1;
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
  const int slot = spmm::timing_begin(ctx);
  spmm::note_launch(ctx, kern.id);
  hipLaunchKernelGGL(kern.fn, dim3(grid), dim3(kWG), 0, ctx->stream, m, d, nnz, heads, rowptr,
                     colind, base, X, (long long)ldx, Y, (long long)ldy, alpha, beta, out);
  spmm::timing_end(ctx, slot);
  return from_hip(hipGetLastError());
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
  using spmm::from_hip;
  const long long W = (long long)heads * d;
  const int vec = csrmm_heads_vec(d, heads, B, ldb, C, ldc);
  const long long ntiles = (W + kWave * vec - 1) / (kWave * vec);
  if (ntiles > 65535) return SPMM_STATUS_NOT_SUPPORTED;  // the grid's y extent
  const unsigned tiles = (unsigned)ntiles;
  const unsigned grid = merge_grid(ctx, (long long)m + nnz, kCsrItemsPerWave);
  const Picked<CsrmmKernel<T>> kern = pick_csrmm<T>(vec);
  const int slot = spmm::timing_begin(ctx);
  spmm::note_launch(ctx, kern.id);
  hipLaunchKernelGGL(kern.fn, dim3(grid, tiles), dim3(kWG), 0, ctx->stream, m, d, nnz, heads,
                     rowptr, colind, val, base, B, (long long)ldb, alpha, beta, C,
                     (long long)ldc);
  spmm::timing_end(ctx, slot);
  return from_hip(hipGetLastError());
}

}  // namespace
