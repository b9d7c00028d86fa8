// sddmm_kernels.hip — CSR-sampled dense-dense product (spmm_sddmm_csr_f32):
//   out[p] = epi(dot(X[i(p), 0..n), Y[j(p), 0..n)))   for every position p of the pattern,
// the gradient of A's values in C = A * B (X = grad_C, Y = B) and the edge logits of a
// graph attention layer (X = Y = H). No reference counterpart (cusparseSDDMM's shape).
//
// The association, a function of the two rows, n, alpha, beta and the
// old out[p] alone:
//   G(n) = min(64, max(1, pow2ceil(ceil(n / 4)))) lanes work on one nonzero. Lane l owns
//   the columns c with (c / 4) mod G == l and sums them in ascending c as one fp32 chain
//   acc = fma(x[c], y[c], acc) from +0. The G chains fold in the butterfly
//   acc_l + acc_(l xor s), s = 1, 2, ..., G / 2 (the pairwise tree over adjacent lanes:
//   addition commutes), and out[p] = alpha * d, or fma(beta, out[p], alpha * d).
// A column's owner depends on c alone: a base that is not 16-byte aligned, an ld or an n
// that is no multiple of 4 floats changes how the words are loaded (one dword per lane
// instead of dwordx4), never the result.
//
// The kernel: a wave takes a contiguous range of positions (an equal share of the
// pattern's steps of 64 / G positions, so degree skew costs nothing: a hub row is many
// waves reading one X row from cache). Every lane group finds the row of its first
// position in csrRowPtr by bisection and then walks forward; it keeps its row's X slice
// in registers until the row changes, and has the Y gathers of PD steps in flight: the
// index and Y loads of a batch carry no branch (a step past the share's end repeats the
// share's last position, an empty chunk reads the row's last one), since a load inside a
// branch is waited for inside it. Folds inside 16 lanes are DPP row rotations (the value
// is complete in a group's last lane), across rows two shuffles. No workspace, no
// atomics, no synchronisation. The fold, the share, the chunk loads and the launch are
// csr_rows.hpp's, shared with the multi-head kernel (heads_impl.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "context.hpp"
#include "csr_rows.hpp"

namespace {

// n up to 4 * 64 * kMaxChunks keeps the X slice in registers; wider rows take
// sddmm_wide_kernel
constexpr int kMaxChunks = 4;

template <int G, int NC, bool VEC, bool FULL>
__global__ __launch_bounds__(kWG) void sddmm_kernel(int m, int n, int nnz,
                                                    const int* __restrict__ rowptr,
                                                    const int* __restrict__ colind, int base,
                                                    const float* __restrict__ X, long long ldx,
                                                    const float* __restrict__ Y, long long ldy,
                                                    float alpha, float beta, float* out) {
  constexpr int S = kWave / G;                           // positions per step
  constexpr int PD = NC == 1 ? 8 : NC == 2 ? 4 : 2;      // steps whose Y gathers are in flight
  const int lane = threadIdx.x & (kWave - 1);
  const int sub = lane & (G - 1), grp = lane / G;
  const Share sh = wave_share(rowptr, m, base, nnz, S);  // wave-uniform
  const unsigned a = sh.a, b = sh.b;
  if (a >= b) return;
  int r = find_row(rowptr, m, base, min(a + grp, b - 1));
  long long re = (long long)rowptr[r + 1] - base;        // end of row r
  int rx = -1;                                           // the row x[] holds
  f32x4 x[NC];
#pragma unroll
  for (int t = 0; t < NC; ++t) x[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // A step past the share's end (the last batch alone) repeats the share's last
  // position: its loads stay in bounds and unconditional, and nothing is stored.
  const unsigned nsteps = (b - a + S - 1) / S;
  for (unsigned t0 = 0; t0 < nsteps; t0 += PD) {
    unsigned p[PD];
    bool ok[PD];
    int j[PD], ru[PD];
    f32x4 y[PD][NC];
#pragma unroll
    for (int u = 0; u < PD; ++u) {
      const unsigned q = a + (t0 + u) * S + grp;
      ok[u] = q < b;
      p[u] = min(q, b - 1);
      j[u] = __builtin_nontemporal_load(colind + p[u]);
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
      const float* yp = Y + (long long)(j[u] - base) * ldy;
#pragma unroll
      for (int t = 0; t < NC; ++t) y[u][t] = load4<float, VEC, FULL>(yp, 4 * (sub + G * t), n);
    }
#pragma unroll
    for (int u = 0; u < PD; ++u) {
      if (t0 + u < nsteps) {  // wave-uniform: the fold below runs with every lane active
        if (ru[u] != rx) {
          rx = ru[u];
          const float* xp = X + (long long)rx * ldx;
#pragma unroll
          for (int t = 0; t < NC; ++t) {
            x[t] = load4<float, VEC, FULL>(xp, 4 * (sub + G * t), n);
            settle(x[t]);
          }
        }
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < NC; ++t) acc = chain4<FULL>(acc, x[t], y[u][t], 4 * (sub + G * t), n);
        const float d = fold<G>(acc);
        if (ok[u] && sub == G - 1)
          __builtin_nontemporal_store(epilogue(d, alpha, beta, out + p[u]), out + p[u]);
      }
    }
  }
}

// n > 1024: a whole wave per position, X and Y read chunk by chunk (the X row stays in
// cache along a CSR row). The same chains: lane l owns the chunks l, l + 64, ...
template <bool VEC>
__global__ __launch_bounds__(kWG) void sddmm_wide_kernel(int m, int n, int nnz,
                                                         const int* __restrict__ rowptr,
                                                         const int* __restrict__ colind, int base,
                                                         const float* __restrict__ X,
                                                         long long ldx,
                                                         const float* __restrict__ Y,
                                                         long long ldy, float alpha, float beta,
                                                         float* out) {
  const int lane = threadIdx.x & (kWave - 1);
  const Share sh = wave_share(rowptr, m, base, nnz, 1);
  if (sh.a >= sh.b) return;
  int r = find_row(rowptr, m, base, sh.a);
  long long re = (long long)rowptr[r + 1] - base;
  for (unsigned p = sh.a; p < sh.b; ++p) {  // wave-uniform
    while ((long long)p >= re && r + 1 < m) {
      ++r;
      re = (long long)rowptr[r + 1] - base;
    }
    const float* xp = X + (long long)r * ldx;
    const float* yp = Y + (long long)(colind[p] - base) * ldy;
    float acc = 0.f;
    for (int c0 = 4 * lane; c0 < n; c0 += 4 * kWave)
      acc = chain4<false>(acc, load4<float, VEC, false>(xp, c0, n),
                          load4<float, VEC, false>(yp, c0, n), c0, n);
    const float d = fold<kWave>(acc);
    if (lane == kWave - 1) out[p] = epilogue(d, alpha, beta, out + p);
  }
}

// n == 0: every dot is +0.
__global__ __launch_bounds__(kWG) void sddmm_zero_kernel(int m, int nnz,
                                                         const int* __restrict__ rowptr, int base,
                                                         float alpha, float beta, float* out) {
  const long long p0 = max((long long)rowptr[0] - base, 0ll);
  const long long p1 = min((long long)rowptr[m] - base, (long long)nnz);
  for (long long p = p0 + (long long)blockIdx.x * kWG + threadIdx.x; p < p1;
       p += (long long)gridDim.x * kWG)
    out[p] = epilogue(0.f, alpha, beta, out + p);
}

using Kernel = void (*)(int, int, int, const int*, const int*, int, const float*, long long,
                        const float*, long long, float, float, float*);

template <int G, int NC>
Picked<Kernel> pick(bool vec, bool full) {
  if (vec) {
    // G = 1 / 2 (n <= 8): the only n with n % 4 == 0 is 4 G itself, so vec implies full
    if constexpr (G > 2)
      if (!full) return picked<sddmm_kernel<G, NC, true, false>>();
    return picked<sddmm_kernel<G, NC, true, true>>();
  }
  return full ? picked<sddmm_kernel<G, NC, false, true>>()
              : picked<sddmm_kernel<G, NC, false, false>>();
}

}  // namespace

namespace spmm {

spmm_status_t launch_sddmm(spmm_context* ctx, int m, int n, int nnz, const int* rowptr,
                           const int* colind, int base, const float* X, int ldx, const float* Y,
                           int ldy, float alpha, float beta, float* out) {
  const int G = sddmm_group_lanes(n);
  const int chunks = (n + 3) / 4;
  const int NC = std::max(1, (chunks + G - 1) / G);
  const bool vec = n % 4 == 0 && aligned(X, 16) && aligned(Y, 16) && ldx % 4 == 0 && ldy % 4 == 0;
  const bool full = n % (4 * G) == 0;
  if (n == 0) {
    const unsigned zgrid = (unsigned)std::min<long long>(((long long)nnz + kWG - 1) / kWG, 65536);
    const int zslot = timing_begin(ctx);
    SPMM_LAUNCH(ctx, sddmm_zero_kernel, dim3(zgrid), dim3(kWG), 0, m, nnz, rowptr,
                base, alpha, beta, out);
    timing_end(ctx, zslot);
    return from_hip(hipGetLastError());
  }
  Picked<Kernel> kern{};
  if (NC > kMaxChunks)
    kern = vec ? picked<sddmm_wide_kernel<true>>() : picked<sddmm_wide_kernel<false>>();
  else if (G == 1) kern = pick<1, 1>(vec, full);
  else if (G == 2) kern = pick<2, 1>(vec, full);
  else if (G == 4) kern = pick<4, 1>(vec, full);
  else if (G == 8) kern = pick<8, 1>(vec, full);
  else if (G == 16) kern = pick<16, 1>(vec, full);
  else if (G == 32) kern = pick<32, 1>(vec, full);
  else if (NC == 1) kern = pick<64, 1>(vec, full);
  else if (NC == 2) kern = pick<64, 2>(vec, full);
  else if (NC == 3) kern = pick<64, 3>(vec, full);
  else kern = pick<64, 4>(vec, full);
  // at least 32 steps of 64 / G positions per wave, at most 128 waves per CU: the share
  // is computed in the kernel from the row pointer's own count
  const long long S = NC > kMaxChunks ? 1 : kWave / G;
  const long long steps = ((long long)nnz + S - 1) / S;
  const long long waves = std::min<long long>(std::max<long long>((steps + 31) / 32, 1),
                                              (long long)ctx->num_cus * 128);
  const unsigned grid = (unsigned)((waves + kWavesPerWG - 1) / kWavesPerWG);
  return launch_picked(ctx, kern, dim3(grid), dim3(kWG), m, n, nnz, rowptr, colind, base, X,
                       (long long)ldx, Y, (long long)ldy, alpha, beta, out);
}

}  // namespace spmm
