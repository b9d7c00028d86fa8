// softmax_rule.hpp — the EXP rule of the edge softmax (include/spmm_hip.h),
// one text for the host form (prep.cpp) and the kernels (softmax_kernels.hip), so that both
// give the same bits: fp32 +, *, explicit FMA, rint, float <-> int conversion and integer
// operations on the bit pattern alone; no libm exp, no hardware exp approximation.
//
//   softmax_exp(t), t = x - max <= 0 or NaN:
//     NaN -> NaN;  t < -64 (-inf included) -> +0;  t == 0 (either sign) -> 1.0f;
//     otherwise k = rint(t * log2(e)), r = t - k * ln2 by a two-constant Cody-Waite
//     reduction (|r| <= 0.3466), a degree-7 Horner polynomial for exp(r) in FMAs, and the
//     scaling by 2^k (-93 <= k <= 0) as an integer addition to the exponent field.
// The polynomial's value lies in [0.70, 1.42], so every nonzero result is a normal number
// (>= 2^-93) and no result depends on a denormal mode. No product feeds an addition
// outside an explicit FMA, so fp-contract cannot change a bit.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SPMM_SOFTMAX_HD __host__ __device__
#else
#define SPMM_SOFTMAX_HD
#endif

namespace spmm_rule {

constexpr int kSoftmaxPiece = 1024;   // positions per piece of the SUM rule
constexpr int kSoftmaxChains = 64;    // chains per piece
constexpr float kSoftmaxCut = -64.f;  // terms below it are exactly +0

SPMM_SOFTMAX_HD inline float softmax_exp(float t) {
  const bool in = t >= kSoftmaxCut;  // false for NaN
  const float tc = in ? t : 0.f;
  const float kf = __builtin_rintf(tc * 1.44269504088896341f);
  // ln2 = hi + lo, hi with 9 trailing zero bits: kf * hi is exact for |kf| < 512
  float r = __builtin_fmaf(kf, -0.693145751953125f, tc);
  r = __builtin_fmaf(kf, -1.42860682030941723e-6f, r);
  float p = 1.98412698412698413e-4f;  // 1 / 7!
  p = __builtin_fmaf(p, r, 1.38888888888888889e-3f);
  p = __builtin_fmaf(p, r, 8.33333333333333333e-3f);
  p = __builtin_fmaf(p, r, 4.16666666666666667e-2f);
  p = __builtin_fmaf(p, r, 1.66666666666666667e-1f);
  p = __builtin_fmaf(p, r, 0.5f);
  p = __builtin_fmaf(p, r, 1.f);
  p = __builtin_fmaf(p, r, 1.f);
  const int bits = __builtin_bit_cast(int, p) + (int)kf * (1 << 23);
  const float e = __builtin_bit_cast(float, bits);
  return in ? e : (t != t ? t : 0.f);
}

}  // namespace spmm_rule
