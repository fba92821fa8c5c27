// How the rollout-decode kernels (mat_decode.hip, mat_decode_wave.hip) sample one agent row from its head outputs:
// the sampling noise, the availability mask, the 64-lane scan, the lane-per-action categorical sampler and the Normal
// draw.  Reference: transformer_act.py:8-22 (masking), 76-99.  The register sampler (A <= 4), the serial sampler and the
// 4-wave kernel's copies of the other two stay in their kernels: moved here, they changed those kernels' register
// allocation (profiles/decode_sample/README.md).
#pragma once
#include "decode_params.h"

// in-kernel sampling noise: one Philox block per (global env, row, call counter, purpose); purpose 0 = the categorical
// uniform (x) and the Normal draws of dims 0, 1 (Box-Muller of y, z); purpose 1 + k = dims 2 + 2k, 3 + 2k
__device__ __forceinline__ float draw_u(const DecParams& p, int env, int row) {
  const mdl::u4 r = mdl::philox4x32_10(p.genv0 + (uint32_t)env, (uint32_t)row, p.rctr, (uint32_t)mdl::P_POLICY, p.rk0, p.rk1);
  return mdl::u01_open_f(r.x);
}
__device__ __forceinline__ float draw_n(const DecParams& p, int env, int row, int a) {
  const int k = a >> 1;
  const mdl::u4 r = mdl::philox4x32_10(p.genv0 + (uint32_t)env, (uint32_t)row, p.rctr, (uint32_t)(mdl::P_POLICY + k),
                                       p.rk0, p.rk1);
  const uint32_t b0 = k == 0 ? r.y : r.x, b1 = k == 0 ? r.z : r.y;
  const float rad = sqrtf(-2.f * __logf(mdl::u01_open_f(b0))), th = 6.283185307179586f * mdl::u01_open_f(b1);
  return (a & 1) ? rad * __sinf(th) : rad * __cosf(th);
}

// an unavailable action's logit (transformer_act.py:8-22); anything at or below MASKED_BELOW is one.  The samplers clamp
// a draw above the rounded CDF's last edge to the last action whose logit is above it (the CDF is flat over masked ones)
constexpr float MASK_LOGIT = -1e10f;
constexpr float MASKED_BELOW = 0.5f * MASK_LOGIT;
__device__ __forceinline__ float mask_logit(bool masked, float l) { return masked ? MASK_LOGIT : l; }

__device__ __forceinline__ float rdlane(float x, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), l));
}
// inclusive prefix sum over the 64 lanes: DPP row_shr 1, 2, 4, 8 within each 16-lane row (zero fill), then the
// totals of the lower rows (3 readlanes) — VALU only, no ds_bpermute round trips
__device__ __forceinline__ float wave_incl_scan(float x, int lane) {
  x += mdl::dppf<0x111>(x);
  x += mdl::dppf<0x112>(x);
  x += mdl::dppf<0x114>(x);
  x += mdl::dppf<0x118>(x);
  const float t0 = rdlane(x, 15), t1 = rdlane(x, 31), t2 = rdlane(x, 47);
  const int r = lane >> 4;
  return x + ((r >= 1 ? t0 : 0.f) + (r >= 2 ? t1 : 0.f) + (r >= 3 ? t2 : 0.f));
}

// Lane-per-action sampler, A <= 64: l = this lane's masked logit (-inf where !aok = lane >= A); first-maximum argmax,
// inverse CDF = the number of actions whose running probability (a DPP scan of exp(l - lse)) is below u = u_of(),
// which is evaluated only when sampling.  Returns the wave-uniform action (the caller reads its logit from that lane).
template <class U>
__device__ __forceinline__ int cat_wave(float l, bool aok, int A, U&& u_of, bool det, int lane, float& lse) {
  const float mx = mdl::wave_max(l);
  int act = __ffsll((unsigned long long)__ballot(l == mx)) - 1;
  lse = mx + __logf(mdl::wave_sum(aok ? __expf(l - mx) : 0.f));
  if (!det) {
    const float cdf = wave_incl_scan(aok ? __expf(l - lse) : 0.f, lane);
    const float uu = u_of();
    const unsigned long long avm = (unsigned long long)__ballot(aok && l > MASKED_BELOW);   // available actions
    act = min((int)__popcll((unsigned long long)__ballot(aok && cdf < uu)), avm ? 63 - __clzll(avm) : A - 1);
  }
  return __builtin_amdgcn_readfirstlane(act);
}

// x = mu (deterministic) or mu + sd z; returns the Normal log-prob of x
__device__ __forceinline__ float normal_sample_lp(float mu, float sd, float z, bool det, float& x) {
  x = det ? mu : mu + sd * z;
  const float zs = (x - mu) / sd;
  return -0.5f * zs * zs - __logf(sd) - mdl::HALF_LOG_2PI;
}
