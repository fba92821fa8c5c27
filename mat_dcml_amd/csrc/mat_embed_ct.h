// In-kernel observation embedding of the fused training kernels, token-on-lane tiles (mat_train_ct.h):
// x0 = LN0(GELU(W_e · LN_obs(obs) + b_e))  (ma_transformer.py:127-129,146-147: obs_encoder, then ln) — the per-tile
// pieces: LN_obs, the W_e / W_eᵀ fragments and the pre-activation.  Shared by the encoder (mat_enc_ct.hip) and MAT-Dec's
// shared actor (mat_actor_ct.hip), whose first four modules are the same stage.
//
// The row-tile loops around them (forward: GELU, ln, the saves; backward: ln / bias / LN_obs / W_e gradients) stay in
// enc_fwd_tile / enc_bwd_tile and actor_fwd_tile / actor_bwd_tile: moved into functions of this header, the same
// statements compiled to other register allocations (profiles/train_headers/README.md), so a fix to one copy of
// those loops still has to be made in the other.
//
// Every function takes the kernel's own argument struct (PT = EncP or ActP) and reads only the fields both carry
// under the same names: Bs / L / od, obs, sidx, lno / we / be / ln0 and their d_*, es.
//
// obs_dim <= 16 runs in-kernel (LN_obs per lane, W_e on MFMA with a hi/lo split of the LN output); larger
// observations (SMAC: 1288) come in as the embedding pre-activation `pre_in` computed by the obs-embedding GEMM
// kernels (obs_embed.hip), and the backward hands d pre back through `dpre_out`.  The encoder branches on pre_in at
// run time; the actor at compile time (its WIDE tiles read pre_in / write dpre_out, its narrow tiles pass a constant
// EncX{nullptr, nullptr}, so their copy of embed_pre holds no pre_in branch).
#pragma once
#include "mat_train_ct.h"

namespace {

struct EncX {   // EncP extension of the round-2 kernels (passed next to EncP)
  const float* pre_in;   // [tok][64] embedding pre-activation (null: embed obs in-kernel, obs_dim <= 16)
  float* dpre_out;       // [tok][64] gradient w.r.t. pre_in (backward, when pre_in is used)
};

// LN_obs of this lane's token: lane (g, c) loads and normalises only its 4 dims 4g .. 4g+3 (od <= 16), the token's
// mean / variance reduce across the 4 lane rows (two-pass, as torch's LayerNorm); -> this lane's 4 dims of the LN
// output and x-hat.  Padded rows read zeros (finite x-hat 0, output = beta).
template <typename PT>
__device__ __forceinline__ void obs_ln(const PT& p, int rt, const Ctx& c, float oh[4], float hat[4]) {
  const int lane = c.lane, g = lane >> 4, od = p.od;
  const int row = rt * 16 + (lane & 15);
  const bool ok = row < c.NR;
  const float* src = p.obs + src_tok(p.sidx, (size_t)(c.tok0 + (ok ? row : 0)), c.L) * od;
  float o[4];
  bool in[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int kk = 4 * g + j;
    in[j] = kk < od;
    o[j] = (ok && in[j]) ? src[kk] : 0.f;
  }
  const float mean = cross_row_sum((o[0] + o[1]) + (o[2] + o[3])) / (float)od;
  float d[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) d[j] = in[j] ? o[j] - mean : 0.f;
  const float var = cross_row_sum((d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]));
  const float rstd = rsqrtf(var / (float)od + 1e-5f);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ks = in[j] ? 4 * g + j : 0;
    hat[j] = d[j] * rstd;
    oh[j] = in[j] ? hat[j] * p.lno_g[ks] + p.lno_b[ks] : 0.f;
  }
}

// W_e (64 x od, fp32) as A fragments: rows 16mt + (lane&15), k = obs dim 4g + j (j < 4; j >= 4 -> dims >= 16: 0)
template <typename PT>
__device__ __forceinline__ void we_frags(const PT& p, bf16x8 W[4], int lane) {
  const int c16 = lane & 15, g = lane >> 4;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int kk = 4 * g + j;
      const bool in = j < 4 && kk < p.od;
      const float w = p.we[(16 * mt + c16) * p.od + (in ? kk : 0)];
      W[mt][j] = (short)f2bf(in ? w : 0.f);
    }
}
// W_eᵀ as A fragments for d(LN_obs out) = W_eᵀ d pre: rows = obs dim (lane&15), k = features perm(s, g, j)
template <typename PT>
__device__ __forceinline__ void weT_frags(const PT& p, bf16x8 W[2], int lane) {
  const int c16 = lane & 15, g = lane >> 4;
  const bool in = c16 < p.od;
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int f = 32 * s + 16 * (j >> 2) + 4 * g + (j & 3);
      const float w = p.we[f * p.od + (in ? c16 : 0)];
      W[s][j] = (short)f2bf(in ? w : 0.f);
    }
}

template <typename PT>
__device__ __forceinline__ CT embed_pre(const PT& p, const EncX& x, int rt, const bf16x8 W[4], float oh[4], float hat[4],
                                        const Ctx& c) {
  if (x.pre_in) return ld_gf(x.pre_in, c.tok0, rt, c.NR, c.lane);
  obs_ln(p, rt, c, oh, hat);
  const uint32_t h01 = pk2(oh[0], oh[1]), h23 = pk2(oh[2], oh[3]);
  const uint32_t l01 = pk2(oh[0] - blo(h01), oh[1] - bhi(h01)), l23 = pk2(oh[2] - blo(h23), oh[3] - bhi(h23));
  const bf16x8 bh = mk8(h01, h23, 0u, 0u), bl = mk8(l01, l23, 0u, 0u);
  CT pre = ld_vec(p.be, c.lane);
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    pre.v[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(W[mt], bh, pre.v[mt], 0, 0, 0);
    pre.v[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(W[mt], bl, pre.v[mt], 0, 0, 0);
  }
  return pre;
}

}  // namespace
