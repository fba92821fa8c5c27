// Fused MAT-Dec shared actor forward / backward, token-on-lane tiles (mat_train_ct.h).  Reference:
// ma_transformer.py:181-188,212-216 (Decoder with dec_actor and share_actor: one MLP on every agent's observation),
// transformer_act.py:103-129,176-189 (log-prob / entropy of the stored actions).
//
// The actor is two stages the training kernels already hold, run back to back on one token tile with no attention, no
// cross attention and no LDS in the forward:
//  * LN(od) -> Linear(od, 64) -> GELU -> LN: the encoder's observation embedding and its ln (mat_embed_ct.h obs_ln /
//    we_frags / embed_pre; the loops around them are those of enc_fwd_tile / enc_bwd_tile).  obs_dim <= 16 embeds
//    in-kernel (a constant EncX{nullptr, nullptr}); wider observations run the WIDE instantiations (the *_wide
//    kernels and entry points), which take the pre-activation of obs_embed.hip as EncX.pre_in and hand d pre back
//    through EncX.dpre_out — the encoder's pre_in branches, chosen at compile time here;
//  * Linear(64, 64) -> GELU -> LN -> Linear(64, A) + the categorical / Normal statistics and masks: the decoder's
//    action head (mat_head_ct.h head_fwd_ct / head_bwd_ct).
// Both headers take the kernel argument ActP as it is (they read the fields it shares by name with EncP / DecP).  This
// file holds the actor's own tiles, kernels and host API.
// The backward runs on the persistent grid of the other training backwards (launch_ct, chunk plan and stagger of
// FOR_TILES), so a minibatch's backwards all write the same mdl_ct_bwd_grid(B, SQ) private gradient copies.
//
// LayerNorm: the two-pass form (mat_train_ct.h ln_fwd_ct), for this unit and its backward wrapper
// mat_actor_ct_bwd.hip, as in the encoder's units.  The decoder's units build the one-pass form, so the actor's action
// head and the decoder's action head — the same head_fwd_ct source — sum their LayerNorm statistics in different
// orders and differ in the last bits.  Each is pinned by its own tests (tests/test_gpu_dec_actor_train.py: fp64 parity,
// bitwise repeats, rollout vs learner for the actor); changing this value changes the actor's bits.
#define MDL_LN_ONEPASS 0
#include "mat_train_ct.h"
#include "mat_embed_ct.h"
#include "mat_head_ct.h"

namespace {

// ============================================================================================== forward
// LOGITS (rollout, never with SAVE): the head's unmasked logits [tok][A] leave instead of log-prob / entropy — the
// same embedding, W_2, LayerNorm and logit products as the learner's pass; masking and sampling stay with the caller
//
// WIDE (obs_dim > 16, compile time): the embedding pre-activation comes in as ex.pre_in, computed by the obs-embedding
// GEMM kernels (obs_embed.hip) — no W_1 fragments and no LN_obs here; GELU, LayerNorm and the saves are the narrow
// tile's.  The narrow instantiations take a constant EncX{nullptr, nullptr} and keep their instruction streams
// (profiles/dec_actor_wide/README.md).
template <bool SAVE, int MA, bool CONT, bool LOGITS, bool WIDE>
__device__ __forceinline__ void actor_fwd_tile(const ActP& a, const EncX& ex, char* smem, int seq0, int nseq) {
  const Ctx c = make_ctx(a, smem, seq0, nseq);
  if (c.nseq <= 0) return;
  const int lane = c.lane, g = lane >> 4;
  CT xr[MAXRT];
  {
    bf16x8 W[4];
    if constexpr (!WIDE) we_frags(a, W, lane);
    const CT gam = ld_vec(a.ln0_g, lane), bet = ld_vec(a.ln0_b, lane);
#pragma unroll
    for (int k = 0; k < MAXRT; ++k) {
      const int rt = c.wave + NW * k;
      if (rt < c.NT) {
        float oh[4], hat[4];
        CT pre, xh;
        if constexpr (WIDE) pre = ld_gf(ex.pre_in, c.tok0, rt, c.NR, lane);
        else pre = embed_pre(a, ex, rt, W, oh, hat, c);
        if (SAVE) {   // x-hat, GELU'(pre), rstd for the backward (which recomputes none of the embedding forward)
          CT gp;
          gelu_ct_both(pre, gp);
          const float rs = ln_fwd_ct(pre, xh, xr[k], gam, bet);
          st_g(a.es.xh, c.tok0, rt, c.NR, ct_pack(xh), lane);
          st_g(a.es.gp, c.tok0, rt, c.NR, ct_pack(gp), lane);
          st_tokf(a.es.rs, rt, rs, c);
        } else {
          gelu_ct(pre);
          ln_fwd_ct(pre, xh, xr[k], gam, bet);
        }
      }
    }
  }
  if (!LOGITS) {
    head_fwd_ct<MA, CONT, false>(a, xr, SAVE, c);
    return;
  }
  HeadW<MA> W;
  head_w<MA>(a, W, lane);
  AFr H;
  loadA(H, a.h1.fa, lane);
  const CT bh = ld_vec(a.h1.b, lane), gam = ld_vec(a.lnh.g, lane), bet = ld_vec(a.lnh.b, lane);
#pragma unroll
  for (int k = 0; k < MAXRT; ++k) {
    const int rt = c.wave + NW * k;
    if (rt < c.NT) {
      const int row = rt * 16 + (lane & 15);
      const bool ok = row < c.NR;
      const size_t tok = (size_t)(c.tok0 + (ok ? row : 0));
      CT hh = bh, xh, n;
      mm(hh, H, ct_pack(xr[k]));
      gelu_ct(hh);
      ln_fwd_ct(hh, xh, n, gam, bet);
      f32x4 L[MA];
      head_logits_ct<MA>(a, W, n, L, lane);
#pragma unroll
      for (int ma = 0; ma < MA; ++ma)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * ma + 4 * g + r;
          if (ok && i < a.A) a.logits[tok * a.A + i] = L[ma][r];
        }
    }
  }
}

#ifndef MDL_CT_BWD_TU
template <bool SAVE, int MA, bool CONT, bool LOGITS>
__global__ __launch_bounds__(NTHR, FWD_WGPC) void mat_actor_fwd_ct(ActP a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  FOR_TILES(a, (actor_fwd_tile<SAVE, MA, CONT, LOGITS, false>(a, EncX{nullptr, nullptr}, smem, s0, ns)));
}
template <bool SAVE, int MA, bool CONT, bool LOGITS>
__global__ __launch_bounds__(NTHR, FWD_WGPC) void mat_actor_fwd_ct_wide(ActP a, EncX ex) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  FOR_TILES(a, (actor_fwd_tile<SAVE, MA, CONT, LOGITS, true>(a, ex, smem, s0, ns)));
}
#endif  // !MDL_CT_BWD_TU

// ============================================================================================== backward
// LDS vector slots: 0-1 head LayerNorm, 4 log_std (head_bwd_ct), 5-6 embedding LayerNorm, 7 embedding bias, 8-9
// observation LayerNorm (as enc_bwd_tile), 10 .. 10 + A - 1 the rows of d W_h2 and 10 + A d b_h2 for A <= 2 (head_bwd_ct
// places them at vs0 + A + 1 ..: vs0 = 9 - A); a wider head flushes d W_h2 per chunk (private copy / atomics)
__device__ __forceinline__ int actor_small_wg_slot0(const ActP& a) {
  return (MDL_SMALL_WG_VACC && a.A <= 2 && 10 + a.A + 1 <= VSLOTS) ? 9 - a.A : -1;
}

//
// WIDE (compile time): d pre leaves through ex.dpre_out (rows < NR only) for the obs-embedding backward kernels, which
// own the W_1, b_1 and LN_obs gradients — no LDS staging, no slots 7-9 and no wgrad_g here; slots 5-6 flush as before.
template <int MA, bool CONT, bool WIDE>
__device__ __forceinline__ void actor_bwd_tile(const ActP& a, const EncX& ex, char* smem, int seq0, int nseq, bool first) {
  const Ctx c = make_ctx(a, smem, seq0, nseq, first);
  if (c.nseq <= 0) return;
  zero_pad_rows(c);
  __syncthreads();
  const int lane = c.lane;
  CT dx[MAXRT];
  // ---------------- head backward: dx = d LN0 output; d W_2, d W_h2, their biases, the head LayerNorm, log_std
  head_bwd_ct<MA, CONT, false>(a, dx, c, actor_small_wg_slot0(a));
  // ---------------- embedding backward: x0 = LN0(GELU(pre)), pre = W_1 · LN_obs(obs) + b_1  (enc_bwd_tile)
  if constexpr (WIDE) {
    CT dlg, dlb;
    ct_zero(dlg);
    ct_zero(dlb);
    const CT gam = ld_vec(a.ln0_g, lane);
#pragma unroll
    for (int k = 0; k < MAXRT; ++k) {
      const int rt = c.wave + NW * k;
      if (rt < c.NT) {
        const bool ok = tok_ok(rt, c);
        const CT xh = ct_unpack(ld_g(a.es.xh, c.tok0, rt, c.NR, lane)), egp = ct_unpack(ld_g(a.es.gp, c.tok0, rt, c.NR, lane));
        CT de;
        ln_bwd_ct(dx[k], xh, ld_tokf(a.es.rs, rt, c), gam, ok, de, dlg, dlb);
#pragma unroll
        for (int i = 0; i < 4; ++i) de.v[i] *= egp.v[i];
        st_gf(ex.dpre_out, c.tok0, rt, c.NR, de, lane);   // stores rows < NR only
      }
    }
    flush_vec(dlg, c.g(a.d_ln0_g), 5, c);
    flush_vec(dlb, c.g(a.d_ln0_b), 6, c);
  } else {
    CT dlg, dlb, dbe;
    ct_zero(dlg);
    ct_zero(dlb);
    ct_zero(dbe);
    f32x4 dog = {0.f, 0.f, 0.f, 0.f}, dob = {0.f, 0.f, 0.f, 0.f};
    bf16x8 WT[2];
    weT_frags(a, WT, lane);
    const CT gam = ld_vec(a.ln0_g, lane);
#pragma unroll
    for (int k = 0; k < MAXRT; ++k) {
      const int rt = c.wave + NW * k;
      if (rt < c.NT) {
        const bool ok = tok_ok(rt, c);
        float oh[4] = {0.f, 0.f, 0.f, 0.f}, hat[4] = {0.f, 0.f, 0.f, 0.f};
        obs_ln(a, rt, c, oh, hat);   // X of W_1 and the LN_obs backward (od <= 16 dims in-lane)
        // the forward's x-hat, GELU'(pre) and rstd (no embedding product, GELU or LayerNorm forward here)
        const CT xh = ct_unpack(ld_g(a.es.xh, c.tok0, rt, c.NR, lane)), egp = ct_unpack(ld_g(a.es.gp, c.tok0, rt, c.NR, lane));
        CT de;
        ln_bwd_ct(dx[k], xh, ld_tokf(a.es.rs, rt, c), gam, ok, de, dlg, dlb);
#pragma unroll
        for (int i = 0; i < 4; ++i) de.v[i] *= egp.v[i];   // padded rows: zero
#pragma unroll
        for (int i = 0; i < 4; ++i) dbe.v[i] += de.v[i];
        CTr dh, dl;
        ct_split(de, dh, dl);
        st_lds(c.DA, rt, dh, ok, lane);   // dY of W_1
        CTr xo = ct_zero_r();
        xo.q[0] = make_uint2(pk2(oh[0], oh[1]), pk2(oh[2], oh[3]));
        st_lds(c.XB, rt, xo, ok, lane);   // X of W_1 (obs dims 0..15 = features 0..15 of the LDS row)
        // d(LN_obs output)[dim 4g + r] of this lane's token
        f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(WT[s], rb(dh, s), d, 0, 0, 0);
          d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(WT[s], rb(dl, s), d, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          dog[r] += ok ? d[r] * hat[r] : 0.f;
          dob[r] += ok ? d[r] : 0.f;
        }
      }
    }
    flush_vec(dlg, c.g(a.d_ln0_g), 5, c);
    flush_vec(dlb, c.g(a.d_ln0_b), 6, c);
    flush_vec(dbe, c.g(a.d_be), 7, c);
    const int c16 = lane & 15, g = lane >> 4;
    float og = 0.f, ob = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float s0 = group_sum<16>(dog[r]), s1 = group_sum<16>(dob[r]);
      og = c16 == r ? s0 : og;
      ob = c16 == r ? s1 : ob;
    }
    const int dim = 4 * g + c16;
    if (c16 < 4 && dim < a.od) {
      if (a.d_lno_g) vacc_add(c.g(a.d_lno_g), 8, dim, og, c, a.od);
      if (a.d_lno_b) vacc_add(c.g(a.d_lno_b), 9, dim, ob, c, a.od);
    }
    __syncthreads();
    wgrad_g(c.DA, c.XB, c.KP, c.g(a.d_we), a.od, 64, a.od, nullptr, c.wave, lane, c.gm);
  }
}

#ifdef MDL_CT_BWD_TU
template <int MA, bool CONT>
__global__ __launch_bounds__(NTHR, WGPC) void mat_actor_bwd_ct(ActP a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  vacc_begin(a, smem);
  FOR_TILES(a, (actor_bwd_tile<MA, CONT, false>(a, EncX{nullptr, nullptr}, smem, s0, ns, it_ == 0)));
  vacc_end(a, smem);
}
template <int MA, bool CONT>
__global__ __launch_bounds__(NTHR, WGPC) void mat_actor_bwd_ct_wide(ActP a, EncX ex) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  vacc_begin(a, smem);
  FOR_TILES(a, (actor_bwd_tile<MA, CONT, true>(a, ex, smem, s0, ns, it_ == 0)));
  vacc_end(a, smem);
}
#endif  // MDL_CT_BWD_TU

}  // namespace

// ============================================================================================== host API
static bool actor_args_ok(const ActP* p) {
  return p->od >= 1 && p->od <= 16 && p->A >= 1 && p->A <= 64 && p->n_disc >= 0 && p->n_disc <= p->L &&
         !(p->cont && p->n_disc != 0);
}
// the _wide entry points: obs_dim > 16 only with the pre-activation `pre_in` ([tok][64] f32 of the dense minibatch
// order, obs_embed.hip); the kernels then read neither obs nor the W_1 / LN_obs fields
static bool actor_args_ok_wide(const ActP* p, const float* pre_in) {
  return pre_in && p->od >= 1 && p->A >= 1 && p->A <= 64 && p->n_disc >= 0 && p->n_disc <= p->L &&
         !(p->cont && p->n_disc != 0);
}

#ifndef MDL_CT_BWD_TU
template <int MA, bool CONT>
static int actor_fwd_ct(const ActP* p, int save, hipStream_t st) {
  return save ? launch_ct(mat_actor_fwd_ct<true, MA, CONT, false>, p, true, st)
              : launch_ct(mat_actor_fwd_ct<false, MA, CONT, false>, p, true, st);
}
// MA = logit tiles of the head as in mdl_mat_dec_fwd_ct.  p->logits (no save): the logits-only pass of the rollout,
// which needs neither stored actions nor availability
MDL_API int mdl_mat_actor_fwd_ct(const ActP* p, int save, hipStream_t st) {
  if (!actor_args_ok(p)) return -1;
  if (p->logits) {
    if (save) return -1;
    if (p->A <= 16) return launch_ct(mat_actor_fwd_ct<false, 1, false, true>, p, true, st);
    return p->A <= 48 ? launch_ct(mat_actor_fwd_ct<false, 3, false, true>, p, true, st)
                      : launch_ct(mat_actor_fwd_ct<false, 4, false, true>, p, true, st);
  }
  if (!p->act || !p->logp || !p->ent) return -1;
  if (p->cont) return p->A <= 16 ? actor_fwd_ct<1, true>(p, save, st) : actor_fwd_ct<4, true>(p, save, st);
  if (p->A <= 16) return actor_fwd_ct<1, false>(p, save, st);
  return p->A <= 48 ? actor_fwd_ct<3, false>(p, save, st) : actor_fwd_ct<4, false>(p, save, st);
}

template <int MA, bool CONT>
static int actor_fwd_ct_wide(const ActP* p, const EncX& ex, int save, hipStream_t st) {
  return save ? launch_ct(mat_actor_fwd_ct_wide<true, MA, CONT, false>, p, true, st, ex)
              : launch_ct(mat_actor_fwd_ct_wide<false, MA, CONT, false>, p, true, st, ex);
}
// the same passes on a pre-activation computed outside (any obs_dim); pre_in null: the in-kernel embedding above
MDL_API int mdl_mat_actor_fwd_ct_wide(const ActP* p, const float* pre_in, int save, hipStream_t st) {
  if (!pre_in) return mdl_mat_actor_fwd_ct(p, save, st);
  if (!actor_args_ok_wide(p, pre_in)) return -1;
  const EncX ex{pre_in, nullptr};
  if (p->logits) {
    if (save) return -1;
    if (p->A <= 16) return launch_ct(mat_actor_fwd_ct_wide<false, 1, false, true>, p, true, st, ex);
    return p->A <= 48 ? launch_ct(mat_actor_fwd_ct_wide<false, 3, false, true>, p, true, st, ex)
                      : launch_ct(mat_actor_fwd_ct_wide<false, 4, false, true>, p, true, st, ex);
  }
  if (!p->act || !p->logp || !p->ent) return -1;
  if (p->cont) return p->A <= 16 ? actor_fwd_ct_wide<1, true>(p, ex, save, st) : actor_fwd_ct_wide<4, true>(p, ex, save, st);
  if (p->A <= 16) return actor_fwd_ct_wide<1, false>(p, ex, save, st);
  return p->A <= 48 ? actor_fwd_ct_wide<3, false>(p, ex, save, st) : actor_fwd_ct_wide<4, false>(p, ex, save, st);
}
#else
MDL_API int mdl_mat_actor_bwd_ct(const ActP* p, hipStream_t st) {
  if (!actor_args_ok(p) || !p->act || !p->dlogp || !p->dent || !p->sv_head || !p->hs.xh || !p->es.xh) return -1;
  if (p->cont) return p->A <= 16 ? launch_ct(mat_actor_bwd_ct<1, true>, p, false, st) : launch_ct(mat_actor_bwd_ct<4, true>, p, false, st);
  if (p->A <= 16) return launch_ct(mat_actor_bwd_ct<1, false>, p, false, st);
  return p->A <= 48 ? launch_ct(mat_actor_bwd_ct<3, false>, p, false, st) : launch_ct(mat_actor_bwd_ct<4, false>, p, false, st);
}
MDL_API int mdl_mat_actor_bwd_ct_wide(const ActP* p, const float* pre_in, float* dpre_out, hipStream_t st) {
  if (!pre_in) return mdl_mat_actor_bwd_ct(p, st);
  if (!actor_args_ok_wide(p, pre_in) || !dpre_out || !p->act || !p->dlogp || !p->dent || !p->sv_head || !p->hs.xh || !p->es.xh)
    return -1;
  const EncX ex{pre_in, dpre_out};
  if (p->cont) return p->A <= 16 ? launch_ct(mat_actor_bwd_ct_wide<1, true>, p, false, st, ex) : launch_ct(mat_actor_bwd_ct_wide<4, true>, p, false, st, ex);
  if (p->A <= 16) return launch_ct(mat_actor_bwd_ct_wide<1, false>, p, false, st, ex);
  return p->A <= 48 ? launch_ct(mat_actor_bwd_ct_wide<3, false>, p, false, st, ex) : launch_ct(mat_actor_bwd_ct_wide<4, false>, p, false, st, ex);
}
#endif  // MDL_CT_BWD_TU
