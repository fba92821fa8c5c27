// Action head of the fused training kernels, token-on-lane tiles (mat_train_ct.h):
// logits = W_h2 · LN(GELU(W_h1 x + b)) + b_h2  (ma_transformer.py:202-203,228) and the log-prob / entropy of the
// stored actions (transformer_act.py:103-129,176-189: masked Categorical, the Normal ratio agent of Semi_Discrete,
// per-dimension Normal, Available_Continuous), forward and backward.  Shared by the decoder (mat_dec_ct.hip) and
// MAT-Dec's shared actor (mat_actor_ct.hip), whose last four modules are the same stage.
//
// Every function takes the kernel's own argument struct (PT = DecP or ActP) and reads only the fields both carry
// under the same names: Bs / L / A / n_disc, act / ava, sidx, h1, lnh, wh2 / bh2 / log_std and their d_*, logp / ent,
// dlogp / dent, sv_head, hs.  (The Available_Continuous paths, AV, read no more than that; only the decoder
// instantiates them.)
//
// The LayerNorm here is the including translation unit's ln_fwd_ct (MDL_LN_ONEPASS, mat_train_ct.h): the decoder's
// head sums one-pass, the actor's two-pass.
//
// The second linear (64 -> A, A <= 64) runs on MFMA in the transposed layout: the logits of a token are spread over
// its 4 lanes (a = 16ma + 4g + r), so the softmax statistics are in-lane + 2 permlane swaps.  Logits use a hi/lo
// bf16 split of both operands (fp32-like: they feed exp(logp - old_logp)).  MA = ceil(A / 16) logit tiles.
#pragma once
#include "mat_train_ct.h"

namespace {

template <int MA>
struct HeadW { bf16x8 hi[MA][2], lo[MA][2]; };

template <int MA, typename PT>
__device__ __forceinline__ void head_w(const PT& p, HeadW<MA>& W, int lane) {
  const int c16 = lane & 15, g = lane >> 4;
#pragma unroll
  for (int ma = 0; ma < MA; ++ma)
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int a = 16 * ma + c16, k = 32 * s + 16 * (j >> 2) + 4 * g + (j & 3);
        const float w = a < p.A ? p.wh2[(a < p.A ? a : 0) * 64 + k] : 0.f;
        const uint16_t h = f2bf(w);
        W.hi[ma][s][j] = (short)h;
        W.lo[ma][s][j] = (short)f2bf(w - bf2f(h));
      }
}

template <int MA, typename PT>
__device__ __forceinline__ void head_logits_ct(const PT& p, const HeadW<MA>& W, const CT& n, f32x4* L, int lane) {
  const int g = lane >> 4;
  CTr nh, nl;
  ct_split(n, nh, nl);
#pragma unroll
  for (int ma = 0; ma < MA; ++ma) {
    f32x4 acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int a = 16 * ma + 4 * g + r;
      acc[r] = a < p.A ? p.bh2[a] : 0.f;
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(W.hi[ma][s], rb(nh, s), acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(W.hi[ma][s], rb(nl, s), acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(W.lo[ma][s], rb(nh, s), acc, 0, 0, 0);
    }
    L[ma] = acc;
  }
}

// availability bits of this lane's logit slots (a = 16ma + 4g + r): bit 4ma + r set = masked (tok: input row)
template <int MA, typename PT>
__device__ __forceinline__ unsigned slot_mask(const PT& p, size_t tok, int lane) {
  if (!p.ava) return 0u;
  const int g = lane >> 4;
  unsigned m = 0u;
#pragma unroll
  for (int ma = 0; ma < MA; ++ma)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int a = 16 * ma + 4 * g + r;
      if (a < p.A && p.ava[tok * p.A + a] == 0.f) m |= 1u << (4 * ma + r);
    }
  return m;
}

// per-token softmax statistics of the masked logits (transformer_act.py:14-21: logit[ava == 0] = -1e10)
struct HeadStat { float lse, H, la, mean; };
template <int MA, typename PT>
__device__ __forceinline__ HeadStat head_stats(const PT& p, const f32x4* L, unsigned am, int act, bool disc, int lane) {
  const int g = lane >> 4;
  float mx = -INFINITY;
#pragma unroll
  for (int ma = 0; ma < MA; ++ma)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int a = 16 * ma + 4 * g + r;
      const float l = ((am >> (4 * ma + r)) & 1u) ? -1e10f : L[ma][r];
      if (a < p.A) mx = fmaxf(mx, l);
    }
  mx = cross_row_max(mx);
  float se = 0.f, mean = 0.f;
#pragma unroll
  for (int ma = 0; ma < MA; ++ma)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int a = 16 * ma + 4 * g + r;
      const float l = ((am >> (4 * ma + r)) & 1u) ? -1e10f : L[ma][r];
      se += a < p.A ? __expf(l - mx) : 0.f;
      mean += a == p.A - 1 ? L[ma][r] : 0.f;
    }
  HeadStat st;
  st.lse = mx + __logf(cross_row_sum(se));
  st.mean = cross_row_sum(mean);
  float H = 0.f, la = 0.f;
  if (disc) {
#pragma unroll
    for (int ma = 0; ma < MA; ++ma)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int a = 16 * ma + 4 * g + r;
        const float l = (((am >> (4 * ma + r)) & 1u) ? -1e10f : L[ma][r]) - st.lse;
        H -= a < p.A ? __expf(l) * l : 0.f;
        la += a == act ? l : 0.f;
      }
  }
  st.H = cross_row_sum(H);
  st.la = cross_row_sum(la);
  return st;
}

// Normal-head std = sigmoid(log_std) * 0.5 (transformer_act.py:6, ma_transformer.py action std), from the parameter
// itself (round 1 read a per-minibatch torch copy: three launches per minibatch)
template <typename PT>
__device__ __forceinline__ float head_sd(const PT& p, int a) { return 0.5f / (1.f + __expf(-p.log_std[a])); }

// Available_Continuous head (A <= 16: one logit tile, logits 0 and 1 in r = 0, 1 of the token's g = 0 lane): the
// categorical over the two availability-masked logits 0, 1.  cls = argmax(act[:2]) (index 0 on a tie, as torch.argmax)
struct AvCat { float lp[2], H; int cls; bool m[2]; };
template <typename PT>
__device__ __forceinline__ AvCat av_cat(const PT& p, const f32x4& L, size_t stok) {
  AvCat s;
  const float* arow = p.act + stok * p.A;
  s.cls = arow[1] > arow[0] ? 1 : 0;
  s.m[0] = p.ava && p.ava[stok * p.A] == 0.f;
  s.m[1] = p.ava && p.ava[stok * p.A + 1] == 0.f;
  const float l0 = s.m[0] ? -1e10f : L[0], l1 = s.m[1] ? -1e10f : L[1];
  const float mx = fmaxf(l0, l1);
  const float lse = mx + __logf(__expf(l0 - mx) + __expf(l1 - mx));
  s.lp[0] = l0 - lse;
  s.lp[1] = l1 - lse;
  s.H = -(__expf(s.lp[0]) * s.lp[0] + __expf(s.lp[1]) * s.lp[1]);
  return s;
}

template <int MA, bool CONT, bool AV = false, typename PT>
__device__ __forceinline__ void head_fwd_ct(const PT& p, const CT* xr, bool save, const Ctx& c) {
  const int lane = c.lane, g = lane >> 4;
  HeadW<MA> W;
  head_w<MA>(p, W, lane);
  AFr H;
  loadA(H, p.h1.fa, lane);
  const CT bh = ld_vec(p.h1.b, lane), gam = ld_vec(p.lnh.g, lane), bet = ld_vec(p.lnh.b, lane);
  CP_MARK(31);
#pragma unroll
  for (int k = 0; k < MAXRT; ++k) {
    const int rt = c.wave + NW * k;
    if (rt < c.NT) {
      const int row = rt * 16 + (lane & 15);
      const bool ok = row < c.NR;
      const size_t tok = (size_t)(c.tok0 + (ok ? row : 0)), stok = src_tok(p.sidx, tok, c.L);
      const unsigned am = (CONT || AV) ? 0u : slot_mask<MA>(p, stok, lane);
      const float actf = (CONT || AV) ? 0.f : p.act[stok];
      const CTr x = ct_pack(xr[k]);
      if (save) st_g(p.sv_head, c.tok0, rt, c.NR, x, lane);
      CT hh = bh, xh, n;
      mm(hh, H, x);
      if (save && p.hs.xh) {   // x-hat, GELU'(h), rstd for the backward
        CT gp;
        gelu_ct_both(hh, gp);
        const float rs = ln_fwd_ct(hh, xh, n, gam, bet);
        st_g(p.hs.xh, c.tok0, rt, c.NR, ct_pack(xh), lane);
        st_g(p.hs.gp, c.tok0, rt, c.NR, ct_pack(gp), lane);
        st_tokf(p.hs.rs, rt, rs, c);
      } else {
        gelu_ct(hh);
        ln_fwd_ct(hh, xh, n, gam, bet);
      }
      CP_MARK(32);
      f32x4 L[MA];
      head_logits_ct<MA>(p, W, n, L, lane);
      CP_MARK(33);
      if (AV) {   // column 0: the availability choice; column a - 1: Normal(mean = logit a, std) of dimension a >= 2
        static_assert(!AV || MA == 1, "Available_Continuous: one logit tile");
        const int nlp = p.A - 1;
        if (ok && g == 0) {
          const AvCat s = av_cat(p, L[0], stok);
          p.logp[tok * nlp] = s.cls ? s.lp[1] : s.lp[0];
          p.ent[tok * nlp] = s.H;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int a = 4 * g + r;
          if (ok && a >= 2 && a < p.A) {
            const float sd = head_sd(p, a), z = (p.act[stok * p.A + a] - L[0][r]) / sd;
            p.logp[tok * nlp + a - 1] = -0.5f * z * z - __logf(sd) - HALF_LOG_2PI;
            p.ent[tok * nlp + a - 1] = 0.5f + HALF_LOG_2PI + __logf(sd);
          }
        }
        continue;
      }
      if (CONT) {   // per-dimension Normal(mean, std): this lane's dims a = 16ma + 4g + r
#pragma unroll
        for (int ma = 0; ma < MA; ++ma)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int a = 16 * ma + 4 * g + r;
            if (ok && a < p.A) {
              const float sd = head_sd(p, a), z = (p.act[stok * p.A + a] - L[ma][r]) / sd;
              p.logp[tok * p.A + a] = -0.5f * z * z - __logf(sd) - HALF_LOG_2PI;
              p.ent[tok * p.A + a] = 0.5f + HALF_LOG_2PI + __logf(sd);
            }
          }
        continue;
      }
      const bool disc = (row % c.L) < p.n_disc;
      const int act = min(max((int)actf, 0), p.A - 1);
      const HeadStat st = head_stats<MA>(p, L, am, act, disc, lane);
      float lp, en;
      if (disc) {
        lp = st.la;
        en = st.H;
      } else {
        const float sd = head_sd(p, p.A - 1), z = (actf - st.mean) / sd;
        lp = -0.5f * z * z - __logf(sd) - HALF_LOG_2PI;
        en = 0.5f + HALF_LOG_2PI + __logf(sd);
      }
      if (ok && g == 0) {
        p.logp[tok] = lp;
        p.ent[tok] = en;
      }
      CP_MARK(34);
    }
  }
}

// A/B: 0 compiles out the LDS vector slots of the small weight gradients (the callers' vs0: small_wg_slot0 in
// mat_dec_ct.hip, actor_small_wg_slot0 in mat_actor_ct.hip), leaving the per-chunk private / atomic flush
#ifndef MDL_SMALL_WG_VACC
#define MDL_SMALL_WG_VACC 1
#endif

// dx[k] = d (head input) of this wave's k-th row tile; d W_h1, d W_h2, their biases, the head LayerNorm (vector slots
// 0-1) and log_std (slot 4).  vs0 >= 0: d W_h2 / d b_h2 go to the LDS vector slots vs0 + A + 1 .. vs0 + 2A + 1
template <int MA, bool CONT, bool AV = false, typename PT>
__device__ __forceinline__ void head_bwd_ct(const PT& p, CT* dx, const Ctx& c, int vs0) {
  const int lane = c.lane, g = lane >> 4;
  constexpr int SB = (MA + 1) / 2;   // k-steps over the logit axis in dn = W_h2ᵀ dz
  CT dlg, dlb;
  ct_zero(dlg);
  ct_zero(dlb);
  float dls = 0.f;
  f32x4 dlsv[MA];   // continuous: per-dimension log_std partials of this lane's slots
#pragma unroll
  for (int ma = 0; ma < MA; ++ma) dlsv[ma] = f32x4{0.f, 0.f, 0.f, 0.f};
  {
    HeadW<MA> W;
    head_w<MA>(p, W, lane);
    // W_h2ᵀ as A fragments: rows = features 16mt + (lane&15), k = logit index perm(s, g, j)
    bf16x8 WT[4][SB];
    {
      const int c16 = lane & 15;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int s = 0; s < SB; ++s)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int a = 32 * s + 16 * (j >> 2) + 4 * g + (j & 3);
            const float w = a < p.A ? p.wh2[(a < p.A ? a : 0) * 64 + 16 * mt + c16] : 0.f;
            WT[mt][s][j] = (short)f2bf(w);
          }
    }
    // the forward's x-hat, GELU'(h) and rstd of the head (no W_h1 product, GELU or LayerNorm forward here)
    CTr hxh[MAXRT], hgp[MAXRT];
    float hrs[MAXRT];
    {
      CTr xs[MAXRT];
#pragma unroll
      for (int k = 0; k < MAXRT; ++k) {
        const int rt = c.wave + NW * k;
        if (rt < c.NT) {
          xs[k] = ld_g(p.sv_head, c.tok0, rt, c.NR, lane);
          hxh[k] = ld_g(p.hs.xh, c.tok0, rt, c.NR, lane);
          hgp[k] = ld_g(p.hs.gp, c.tok0, rt, c.NR, lane);
          hrs[k] = ld_tokf(p.hs.rs, rt, c);
        }
      }
#pragma unroll
      for (int k = 0; k < MAXRT; ++k) {
        const int rt = c.wave + NW * k;
        if (rt < c.NT) st_lds(c.KB, rt, xs[k], tok_ok(rt, c), lane);   // X of W_h1
      }
    }
    const CT gam = ld_vec(p.lnh.g, lane), bet = ld_vec(p.lnh.b, lane);
#pragma unroll
    for (int k = 0; k < MAXRT; ++k) {
      const int rt = c.wave + NW * k;
      if (rt < c.NT) {
        const int row = rt * 16 + (lane & 15);
        const bool ok = row < c.NR;
        const size_t tok = (size_t)(c.tok0 + (ok ? row : 0)), stok = src_tok(p.sidx, tok, c.L);
        const unsigned am = (CONT || AV) ? 0u : slot_mask<MA>(p, stok, lane);
        const float actf = (CONT || AV) ? 0.f : p.act[stok];
        const float dlp = (ok && !CONT && !AV) ? p.dlogp[tok] : 0.f, den = (ok && !CONT && !AV) ? p.dent[tok] : 0.f;
        const CT xh = ct_unpack(hxh[k]), ggp = ct_unpack(hgp[k]);
        const float rs = hrs[k];
        CT n;
#pragma unroll
        for (int i = 0; i < 4; ++i) n.v[i] = xh.v[i] * gam.v[i] + bet.v[i];
        f32x4 L[MA];
        head_logits_ct<MA>(p, W, n, L, lane);
        const bool disc = !CONT && !AV && (row % c.L) < p.n_disc;
        const int act = min(max((int)actf, 0), p.A - 1);
        const HeadStat st = (CONT || AV) ? HeadStat{0.f, 0.f, 0.f, 0.f} : head_stats<MA>(p, L, am, act, disc, lane);
        // d loss / d logits of this lane's slots
        f32x4 Z[2 * SB];
#pragma unroll
        for (int ma = 0; ma < 2 * SB; ++ma) Z[ma] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (AV) {   // softmax gradient of the two masked logits (g = 0, r = 0, 1); Normal mean gradient of the rest
          const int nlp = p.A - 1;
          if (ok && g == 0) {
            const AvCat s = av_cat(p, L[0], stok);
            const float dl = p.dlogp[tok * nlp], de = p.dent[tok * nlp];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
              const float pr = __expf(s.lp[r]);
              // a masked logit is a constant (masked_fill): no gradient reaches it
              Z[0][r] = s.m[r] ? 0.f : dl * ((r == s.cls ? 1.f : 0.f) - pr) - de * pr * (s.lp[r] + s.H);
            }
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int a = 4 * g + r;
            if (ok && a >= 2 && a < p.A) {
              const float sd = head_sd(p, a), diff = p.act[stok * p.A + a] - L[0][r];
              const float dl = p.dlogp[tok * nlp + a - 1], de = p.dent[tok * nlp + a - 1];
              Z[0][r] = dl * diff / (sd * sd);
              const float dsd = dl * (diff * diff / (sd * sd * sd) - 1.f / sd) + de / sd;
              const float sg = 1.f / (1.f + __expf(-p.log_std[a]));
              dlsv[0][r] += dsd * 0.5f * sg * (1.f - sg);   // dimensions 0, 1 stay exactly zero
            }
          }
        } else if (CONT) {   // per-dimension Normal heads: d log p / d mean, and the log_std partials of this lane's dims
#pragma unroll
          for (int ma = 0; ma < MA; ++ma)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int a = 16 * ma + 4 * g + r;
              if (ok && a < p.A) {
                const float sd = head_sd(p, a), diff = p.act[stok * p.A + a] - L[ma][r];
                const float dl = p.dlogp[tok * p.A + a], de = p.dent[tok * p.A + a];
                Z[ma][r] = dl * diff / (sd * sd);
                const float dsd = dl * (diff * diff / (sd * sd * sd) - 1.f / sd) + de / sd;
                const float sg = 1.f / (1.f + __expf(-p.log_std[a]));
                dlsv[ma][r] += dsd * 0.5f * sg * (1.f - sg);
              }
            }
        } else if (disc) {
#pragma unroll
          for (int ma = 0; ma < MA; ++ma)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int a = 16 * ma + 4 * g + r;
              const float l = (((am >> (4 * ma + r)) & 1u) ? -1e10f : L[ma][r]) - st.lse;
              const float pr = __expf(l);
              const float z = dlp * ((a == act ? 1.f : 0.f) - pr) - den * pr * (l + st.H);
              Z[ma][r] = (ok && a < p.A) ? z : 0.f;
            }
        } else {
          const float sd = head_sd(p, p.A - 1), diff = actf - st.mean;
#pragma unroll
          for (int ma = 0; ma < MA; ++ma)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              Z[ma][r] = (ok && 16 * ma + 4 * g + r == p.A - 1) ? dlp * diff / (sd * sd) : 0.f;
          if (ok && g == 0) {
            const float dsd = dlp * (diff * diff / (sd * sd * sd) - 1.f / sd) + den / sd;
            const float sg = 1.f / (1.f + __expf(-p.log_std[p.A - 1]));
            dls += dsd * 0.5f * sg * (1.f - sg);
          }
        }
        // dn = W_h2ᵀ dz (hi / lo split of dz)
        CT dn;
        ct_zero(dn);
        CTr zh, zl;   // dz as a CT-shaped operand: piece ma = logits 16ma + 4g .. +3
        {
          CT zc;
#pragma unroll
          for (int ma = 0; ma < 4; ++ma) zc.v[ma] = ma < 2 * SB ? Z[ma < 2 * SB ? ma : 0] : f32x4{0.f, 0.f, 0.f, 0.f};
          ct_split(zc, zh, zl);
        }
#pragma unroll
        for (int s = 0; s < SB; ++s)
#pragma unroll
          for (int mt = 0; mt < 4; ++mt) {
            dn.v[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(WT[mt][s], rb(zh, s), dn.v[mt], 0, 0, 0);
            dn.v[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(WT[mt][s], rb(zl, s), dn.v[mt], 0, 0, 0);
          }
        st_lds(c.DA, rt, zh, ok, lane);            // dY of W_h2 (logit axis in the feature slots)
        st_lds(c.XB, rt, ct_pack(n), ok, lane);    // X of W_h2
        CT dgg;
        ln_bwd_ct(dn, xh, rs, gam, ok, dgg, dlg, dlb);
#pragma unroll
        for (int i = 0; i < 4; ++i) dgg.v[i] *= ggp.v[i];   // padded rows: x-hat, GELU' and rstd are zero
        st_lds(c.DQ, rt, ct_pack(dgg), ok, lane);   // dY of W_h1
      }
    }
  }
  {   // second pass (W_h1ᵀ): dx = W_h1ᵀ dY
    AFr Hb;
    loadA(Hb, p.h1.ba, lane);
#pragma unroll
    for (int k = 0; k < MAXRT; ++k) {
      const int rt = c.wave + NW * k;
      if (rt < c.NT) {
        ct_zero(dx[k]);
        mm(dx[k], Hb, ld_lds(c.DQ, rt, lane));
      }
    }
  }
  flush_vec(dlg, c.g(p.lnh.dg), 0, c);
  flush_vec(dlb, c.g(p.lnh.db), 1, c);
  if (CONT || AV) {   // (Available_Continuous: elements 0, 1 are added as zeros, so the flush stores them)
#pragma unroll
    for (int ma = 0; ma < MA; ++ma)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float t = group_sum<16>(dlsv[ma][r]);
        const int a = 16 * ma + 4 * g + r;
        if ((lane & 15) == 0 && a < p.A && p.d_log_std) vacc_add(c.g(p.d_log_std), 4, a, t, c, p.A);
      }
  } else {
    const float t = wave_sum(dls);
    if (lane == 0 && p.d_log_std && p.n_disc < p.L) vacc_add(c.g(p.d_log_std), 4, p.A - 1, t, c, p.A);
  }
  __syncthreads();
  CP_MARK(1);
  if (vs0 >= 0)   // slots vs0 + A + 1 .. (W_h2 rows), vs0 + 2A + 1 (bias)
    wgrad_g_vacc(c.DA, c.XB, c.KP, c.g(p.d_wh2), 64, p.A, 64, c.g(p.d_bh2), vs0 + p.A + 1, vs0 + 2 * p.A + 1, c);
  else
    wgrad_g(c.DA, c.XB, c.KP, c.g(p.d_wh2), 64, p.A, 64, c.g(p.d_bh2), c.wave, lane, c.gm);
  wgrad64(c.DQ, c.KB, p.h1, c);
  __syncthreads();
  CP_MARK(19);
}

}  // namespace
