// Fused MAT decoder (teacher-forced) forward / backward, token-on-lane tiles (mat_train_ct.h).  Reference:
// ma_transformer.py:95-116 (DecodeBlock: causal self attention, causal cross attention on the encoder output, MLP),
// :157-230 (Decoder: action embedding, blocks, action head), transformer_act.py:103-129,176-189 (teacher-forced
// log-prob / entropy of the stored actions: masked Categorical, and the Normal ratio agent of Semi_Discrete).
//
// This file holds the decoder's own tiles (action embedding, cross attention, dec_fwd_tile / dec_bwd_tile), kernels
// and host API; the action head is mat_head_ct.h, shared with the MAT-Dec actor (mat_actor_ct.hip).
//
// LayerNorm: the one-pass form (mat_train_ct.h ln_fwd_ct), for every LayerNorm of this unit and of its backward
// wrapper mat_dec_ct_bwd.hip — the action head's included.  The actor's units build the same head with the two-pass
// form, so the two heads sum in different orders; each is pinned by its own tests.
#define MDL_LN_ONEPASS 1
#include "mat_train_ct.h"
#include "mat_head_ct.h"

namespace {

// token of row i: 0 = start, 1 + a = one-hot of the previous agent's (discrete) action   (transformer_act.py:103-111)
__device__ __forceinline__ int dec_token_ct(const DecP& p, int tok, int i) {
  if (i == 0) return 0;
  int a = (int)p.act[src_tok(p.sidx, (size_t)tok, p.L) - 1];   // the previous agent of the same sequence
  a = a < 0 ? 0 : (a >= p.A ? p.A - 1 : a);
  return 1 + a;
}

// x0 pre-activation = W_a · onehot(token) — a column gather of W_a [64][A+1]; continuous action type:
// W_a · a_prev + b_a with a_prev the previous agent's action vector (zero for row 0)
// Available_Continuous: W_a [64][A+1] · (start flag, a_prev), no bias — column 0 for a sequence's first row, columns
// 1 .. A times the previous agent's action vector (one-hot choice, then the continuous dimensions) for the others
template <bool CONT, bool AV = false>
__device__ __forceinline__ CT dec_embed_pre_ct(const DecP& p, int rt, int& tokid, const Ctx& c) {
  const int lane = c.lane, g = lane >> 4;
  const int row = rt * 16 + (lane & 15);
  const bool ok = row < c.NR;
  CT pre;
  if (AV) {
    tokid = -1;
    const bool first = !ok || row % c.L == 0;
    const float* prev = p.act + (first ? 0 : src_tok(p.sidx, (size_t)(c.tok0 + row), c.L) - 1) * p.A;
    const int ld = p.A + 1;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) pre.v[mt][r] = first ? p.wa[(16 * mt + 4 * g + r) * ld] : 0.f;
    for (int k = 0; k < p.A; ++k) {
      const float x = first ? 0.f : prev[k];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) pre.v[mt][r] += p.wa[(16 * mt + 4 * g + r) * ld + 1 + k] * x;
    }
    return pre;
  }
  if (CONT) {
    tokid = -1;
    const bool first = !ok || row % c.L == 0;
    const float* prev = p.act + (first ? 0 : src_tok(p.sidx, (size_t)(c.tok0 + row), c.L) - 1) * p.A;
    pre = ld_vec(p.ba, lane);
    for (int k = 0; k < p.A; ++k) {
      const float x = first ? 0.f : prev[k];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) pre.v[mt][r] += p.wa[(16 * mt + 4 * g + r) * p.A + k] * x;
    }
    return pre;
  }
  tokid = ok ? dec_token_ct(p, c.tok0 + row, row % c.L) : 0;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) pre.v[mt][r] = p.wa[(16 * mt + 4 * g + r) * (p.A + 1) + tokid];
  return pre;
}

// Action-embedding table (discrete tokens): x0 = LN_dec(GELU(W_a[:, t])) depends only on the token id t in [0, A]
// (ma_transformer.py:194-195,224 on the one-hot shifted action), so its A + 1 rows — and for the backward x-hat,
// rstd and GELU' — are computed once per tile chunk, one wave per token row (lane = feature), instead of a W_a
// gather, an erf and a LayerNorm per token row.  fwd: X = x0; bwd: X = x-hat, GP = GELU'(pre), RS = rstd.
__device__ __forceinline__ void emb_table(const DecP& p, float* X, float* GP, float* RS, bool fwd, const Ctx& c) {
  const int f = c.lane;
  for (int t = c.wave; t <= p.A; t += NW) {
    float gp;
    const float e = gelu_erf_both(p.wa[f * (p.A + 1) + t], gp);
    const float mean = wave_sum(e) * (1.f / 64.f);
    const float d = e - mean;
    const float rstd = rsqrtf(wave_sum(d * d) * (1.f / 64.f) + 1e-5f);
    const float xh = d * rstd;
    if (fwd) {
      X[t * 64 + f] = fmaf(xh, p.lnd_g[f], p.lnd_b[f]);
    } else {
      X[t * 64 + f] = xh;
      GP[t * 64 + f] = gp;
      if (f == 0) RS[t] = rstd;
    }
  }
}
__device__ __forceinline__ CT emb_row(const float* T, int tok, int lane) {
  const int g = lane >> 4;
  CT x;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) x.v[mt] = *(const f32x4*)(T + tok * 64 + 16 * mt + 4 * g);
  return x;
}
// the tables fit the (free at that point) Q buffer (forward) / Q + K buffers (backward)
__device__ __forceinline__ bool emb_tab_fwd_ok(const DecP& p) { return (p.A + 1) * 64 * 4 <= p.NRP * 128; }
__device__ __forceinline__ bool emb_tab_bwd_ok(const DecP& p) { return (p.A + 1) * (2 * 64 + 1) * 4 <= 2 * p.NRP * 128; }

// ------------------------------------------------------------------------------------------ cross attention
// cross-attention projections: q = W_q rep (from global f32), k / v = W_k x1, W_v x1 (x1 = xr, or the saved x1 when
// xr is null) -> QB / KB / VB; x1 optionally saved (forward) or staged into XB (backward, X of dW_k / dW_v)
// (REG: x1 comes from the registers xr — a compile-time switch: a runtime `xr ? xr[k] : load` put the register
// array's address into a pointer select, which kept all of xr in scratch memory in the forward kernel)
template <bool REG>
__device__ __forceinline__ void cross_proj(const Mat* m, const CT* xr, const bf16_t* sv_x1_in, const float* rep,
                                           bf16_t* sv_x1_out, const Ctx& c, bool store_xb = true) {
  const int lane = c.lane;
  CTr xp[MAXRT], rp[MAXRT];
#pragma unroll
  for (int k = 0; k < MAXRT; ++k) {
    const int rt = c.wave + NW * k;
    if (rt < c.NT) {
      rp[k] = ct_pack(ld_gf(rep, c.tok0, rt, c.NR, lane));
      if constexpr (REG) xp[k] = ct_pack(xr[k]);
      else xp[k] = ld_g(sv_x1_in, c.tok0, rt, c.NR, lane);
      if constexpr (!REG) { if (store_xb) st_lds(c.XB, rt, xp[k], tok_ok(rt, c), lane); }
    }
  }
#pragma unroll
  for (int mi = 0; mi < 3; ++mi) {
    AFr W;
    loadA(W, m[4 + mi].fa, lane);
    const CT b = ld_vec(m[4 + mi].b, lane);
    if (mi == 0 && sv_x1_out) {   // saved x1 behind the first weight load (in-order vmcnt), not ahead of it
#pragma unroll
      for (int k = 0; k < MAXRT; ++k) {
        const int rt = c.wave + NW * k;
        if (rt < c.NT) st_g(sv_x1_out, c.tok0, rt, c.NR, xp[k], lane);
      }
    }
#pragma unroll
    for (int k = 0; k < MAXRT; ++k) {
      const int rt = c.wave + NW * k;
      if (rt < c.NT) {
        CT t = b;
        mm(t, W, mi == 0 ? rp[k] : xp[k]);
        st_lds(mi == 0 ? c.QB : mi == 1 ? c.KB : c.VB, rt, ct_pack(t), tok_ok(rt, c), lane);
      }
    }
  }
}

// x <- LN(rep + proj(attn(q = W_q rep, k = W_k x, v = W_v x)))   (ma_transformer.py:114)
template <bool SAVE>
__device__ __forceinline__ void cross_attn_fwd_ct(const Mat* m, const LNp& ln, CT* xr, const float* rep, bf16_t* sv_x1,
                                                  bf16_t* sv_a, bf16_t* sv_alo, float* sv_lse, bf16_t* sv_xh,
                                                  float* sv_rs, const Ctx& c) {
  const int lane = c.lane;
  __syncthreads();   // every wave done reading the self-attention's K / V
  cross_proj<true>(m, xr, nullptr, rep, SAVE ? sv_x1 : nullptr, c);
  __syncthreads();
  CP_MARK(24);
  CT O[MAXRT];
  float lse[MAXRT][2];
  attn_fwd_ct(c.QB, c.KB, c.VB, true, nullptr, O, c, lse);
  CP_MARK(25);
  AFr Wp;
  loadA(Wp, m[7].fa, lane);
  const CT bp = ld_vec(m[7].b, lane), gam = ld_vec(ln.g, lane), bet = ld_vec(ln.b, lane);
  CT rp[MAXRT];
#pragma unroll
  for (int k = 0; k < MAXRT; ++k) {
    const int rt = c.wave + NW * k;
    if (rt < c.NT) rp[k] = ld_gf(rep, c.tok0, rt, c.NR, lane);
  }
  if (SAVE) lse_store_fwd(sv_lse, lse, c);   // behind the proj weight / rep loads
#pragma unroll
  for (int k = 0; k < MAXRT; ++k) {
    const int rt = c.wave + NW * k;
    if (rt < c.NT) {
      CTr a, alo;
      if (MDL_SAVE_OLO2) ct_split(O[k], a, alo); else a = ct_pack(O[k]);
      if (SAVE) {
        st_g(sv_a, c.tok0, rt, c.NR, a, lane);
        if (MDL_SAVE_OLO2) st_g(sv_alo, c.tok0, rt, c.NR, alo, lane);
      }
      CT t = ct_add(bp, rp[k]), xh;
      mm(t, Wp, a);
      const float rs = ln_fwd_ct(t, xh, xr[k], gam, bet);
      if (SAVE) {
        st_g(sv_xh, c.tok0, rt, c.NR, ct_pack(xh), lane);
        st_tokf(sv_rs, rt, rs, c);
      }
    }
  }  CP_MARK(26);
}

// backward: dx (w.r.t. the sublayer output) -> d x1 (returned in dx); d rep accumulated into global drep
__device__ __forceinline__ void cross_attn_bwd_ct(const Mat* m, const LNp& ln, CT* dx, const float* rep, float* drep,
                                                  const bf16_t* sv_x1, const bf16_t* sv_a, const bf16_t* sv_alo,
                                                  const float* sv_lse, const bf16_t* sv_xh, const float* sv_rs,
                                                  bool first, const Ctx& c, int vslot) {
  const int lane = c.lane;
  const LseR lse = lse_fetch(sv_lse, c);   // consumed after the recompute phase (latency hidden by passes 1-2)
  CT dres[MAXRT];
  {
    CT dlg, dlb;
    ct_zero(dlg);
    ct_zero(dlb);
    {   // pass 1: LN backward from the saved x-hat / rstd -> ds ; DQ = dY of Wp, XB = X of Wp
      const CT gam = ld_vec(ln.g, lane);
      CTr as[MAXRT], xhs[MAXRT];
      float rsv[MAXRT];
#pragma unroll
      for (int k = 0; k < MAXRT; ++k) {
        const int rt = c.wave + NW * k;
        if (rt < c.NT) {
          as[k] = ld_g(sv_a, c.tok0, rt, c.NR, lane);
          xhs[k] = ld_g(sv_xh, c.tok0, rt, c.NR, lane);
          rsv[k] = ld_tokf(sv_rs, rt, c);
        }
      }
#pragma unroll
      for (int k = 0; k < MAXRT; ++k) {
        const int rt = c.wave + NW * k;
        if (rt < c.NT) {
          const bool ok = tok_ok(rt, c);
          CT ds;
          ln_bwd_ct(dx[k], ct_unpack(xhs[k]), rsv[k], gam, ok, ds, dlg, dlb);
          st_lds(c.DQ, rt, ct_pack(ds), ok, lane);   // dY of Wp
          st_lds(c.XB, rt, as[k], ok, lane);         // X of Wp
          dres[k] = ds;                              // residual path -> d rep
        }
      }
      flush_vec(dlg, c.g(ln.dg), vslot, c);
      flush_vec(dlb, c.g(ln.db), vslot + 1, c);
    }
    {   // pass 2 (Wpᵀ): dO = Wpᵀ ds -> DA; delta = rowsum(dO O) -> DEL (O = X of Wp, in XB)
      AFr Wpb;
      loadA(Wpb, m[7].ba, lane);
#pragma unroll
      for (int k = 0; k < MAXRT; ++k) {
        const int rt = c.wave + NW * k;
        if (rt < c.NT) {
          const CTr alo = MDL_SAVE_OLO2 ? ld_g(sv_alo, c.tok0, rt, c.NR, lane) : ct_zero_r();
          CT da;
          ct_zero(da);
          mm(da, Wpb, ld_lds(c.DQ, rt, lane));
          const bool ok = tok_ok(rt, c);
          const CTr dap = ct_pack(da);
          st_lds(c.DA, rt, dap, ok, lane);
          attn_delta_ct(ld_lds(c.XB, rt, lane), alo, dap, rt, ok, c);
        }
      }
    }
  }
  __syncthreads();
  CP_MARK(4);
  // q / k / v recompute (writes QB / KB / VB only; x1 goes to XB later) before the Wp weight gradient (reads DQ / XB):
  // its atomics drain under the attention, one barrier fewer
  cross_proj<false>(m, nullptr, sv_x1, rep, nullptr, c, false);
  wgrad64(c.DQ, c.XB, m[7], c);
  lse_store(lse, c);
  __syncthreads();
  CP_MARK(6);
  attn_bwd_q_ct(c.QB, c.KB, c.VB, c.DA, c.DQ, true, c);
  __syncthreads();
  CP_MARK(7);
  attn_bwd_kv_ct(c.QB, c.KB, c.VB, c.DA, true, c);
  __syncthreads();
  CP_MARK(8);
  {
    CTr rq[MAXRT], xq[MAXRT];
#pragma unroll
    for (int k = 0; k < MAXRT; ++k) {   // q input (rep) into QB for dW_q, k / v input (x1) into XB for dW_k / dW_v
      const int rt = c.wave + NW * k;
      if (rt < c.NT) {
        rq[k] = ct_pack(ld_gf(rep, c.tok0, rt, c.NR, lane));
        xq[k] = ld_g(sv_x1, c.tok0, rt, c.NR, lane);
      }
    }
#pragma unroll
    for (int k = 0; k < MAXRT; ++k) {
      const int rt = c.wave + NW * k;
      if (rt < c.NT) {
        st_lds(c.QB, rt, rq[k], tok_ok(rt, c), lane);
        st_lds(c.XB, rt, xq[k], tok_ok(rt, c), lane);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < MAXRT; ++k) {
    const int rt = c.wave + NW * k;
    if (rt < c.NT) ct_zero(dx[k]);
  }
  proj3_bwd(m, 4, c.DQ, c.KB, c.VB, dres, dx, c);   // reads DQ / KB / VB: before the barrier and the weight gradients
  {
    CT cur[MAXRT];
#pragma unroll
    for (int k = 0; k < MAXRT; ++k) {   // d rep read-modify-write (each row owned by exactly one wave of one workgroup);
      const int rt = c.wave + NW * k;   // the first block written (the last decoder block) overwrites: no zero fill
      if (rt < c.NT) {
        if (first) ct_zero(cur[k]);
        else cur[k] = ld_gf(drep, c.tok0, rt, c.NR, lane);
      }
    }
#pragma unroll
    for (int k = 0; k < MAXRT; ++k) {
      const int rt = c.wave + NW * k;
      if (rt < c.NT) st_gf(drep, c.tok0, rt, c.NR, ct_add(cur[k], dres[k]), lane);
    }
  }
  __syncthreads();
  CP_MARK(9);
  wgrad64(c.DQ, c.QB, m[4], c);
  {
    const bf16_t* const ys[2] = {c.KB, c.VB};
    const Mat* const ms[2] = {&m[5], &m[6]};
    wgrad64_shared_x<2>(ys, c.XB, ms, c);
  }
  __syncthreads();
  CP_MARK(10);
}

// LDS vector slots of the small weight gradients (wgrad_g_vacc): d W_a (A+1 slots; continuous: A slots, then d b_a),
// d W_h2 (A slots), d b_h2 (1), after
// the 5 + 6 NB LayerNorm / log_std slots; -1 when they do not fit (A > 2 or NB = 3: per-chunk private / atomic flush)
// (MDL_SMALL_WG_VACC: mat_head_ct.h)
__device__ __forceinline__ int small_wg_slot0(const DecP& p, int NB) {
  const int s0 = 5 + 6 * NB;
  return (MDL_SMALL_WG_VACC && p.A <= 2 && s0 + 2 * p.A + 2 <= VSLOTS) ? s0 : -1;
}

// ============================================================================================== forward
template <int NB, bool SAVE, int MA, bool CONT, bool AV>
__device__ __forceinline__ void dec_fwd_tile(const DecP& p, char* smem, int seq0, int nseq) {
  const Ctx c = make_ctx(p, smem, seq0, nseq);
  if (c.nseq <= 0) return;
  zero_pad_rows_fwd(c);
  __syncthreads();
  CP_MARK(0);
  const int lane = c.lane;
  CT xr[MAXRT];
  if (!CONT && !AV && emb_tab_fwd_ok(p)) {   // x0 rows from the per-token table (in QB until the first projection)
    float* X0 = (float*)c.QB;
    emb_table(p, X0, nullptr, nullptr, true, c);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < MAXRT; ++k) {
      const int rt = c.wave + NW * k;
      if (rt < c.NT) {
        const int row = rt * 16 + (lane & 15);
        const int tk = row < c.NR ? dec_token_ct(p, c.tok0 + row, row % c.L) : 0;
        xr[k] = emb_row(X0, tk, lane);
      }
    }
  } else {
    const CT gam = ld_vec(p.lnd_g, lane), bet = ld_vec(p.lnd_b, lane);
#pragma unroll
    for (int k = 0; k < MAXRT; ++k) {
      const int rt = c.wave + NW * k;
      if (rt < c.NT) {
        int tk;
        CT pre = dec_embed_pre_ct<CONT, AV>(p, rt, tk, c), xh;
        gelu_ct(pre);
        ln_fwd_ct(pre, xh, xr[k], gam, bet);
      }
    }
  }
#pragma unroll 1
  for (int b = 0; b < NB; ++b) {
    const Blk& B = p.blk[b];
    Ctx cc = c;
    asm volatile("" : "+v"(cc.lane), "+v"(cc.tid));
    self_attn_fwd_ct<SAVE>(B.m, B.ln[0], xr, true, p.sv[b].xin, p.sv[b].a1, p.sv[b].a1lo, p.sv[b].lse1,
                           p.sv[b].xh[0], p.sv[b].rs + 0 * (size_t)p.Bs * p.L, cc);
    cross_attn_fwd_ct<SAVE>(B.m, B.ln[1], xr, p.rep, p.sv[b].x1, p.sv[b].a2, p.sv[b].a2lo, p.sv[b].lse2,
                            p.sv[b].xh[1], p.sv[b].rs + 1 * (size_t)p.Bs * p.L, cc);
    mlp_fwd_ct<SAVE>(B.m[8], B.m[9], B.ln[2], xr, p.sv[b].x2, p.sv[b].g, p.sv[b].gp, p.sv[b].xh[2], p.sv[b].rs + 2 * (size_t)p.Bs * p.L, cc);
  }
  head_fwd_ct<MA, CONT, AV>(p, xr, SAVE, c);
  CP_MARK(27);
}

#ifndef MDL_CT_BWD_TU
// MA = logit tiles of the action head: 1 (A <= 16: DCML, MPE), 3 (A <= 48: SMAC's 36 actions) or 4 (A <= 64)
template <int NB, bool SAVE, int MA, bool CONT, bool AV = false>
__global__ __launch_bounds__(NTHR, FWD_WGPC) void mat_dec_fwd_ct(DecP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  CP_BEGIN();
  FOR_TILES(p, (dec_fwd_tile<NB, SAVE, MA, CONT, AV>(p, smem, s0, ns)));
  CP_END();
}

#endif  // !MDL_CT_BWD_TU

// ============================================================================================== backward
template <int NB, int MA, bool CONT, bool AV>
__device__ __forceinline__ void dec_bwd_tile(const DecP& p, char* smem, int seq0, int nseq, bool first) {
  const Ctx c = make_ctx(p, smem, seq0, nseq, first);
  if (c.nseq <= 0) return;
  zero_pad_rows(c);
  __syncthreads();
  CP_MARK(0);
  const int lane = c.lane;
  CT dx[MAXRT];
  const int vs0 = small_wg_slot0(p, NB);
  head_bwd_ct<MA, CONT, AV>(p, dx, c, vs0);
#pragma unroll 1
  for (int bb = NB - 1; bb >= 0; --bb) {
    const Blk& B = p.blk[bb];
    Ctx cc = c;
    asm volatile("" : "+v"(cc.lane), "+v"(cc.tid));
    // parameter-vector slots (vacc): 0-1 head LayerNorm, 2-3 embedding LayerNorm, 4 log_std, 5 + 6 bb + 2 k the
    // block's k-th LayerNorm (gamma, beta); then the small weight gradients from vs0 (small_wg_slot0)
    mlp_bwd_ct(B.m[8], B.m[9], B.ln[2], dx, p.sv[bb].x2, p.sv[bb].g, p.sv[bb].gp, p.sv[bb].xh[2], p.sv[bb].rs + 2 * (size_t)p.Bs * p.L, cc,
               9 + 6 * bb);
    cross_attn_bwd_ct(B.m, B.ln[1], dx, p.rep, p.drep, p.sv[bb].x1, p.sv[bb].a2, p.sv[bb].a2lo, p.sv[bb].lse2,
                      p.sv[bb].xh[1], p.sv[bb].rs + 1 * (size_t)p.Bs * p.L, bb == NB - 1, cc, 7 + 6 * bb);
    self_attn_bwd_ct(B.m, B.ln[0], dx, p.sv[bb].xin, p.sv[bb].a1, p.sv[bb].a1lo, p.sv[bb].lse1, p.sv[bb].xh[0],
                     p.sv[bb].rs + 0 * (size_t)p.Bs * p.L, true, cc, 5 + 6 * bb);
  }
  // ---------------- embedding backward: dW_a[:, token] += d pre ; LN_dec params
  if (!CONT && !AV) {
    // discrete tokens: dW_a (64 x (A+1)) = Σ_rows d pre ⊗ onehot(token) — a weight-gradient GEMM on MFMA with the
    // one-hot rows as X (wgrad_g), d pre as a hi/lo bf16 pair; replaces per-element LDS atomics that collided on
    // the (A+1) token rows (16-way address conflicts per wave instruction)
    CT dlg, dlb;
    ct_zero(dlg);
    ct_zero(dlb);
    const CT gam = ld_vec(p.lnd_g, lane), bet = ld_vec(p.lnd_b, lane);
    const int g = lane >> 4;
    const bool tab = emb_tab_bwd_ok(p);   // x-hat / GELU' / rstd per token id in QB + KB (free after the blocks)
    float* XT = (float*)c.QB;
    float* GT = XT + (p.A + 1) * 64;
    float* RT = GT + (p.A + 1) * 64;
    if (tab) {
      emb_table(p, XT, GT, RT, false, c);
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < MAXRT; ++k) {
      const int rt = c.wave + NW * k;
      if (rt < c.NT) {
        const bool ok = tok_ok(rt, c);
        int tk;
        CT egp, xh, de;
        float rs;
        if (tab) {
          const int row = rt * 16 + (lane & 15);
          tk = row < c.NR ? dec_token_ct(p, c.tok0 + row, row % c.L) : 0;
          xh = emb_row(XT, tk, lane);
          egp = emb_row(GT, tk, lane);
          rs = RT[tk];
        } else {
          CT e = dec_embed_pre_ct<CONT>(p, rt, tk, c), yy;
          gelu_ct_both(e, egp);
          rs = ln_fwd_ct(e, xh, yy, gam, bet);
        }
        ln_bwd_ct(dx[k], xh, rs, gam, ok, de, dlg, dlb);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r) de.v[mt][r] = ok ? de.v[mt][r] * egp.v[mt][r] : 0.f;
        CTr dh, dl, oh;
        ct_split(de, dh, dl);
        CT onehot;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r) onehot.v[mt][r] = (ok && 16 * mt + 4 * g + r == tk) ? 1.f : 0.f;
        oh = ct_pack(onehot);
        st_lds(c.DA, rt, dh, ok, lane);   // dY (hi)
        st_lds(c.DQ, rt, dl, ok, lane);   // dY (lo)
        st_lds(c.XB, rt, oh, ok, lane);   // X = one-hot token rows
      }
    }
    flush_vec(dlg, c.g(p.d_lnd_g), 2, c);
    flush_vec(dlb, c.g(p.d_lnd_b), 3, c);
    __syncthreads();
    if (p.d_wa) {
      // hi and lo halves of d pre in one pass: one flush (LDS slots vs0 .. vs0 + A, or one read-modify-write of a
      // private copy per chunk)
      if (vs0 >= 0) wgrad_g_vacc(c.DA, c.XB, c.KP, c.g(p.d_wa), p.A + 1, 64, p.A + 1, nullptr, vs0, -1, c, c.DQ);
      else wgrad_g(c.DA, c.XB, c.KP, c.g(p.d_wa), p.A + 1, 64, p.A + 1, nullptr, c.wave, lane, c.gm, c.DQ);
    }
  } else {
    // continuous actions: dW_a (64 x A) = Σ_rows d pre ⊗ a_prev and db_a = Σ_rows d pre — the same weight-gradient
    // GEMM on MFMA (wgrad_g) with the previous agent's action vector as X (a zero row for a sequence's first token:
    // it reaches db_a only).  Actions are arbitrary fp32 values, so X is a hi / lo bf16 pair like d pre (the lo
    // tile in QB, free after the blocks): Yhi·Xhi + Ylo·Xhi + Yhi·Xlo in one pass, one flush.  No floating-point
    // atomic sums in LDS (fp32 atomicAdd from the 8 waves made the sum's order, and its last bits, vary by run)
    // opaque lane (as for the blocks): this phase's lane-derived addresses are otherwise computed at the kernel's start
    // and held, or spilled, across all of it
    // Available_Continuous: dW_a (64 x (A+1)) = Σ_rows d pre ⊗ (start flag, a_prev), no bias — the same product with
    // X column 0 = 1 on a sequence's first row and columns 1 .. A = the previous agent's action vector on the others
    // (its one-hot head is exact in bf16; the continuous tail needs the lo tile).  A + 1 = 17 puts X column 16 into
    // the second 16-column tile: XW column tiles are filled here, and wgrad_g walks ceil((A + 1) / 16) of them
    constexpr int XW = AV ? 2 : MA;
    Ctx ce = c;
    asm volatile("" : "+v"(ce.lane), "+v"(ce.tid));
    const int lane = ce.lane, g = lane >> 4;
    CT dlg, dlb;
    ct_zero(dlg);
    ct_zero(dlb);
    const CT gam = ld_vec(p.lnd_g, lane), bet = ld_vec(p.lnd_b, lane);
    // rows [16 NT, KP) of QB: no row tile writes them and the attention passes leave their own values there
    for (int i = ce.tid; i < (ce.KP - 16 * ce.NT) * 8; i += NTHR)
      *(uint4*)(ce.QB + (size_t)16 * ce.NT * 64 + (size_t)i * 8) = make_uint4(0, 0, 0, 0);
    // X first, in a pass of its own: the action loads and their split are not live across the LayerNorm backward
#pragma unroll
    for (int k = 0; k < MAXRT; ++k) {
      const int rt = ce.wave + NW * k;
      if (rt < ce.NT) {
        const bool ok = tok_ok(rt, ce);
        const int row = rt * 16 + (lane & 15);
        const bool has_prev = ok && row % ce.L != 0;
        const float* prev = p.act + (has_prev ? src_tok(p.sidx, (size_t)(ce.tok0 + row), ce.L) - 1 : 0) * p.A;
        CT ap;   // a_prev in the feature slots: element 16 mt + 4 g + r (< A); Available_Continuous: shifted by one
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int a = 16 * mt + 4 * g + r;
            if (AV) ap.v[mt][r] = (mt < XW && a <= p.A) ? (a == 0 ? ((ok && !has_prev) ? 1.f : 0.f)
                                                                  : (has_prev ? prev[a > 0 ? a - 1 : 0] : 0.f)) : 0.f;
            else ap.v[mt][r] = (mt < XW && has_prev && a < p.A) ? prev[a] : 0.f;
          }
        CTr ah, al;
        ct_split(ap, ah, al);
        st_lds(ce.XB, rt, ah, ok, lane);   // X (hi) = previous-action rows
        st_lds(ce.QB, rt, al, ok, lane);   // X (lo)
      }
    }
#pragma unroll
    for (int k = 0; k < MAXRT; ++k) {
      const int rt = ce.wave + NW * k;
      if (rt < ce.NT) {
        const bool ok = tok_ok(rt, ce);
        int tk;
        CT e = dec_embed_pre_ct<CONT, AV>(p, rt, tk, ce), egp, xh, yy, de;
        gelu_ct_both(e, egp);
        const float rs = ln_fwd_ct(e, xh, yy, gam, bet);
        ln_bwd_ct(dx[k], xh, rs, gam, ok, de, dlg, dlb);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r) de.v[mt][r] = ok ? de.v[mt][r] * egp.v[mt][r] : 0.f;
        CTr dh, dl;
        ct_split(de, dh, dl);
        st_lds(ce.DA, rt, dh, ok, lane);   // dY (hi)
        st_lds(ce.DQ, rt, dl, ok, lane);   // dY (lo)
      }
    }
    flush_vec(dlg, ce.g(p.d_lnd_g), 2, ce);
    flush_vec(dlb, ce.g(p.d_lnd_b), 3, ce);
    __syncthreads();
    if (AV) {   // W_a [64][A + 1] (row stride A + 1), no bias gradient; A >= 3: never the LDS slots
      if (p.d_wa) wgrad_g(ce.DA, ce.XB, ce.KP, ce.g(p.d_wa), p.A + 1, 64, p.A + 1, nullptr, ce.wave, lane, ce.gm, ce.DQ, ce.QB);
    } else if (p.d_wa || p.d_ba) {
      // W_a [64][A] (row stride A) and b_a: LDS slots vs0 .. vs0 + A - 1 and vs0 + A (the A + 1 slots the discrete
      // table takes), or one read-modify-write of a private copy per chunk
      if (vs0 >= 0) wgrad_g_vacc(ce.DA, ce.XB, ce.KP, ce.g(p.d_wa), p.A, 64, p.A, ce.g(p.d_ba), vs0, vs0 + p.A, ce, ce.DQ, ce.QB);
      else wgrad_g(ce.DA, ce.XB, ce.KP, ce.g(p.d_wa), p.A, 64, p.A, ce.g(p.d_ba), ce.wave, lane, ce.gm, ce.DQ, ce.QB);
    }
  }
  CP_MARK(30);
}

#ifdef MDL_CT_BWD_TU
template <int NB, int MA, bool CONT, bool AV = false>
__global__ __launch_bounds__(NTHR, WGPC) void mat_dec_bwd_ct(DecP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  CP_BEGIN();
  vacc_begin(p, smem);
  FOR_TILES(p, (dec_bwd_tile<NB, MA, CONT, AV>(p, smem, s0, ns, it_ == 0)));
  vacc_end(p, smem);
  CP_END();
}

#endif  // MDL_CT_BWD_TU

}  // namespace

// ============================================================================================== host API
#ifndef MDL_CT_BWD_TU
template <int MA, bool CONT, bool AV = false>
static int dec_fwd_ct(const DecP* p, int NB, int save, hipStream_t st) {
  if (NB == 1) return save ? launch_ct(mat_dec_fwd_ct<1, true, MA, CONT, AV>, p, true, st) : launch_ct(mat_dec_fwd_ct<1, false, MA, CONT, AV>, p, true, st);
  if (NB == 2) return save ? launch_ct(mat_dec_fwd_ct<2, true, MA, CONT, AV>, p, true, st) : launch_ct(mat_dec_fwd_ct<2, false, MA, CONT, AV>, p, true, st);
  if (NB == 3) return save ? launch_ct(mat_dec_fwd_ct<3, true, MA, CONT, AV>, p, true, st) : launch_ct(mat_dec_fwd_ct<3, false, MA, CONT, AV>, p, true, st);
  return -3;
}
// MA = logit tiles of the action head (1: A <= 16, 3: A <= 48 — SMAC's 36 actions, 4: A <= 64); the continuous
// action type is its own instantiation (its Normal-head / Linear-embedding code kept out of the discrete kernels'
// instruction stream), and so is Available_Continuous (3 <= A <= 16: one logit tile)
MDL_API int mdl_mat_dec_fwd_ct(const DecP* p, int NB, int save, hipStream_t st) {
  if (p->A > 64 || p->A < 1) return -1;
  if (p->avail) return (p->cont || p->A < 3 || p->A > 16) ? -1 : dec_fwd_ct<1, false, true>(p, NB, save, st);
  if (p->cont) return p->A <= 16 ? dec_fwd_ct<1, true>(p, NB, save, st) : dec_fwd_ct<4, true>(p, NB, save, st);
  if (p->A <= 16) return dec_fwd_ct<1, false>(p, NB, save, st);
  return p->A <= 48 ? dec_fwd_ct<3, false>(p, NB, save, st) : dec_fwd_ct<4, false>(p, NB, save, st);
}
#else
template <int MA, bool CONT, bool AV = false>
static int dec_bwd_ct(const DecP* p, int NB, hipStream_t st) {
  if (NB == 1) return launch_ct(mat_dec_bwd_ct<1, MA, CONT, AV>, p, false, st);
  if (NB == 2) return launch_ct(mat_dec_bwd_ct<2, MA, CONT, AV>, p, false, st);
  if (NB == 3) return launch_ct(mat_dec_bwd_ct<3, MA, CONT, AV>, p, false, st);
  return -3;
}

MDL_API int mdl_mat_dec_bwd_ct(const DecP* p, int NB, hipStream_t st) {
  if (p->A > 64 || p->A < 1 || 2 * p->NRP * 128 < (p->A + 1) * 256) return -1;
  if (p->avail) return (p->cont || p->A < 3 || p->A > 16) ? -1 : dec_bwd_ct<1, false, true>(p, NB, st);
  if (p->cont) return p->A <= 16 ? dec_bwd_ct<1, true>(p, NB, st) : dec_bwd_ct<4, true>(p, NB, st);
  if (p->A <= 16) return dec_bwd_ct<1, false>(p, NB, st);
  return p->A <= 48 ? dec_bwd_ct<3, false>(p, NB, st) : dec_bwd_ct<4, false>(p, NB, st);
}
#endif  // MDL_CT_BWD_TU

#ifdef MDL_CT_PROF
MDL_API int MDL_CAT(mdl_ctprof_dec, MDL_CT_TU_SUFFIX)(unsigned long long* out, int reset) {
  if (reset) {
    unsigned long long z[64] = {0};
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_ctprof), z, sizeof(z));
  }
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ctprof), sizeof(unsigned long long) * 64, 0, hipMemcpyDeviceToHost);
}
#endif
