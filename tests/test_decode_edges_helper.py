"""Helpers of tests/test_gpu_decode_edges.py and their CPU self-tests: the fp64 replay of a decode on the kernel's own
actions, the per-decision checks against it, the two weight sets, and the enumeration of the host dispatch code
(csrc/mat_decode.hip mdl_mat_decode, csrc/mat_decode_wave.hip mdl_decode_wave_plan / mdl_decode_spec_plan) over
n_block x L x act_dim that names the kernel instantiation a call launches."""
import contextlib
import copy
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from mat_dcml_amd.models import act
from mat_dcml_amd.models.mat import MultiAgentTransformer
from test_train_edges_helper import token_bound, token_errors, token_stat

CONT = ("Continuous", "Continous")
AVAIL = ("Available_Continuous", "Available_Continous")
U_TOP = float(torch.tensor((2.0 ** 24 - 0.5) / 2.0 ** 24, dtype=torch.float64).float())   # u01_open's maximum as fp32: 1.0
U_NEAR = 1.0 - 2.0 ** -24                                                                 # the largest fp32 below 1.0
NORMAL_LP_ATOL = 1e-5     # lp_k against normal_logprob(x_k, implied mean, std): an fp32 identity


@contextlib.contextmanager
def float_keeps_fp64():
    """The eager model casts logits / attention scores with ``.float()``; an fp64 reference must not round there."""
    orig = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self if self.dtype == torch.float64 else orig(self, *a, **k)
    try:
        yield
    finally:
        torch.Tensor.float = orig


@contextlib.contextmanager
def eager_in_fp64():
    """``float_keeps_fp64`` plus fp64 for the output tensors ``autoregressive_act`` allocates with the default dtype."""
    saved = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        with float_keeps_fp64():
            yield
    finally:
        torch.set_default_dtype(saved)


# ------------------------------------------------------------------------------------------------ models and inputs
def make_model(kind, A, L, nb, dev="cpu", seed=0, sharp=False, od=7):
    """The model's own (orthogonal) initialisation with every bias, LayerNorm parameter and log_std moved off its
    constant; ``sharp``: the head's last layer scaled so that the logits span roughly +-10 (a trained policy), and
    the decoder's attention matrices scaled to gain 0.5 so that the logits depend on the KV caches.  The
    last layer's rows are orthogonal of norm 0.01 and its input is a LayerNorm output of unit variance, so the logits
    have standard deviation 0.01 x the scale: 350 gives 3.5."""
    torch.manual_seed(seed)
    m = MultiAgentTransformer(L + 1, od, A, L, nb, 64, 2, action_type=kind, semi_index=-1)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("log_std"):
                p.copy_(1.0 + 0.5 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1 and n.endswith("weight"):          # LayerNorm gain
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1:                                    # every bias (Linear and LayerNorm)
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
        if sharp:
            m.decoder.head[3].weight.mul_(350.0)
            m.decoder.head[3].bias.mul_(10.0)
            # a trained policy attends: at the initial gain of 0.01 an attention output is 1e-4 of the residual it is
            # added to and no logit depends visibly on an earlier action or on a cache row.  Gain 0.5 makes it a
            # quarter of the residual, with scores of order 1
            for blk in m.decoder.blocks:
                for att in (blk.attn1, blk.attn2):
                    for lin in (att.key, att.query, att.value, att.proj):
                        lin.weight.mul_(50.0)
    return m.to(dev)


def make_inputs(m, B, L, A, dev, seed=1, od=7, ava_mode="mixed", n_cat=None):
    """obs, rep (the fp32 encoder's), ava and explicit draws.  ``mixed`` availability: random with at least one action
    per row; per env, row (b + 1) % L allows only action 0, row (b + 2) % L only action A - 1 and row (b + 3) % L
    everything but action A - 1.  Draws: u of exactly u01_open's maximum (1.0 in fp32) on row b % L of the even envs
    and on the rows without action A - 1, the largest fp32 below 1.0 on row b % L of the odd envs."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.rand(B, L, od, generator=g)
    u = torch.rand(B, L, generator=g)
    n = torch.randn(B, L, A, generator=g)
    ava = None
    K = n_cat or A        # Available_Continuous: the categorical part is the first two columns
    if ava_mode != "none":
        ava = (torch.rand(B, L, K, generator=g) < 0.6).float()
        first = torch.randint(0, K, (B, L), generator=g)
        ava.scatter_(-1, first.unsqueeze(-1), 1.0)
        for b in range(B):
            ava[b, (b + 1) % L] = 0
            ava[b, (b + 1) % L, 0] = 1
            if L > 1:
                ava[b, (b + 2) % L] = 0
                ava[b, (b + 2) % L, K - 1] = 1
            if L > 2 and K > 1:
                ava[b, (b + 3) % L] = 1
                ava[b, (b + 3) % L, K - 1] = 0
                u[b, (b + 3) % L] = U_TOP
        ava = torch.cat([ava, torch.ones(B, L, A - K)], -1)
    for b in range(B):
        u[b, b % L] = U_TOP if b % 2 == 0 else U_NEAR
    obs, u, n = obs.to(dev), u.to(dev), n.to(dev)
    ava = None if ava is None else ava.to(dev)
    with torch.no_grad():
        _, rep = m.encoder(None, obs)
    return obs, rep.float().contiguous(), ava, {"u": u, "n": n}


# ------------------------------------------------------------------------------------------------ the fp64 replay
@torch.no_grad()
def replay_logits(m64, rep64, obs, actions, deterministic=False, stride=1):
    """``models/act.autoregressive_act`` with ``emit`` taking row i's action from ``actions`` instead of sampling it:
    the same decoder inputs, the same ``block_schedule`` and the same ``decode_rows`` calls over [lo, e).  Returns the
    head outputs of every row, (B, L, A), in the model's dtype."""
    dec = m64.decoder
    B, L, _ = rep64.shape
    A = m64.action_dim
    kind = m64.action_type
    dt, dev = rep64.dtype, rep64.device
    n_disc = act.n_discrete_agents(m64, L)
    actions = actions.to(dt)
    cont_in = kind in CONT
    shifted = torch.zeros(B, L, A if cont_in else A + 1, device=dev, dtype=dt)
    if not cont_in:
        shifted[:, 0, 0] = 1
    out = torch.zeros(B, L, A, device=dev, dtype=dt)
    cache = dec.new_cache(B, L, dev, dt)

    def emit(i, logit):
        out[:, i] = logit
        if i + 1 >= L:
            return
        if cont_in:
            shifted[:, i + 1] = actions[:, i]
        elif kind in AVAIL:
            shifted[:, i + 1, 1:] = actions[:, i]
        elif i < n_disc:
            shifted[:, i + 1, 1:] = F.one_hot(actions[:, i, 0].long(), A).to(dt)
        else:
            # the ratio agent feeds its whole sampled vector; only its last column is an output.  It is the last
            # row under semi_index -1, so nothing reads this input
            shifted[:, i + 1, 1:] = actions[:, i, :1].expand(B, A)

    with float_keeps_fp64():
        if kind in AVAIL or not deterministic or stride <= 1:
            for i in range(L):
                emit(i, dec.decode_rows(shifted[:, i:i + 1], rep64[:, i:i + 1], cache, i)[:, 0])
        else:
            prev_s = -1
            for (s, e) in act.block_schedule(L, n_disc, stride):
                lo = prev_s + 1 if prev_s >= 0 else 0
                lo = min(lo, s)
                logits = dec.decode_rows(shifted[:, lo:e], rep64[:, lo:e], cache, lo)
                for i in range(s, e):
                    emit(i, logits[:, i - lo])
                prev_s = s
    return out


def double_model(m):
    return copy.deepcopy(m).double()


# ------------------------------------------------------------------------------------------------ heads in fp64
def split_heads(kind, A, L, logits, actions, lps, ava, rand, std):
    """The categorical and the Normal part of a decode's outputs, everything fp64 on the CPU.
    cat: (z masked logits (N, K), a (N,), lp (N,), u (N,), available (N, K)) or None;
    nrm: (mean (M,), x (M,), lp (M,), n (M,), std (M,)) or None."""
    d = lambda t: None if t is None else t.detach().double().cpu()   # noqa: E731
    logits, actions, lps, ava, std = d(logits), d(actions), d(lps), d(ava), d(std)
    B = logits.shape[0]
    u = d(rand["u"]) if rand is not None else torch.zeros(B, L, dtype=torch.float64)
    n = d(rand["n"]) if rand is not None and "n" in rand else torch.zeros(B, L, A, dtype=torch.float64)
    cat = nrm = None
    if kind in CONT:
        nrm = (logits, actions, lps, n, std.expand(B, L, A))
    elif kind in AVAIL:
        av = torch.ones(B, L, 2, dtype=torch.float64) if ava is None else ava[..., :2]
        assert bool(((actions[..., :2] == 0) | (actions[..., :2] == 1)).all()) and bool((actions[..., :2].sum(-1) == 1).all())
        cat = (logits[..., :2].masked_fill(av == 0, act.MASK_LOGIT), actions[..., :2].argmax(-1), lps[..., 0], u, av)
        nrm = (logits[..., 2:], actions[..., 2:], lps[..., 1:], n[..., 2:], std[2:].expand(B, L, A - 2))
    else:
        nd = L if kind == "Discrete" else L - 1
        if nd > 0:
            av = torch.ones(B, nd, A, dtype=torch.float64) if ava is None else ava[:, :nd]
            cat = (logits[:, :nd].masked_fill(av == 0, act.MASK_LOGIT), actions[:, :nd, 0].long(), lps[:, :nd, 0],
                   u[:, :nd], av)
        if nd < L:
            nrm = (logits[:, nd:, A - 1], actions[:, nd:, 0], lps[:, nd:, 0], n[:, nd:, A - 1],
                   std[A - 1].expand(B, L - nd))
    if cat is not None:
        K = cat[0].shape[-1]
        cat = (cat[0].reshape(-1, K), cat[1].reshape(-1), cat[2].reshape(-1), cat[3].reshape(-1), cat[4].reshape(-1, K))
    if nrm is not None:
        nrm = tuple(t.reshape(-1) for t in nrm)
    return cat, nrm


def check_decode(kind, A, L, logits64, yard_logits, actions, lps, ava, rand, std, deterministic):
    """Every check of one decode call against the fp64 replay ``logits64`` of its own actions, with the bounds from
    the yardstick's logits on the same actions.  Returns (stats, failures): stats = {lp: (kernel statistic, yardstick,
    bound), mean: (...)}; failures = a list of messages, empty when every token and every decision passes."""
    cat, nrm = split_heads(kind, A, L, logits64, actions, lps, ava, rand, std)
    ycat, ynrm = split_heads(kind, A, L, yard_logits, actions, lps, ava, rand, std)
    stats, fails = {}, []
    if cat is not None:
        z, a, lp_k, u, av = cat
        if bool(((a < 0) | (a >= z.shape[-1])).any()):
            return stats, [f"action out of range: {a.min().item()} .. {a.max().item()}"]
        ok_av = av.gather(-1, a.unsqueeze(-1)).squeeze(-1) == 1
        if not bool(ok_av.all()):
            fails.append(f"masking: {(~ok_av).sum().item()} unavailable actions chosen, first at token "
                         f"{(~ok_av).nonzero()[0].item()} (u {u[~ok_av][0].item():.9g})")
        lp64 = torch.log_softmax(z, -1)
        ref = lp64.gather(-1, a.unsqueeze(-1)).squeeze(-1)
        yard = torch.log_softmax(ycat[0], -1).gather(-1, a.unsqueeze(-1)).squeeze(-1)
        s, y = token_stat(lp_k[ok_av], ref[ok_av]), token_stat(yard[ok_av], ref[ok_av])
        d = token_bound(y)
        stats["lp"] = (s, y, d)
        if not s <= d:
            e = token_errors(lp_k, ref)
            fails.append(f"log-prob: statistic {s:.3e} > bound {d:.3e} (yardstick {y:.3e}) at {(e > d).sum().item()} "
                         f"tokens, first {(e > d).nonzero()[0].item() if bool((e > d).any()) else 'nan'}")
        fails += decision_failures(lp64, a, u, d, deterministic)
    if nrm is not None:
        mean64, x, lp_k, n, sd = nrm
        implied = x if deterministic else x - sd * n
        s, y = token_stat(implied, mean64), token_stat(ynrm[0], mean64)
        b = token_bound(y)
        stats["mean"] = (s, y, b)
        if not s <= b:
            e = token_errors(implied, mean64)
            fails.append(f"Normal mean: statistic {s:.3e} > bound {b:.3e} (yardstick {y:.3e}) at "
                         f"{(e > b).sum().item()} entries")
        ident = (lp_k - act.normal_logprob(x, implied, sd)).abs()
        stats["normal_lp_identity"] = ident.max().item()
        if not bool((ident <= NORMAL_LP_ATOL).all()):
            fails.append(f"Normal log-prob identity: max {ident.max().item():.3e} > {NORMAL_LP_ATOL:g} at "
                         f"{(~(ident <= NORMAL_LP_ATOL)).sum().item()} entries")
    return stats, fails


def decision_failures(lp64, a, u, d, deterministic):
    """Deterministic: the chosen action is within 2 d of the best.  Sampled: cdf64[a - 1] - d < u <= cdf64[a] + d."""
    idx = a.unsqueeze(-1)
    if deterministic:
        regret = lp64.max(-1).values - lp64.gather(-1, idx).squeeze(-1)
        bad = ~(regret <= 2 * d)
        return [f"argmax: {bad.sum().item()} decisions with regret > {2 * d:.3e}, worst {regret.max().item():.3e} at "
                f"token {regret.argmax().item()}"] if bool(bad.any()) else []
    cdf = torch.cumsum(lp64.exp(), -1)
    hi = cdf.gather(-1, idx).squeeze(-1)
    lo = torch.where(a > 0, cdf.gather(-1, (idx - 1).clamp_min(0)).squeeze(-1), torch.zeros_like(hi))
    bad = ~((lo - d < u) & (u <= hi + d))
    if bool(bad.any()):
        t = bad.nonzero()[0].item()
        return [f"sampling: {bad.sum().item()} unexplained decisions, first at token {t}: u {u[t].item():.9g} action "
                f"{a[t].item()} edges ({lo[t].item():.9g}, {hi[t].item():.9g}] d {d:.3e}"]
    return []


# ------------------------------------------------------------------------------------------------ dispatch enumeration
SMALL_AD = 4    # csrc/mat_decode.hip: up to this many actions the heads keep the logits in registers
L_SCAN = 300    # the enumeration's upper end: beyond what the geometry accepts for any n_block (269 at n_block 1)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def n_tok_of(kind, A):
    return 2 if kind in CONT or kind in AVAIL else A + 2


def native_lib():
    """The HIP library (its plan functions are host code: no GPU needed).  Skipped only where there is neither a built
    library nor a compiler to build one; a library that fails to build or to load fails the test."""
    from mat_dcml_amd.ops import kernels, mat_fused   # noqa: F401  (mat_fused declares the plan signatures)
    if not os.path.exists(kernels.LIB_PATH) and not os.path.exists(HIPCC):
        pytest.skip("no built native library and no hipcc")
    return kernels.lib()


def dec_params(nb, L, A, kind="Discrete", wave=True, deterministic=False, stride=1, B=8):
    """A DecParams filled as ``mat_fused.decode`` fills it, with dummy non-null pointers: for the plan queries only."""
    from mat_dcml_amd.ops import mat_fused
    cont, avail = kind in CONT, kind in AVAIL
    nd = L if kind == "Discrete" else 0 if cont or avail else L - 1
    p = mat_fused.DecParams()
    for n in ("wpack", "bias", "lnp", "emb", "wh2", "bh2", "stdv", "rep", "ava", "rnd_u", "rnd_n", "out_a", "out_lp"):
        setattr(p, n, 64)
    if cont or avail:
        p.wa = p.ba = p.lnd = 64
    else:
        p.qkv0 = p.hfold = 64
    p.wfa = 64 if wave else None
    p.B, p.L, p.act_dim, p.n_disc, p.stride, p.deterministic = B, L, A, nd, stride if deterministic else 1, int(deterministic)
    p.epw, p.rmax, p.n_tok, p.tok_zero, p.cont, p.avail_cont = 1, 16, n_tok_of(kind, A), A + 1, int(cont or avail), int(avail)
    return p


def plan_path(lib, nb, L, A, kind="Discrete", wave=True, spec=True, **kw):
    """The path string ``mat_fused.decode`` reports for this call, from the library's plan functions (nothing is
    launched).  The library's speculative switch is put back to ``mat_fused.SPEC_DECODE`` afterwards."""
    from mat_dcml_amd.ops import mat_fused
    mat_fused.set_spec_enabled(spec)
    try:
        return mat_fused.wave_path(dec_params(nb, L, A, kind, wave, **kw), nb)
    finally:
        mat_fused.set_spec_enabled(mat_fused.SPEC_DECODE)


def plan_4wave(lib, nb, L, A, kind="Discrete"):
    """(stage, q2pre) of the 4-wave launch ``mdl_mat_decode`` makes for this call (mdl_decode_4wave_plan: the function
    the launch itself takes them from), or None when the caches do not fit."""
    r = lib.mdl_decode_4wave_plan(ctypes.byref(dec_params(nb, L, A, kind)), nb)
    return None if r < 0 else (r & 1, (r >> 1) & 1)


def instantiation(lib, nb, L, A, kind="Discrete", **kw):
    """Name of the kernel instantiation the call launches, or None when the geometry rejects it."""
    if lib.mdl_mat_decode_geometry(nb, L, 1) <= 0:
        return None
    path = plan_path(lib, nb, L, A, kind, **kw)
    wide = A > SMALL_AD
    if path.startswith("spec"):
        ns = (A + 15) // 16
        nreg = int(path.split("nreg=")[1].split(",")[0].rstrip(")"))
        lay = "IND+Q2F" if "q2inline" in path else "IND" if "tokrows" in path else "plain"
        head = f"NS={ns}, MA=3" if wide else ("MA=1, 16-candidate" if A > 2 else "MA=1, pair")
        return f"spec<NB=2, {head}, NREG={nreg}, {lay}>"
    if path.startswith("wave"):
        nreg = int(path.split("nreg=")[1].rstrip(")"))
        return f"wave<NB={nb}, NREG={nreg}, MA={1 if not wide else 3 if A <= 48 else 4}>"
    stage, q2pre = plan_4wave(lib, nb, L, A, kind)
    return f"4wave<NB={nb}, STAGE={stage}> q2pre={q2pre}"


def enumerate_dispatch(lib, kind="Discrete", **kw):
    """{instantiation: smallest (n_block, L, A) that reaches it} over n_block 1..3 x every L the geometry accepts x A 1..64,
    smallest L first, then smallest A (the one-wave and speculative kernels end at L = 192 by their own gate)."""
    first = {}
    for nb in (1, 2, 3):
        for L in range(1, L_SCAN + 1):
            if lib.mdl_mat_decode_geometry(nb, L, 1) <= 0:
                continue
            for A in range(1, 65):
                first.setdefault(instantiation(lib, nb, L, A, kind, **kw), (nb, L, A))
    return first


# ------------------------------------------------------------------------------------------------ the GPU cases
def _kind(A):
    return "Semi_Discrete" if A == 2 else "Discrete"


# 4-wave kernel (one-wave path off): per (n_block, A) an L with stage and q2pre on, then the smallest L of every other
# (stage, q2pre) combination in the order they appear, then the largest L the geometry accepts (269 / 134 / 88); at
# n_block 1 also L = 192, the one-wave kernel's limit
W4_L = {(1, 2): [(6, 1, 1), (145, 1, 0), (170, 0, 1), (192, 0, 1), (213, 0, 0), (269, 0, 0)],
        (1, 36): [(6, 1, 1), (67, 1, 0), (77, 0, 1), (192, 0, 1), (213, 0, 0), (269, 0, 0)],
        (2, 2): [(6, 1, 1), (83, 1, 0), (103, 0, 1), (105, 0, 0), (134, 0, 0)],
        (2, 36): [(6, 1, 1), (42, 1, 0), (51, 0, 1), (105, 0, 0), (134, 0, 0)],
        (3, 2): [(6, 1, 1), (58, 1, 0), (73, 0, 0), (88, 0, 0)], (3, 36): [(6, 1, 1), (30, 1, 0), (38, 0, 1), (68, 0, 0), (88, 0, 0)]}
# one-wave kernel (speculative path off): per (n_block, A) the (L, NREG) pairs: L = 5 for the instantiation that L = 1
# already selects (L = 1 itself is in the degenerate cases), the smallest L of every further NREG, and the largest L
# the one-wave kernel takes for that head (192 by its gate, or less where its LDS carve ends first)
WV_L = {(1, 2): [(5, 0), (149, 2), (174, 4), (192, 4)], (1, 5): [(5, 0), (148, 2), (174, 4), (192, 4)],
        (1, 48): [(5, 0), (123, 2), (148, 4), (173, 4)], (1, 49): [(5, 0), (122, 2), (148, 4), (172, 4)],
        (1, 64): [(5, 0), (113, 2), (139, 4), (163, 4)],
        (2, 2): [(5, 0), (14, 2), (27, 4), (39, 6), (51, 6)], (2, 5): [(5, 0), (14, 2), (26, 4), (39, 6), (51, 6)],
        (2, 48): [(5, 2), (14, 4), (26, 6), (38, 6)], (2, 49): [(5, 2), (13, 4), (26, 6), (38, 6)],
        (2, 64): [(5, 2), (9, 4), (22, 6), (33, 6)]}
# speculative kernel (default switches, n_block 2): per A the (L, path) pairs, same rule
SP_L = {2: [(5, "spec(nreg=0)"), (51, "spec(nreg=8)"), (102, "spec(nreg=6, tokrows)"), (111, "spec(nreg=6, tokrows, q2inline)")],
        3: [(5, "spec(nreg=0)"), (50, "spec(nreg=8)"), (101, "spec(nreg=6, tokrows)"), (110, "spec(nreg=6, tokrows, q2inline)")],
        4: [(5, "spec(nreg=0)"), (49, "spec(nreg=8)"), (100, "spec(nreg=6, tokrows)"), (109, "spec(nreg=6, tokrows, q2inline)")],
        5: [(5, "spec(nreg=6)")], 16: [(5, "spec(nreg=6)")], 17: [(5, "spec(nreg=6)")], 32: [(5, "spec(nreg=6)")],
        33: [(5, "spec(nreg=6)")], 48: [(5, "spec(nreg=6)")]}
# mdl_decode_spec_layout forced at a small L: the only way to the token-table layout with 4 register matrices
SP_FORCED = [(2, 12, 1, "spec(nreg=4, tokrows)"), (3, 12, 1, "spec(nreg=4, tokrows)"),
             (2, 12, 2, "spec(nreg=6, tokrows, q2inline)"), (3, 12, 2, "spec(nreg=6, tokrows, q2inline)")]


def launch_cases():
    """{id: dict(kind, A, L, nb, mode, path, layout)}: mode '4wave' = one-wave path off, 'wave' = speculative path off,
    'spec' = the default switches."""
    out = {}
    for (nb, A), ls in W4_L.items():
        for L, stg, q2 in ls:
            out[f"4wave-nb{nb}-A{A}-L{L}"] = dict(kind=_kind(A), A=A, L=L, nb=nb, mode="4wave", path="4wave", layout=0,
                                                  inst=f"4wave<NB={nb}, STAGE={stg}> q2pre={q2}")
    for (nb, A), ls in WV_L.items():
        for L, nreg in ls:
            out[f"wave-nb{nb}-A{A}-L{L}"] = dict(kind=_kind(A), A=A, L=L, nb=nb, mode="wave", path=f"wave(nreg={nreg})", layout=0)
    for A, ls in SP_L.items():
        for L, path in ls:
            out[f"spec-A{A}-L{L}"] = dict(kind=_kind(A), A=A, L=L, nb=2, mode="spec", path=path, layout=0)
    for A, L, layout, path in SP_FORCED:
        out[f"spec-A{A}-L{L}-layout{layout}"] = dict(kind=_kind(A), A=A, L=L, nb=2, mode="spec", path=path, layout=layout)
    return out


MODES = {"4wave": (False, False), "wave": (True, False), "spec": (True, True)}   # (WAVE_DECODE, SPEC_DECODE)


# ------------------------------------------------------------------------------------------------ CPU self-tests
def _cpu_case(kind, A=3, L=7, B=4, nb=2, sharp=True):
    m = make_model(kind, A, L, nb, sharp=sharp)
    obs, rep, ava, rand = make_inputs(m, B, L, A, "cpu", ava_mode="mixed" if kind not in CONT else "none",
                                      n_cat=2 if kind in AVAIL else None)
    rand = {k: v.double() for k, v in rand.items()}
    return m.double(), obs.double(), rep.double(), None if ava is None else ava.double(), rand


@pytest.mark.parametrize("kind,A", [("Discrete", 5), ("Semi_Discrete", 2), ("Continuous", 3), ("Available_Continuous", 4)])
@pytest.mark.parametrize("stride", [1, 3, 20])
@pytest.mark.parametrize("det", [False, True])
def test_replay_of_own_actions_reproduces_autoregressive_act(kind, A, stride, det):
    """fp64: the replay of ``autoregressive_act``'s own actions gives the log-probs it returned, to 1e-12."""
    L = 9
    m, obs, rep, ava, rand = _cpu_case(kind, A, L)
    with eager_in_fp64():
        a, lp = act.autoregressive_act(m, rep, obs, ava, det, stride, rand)
        lg = replay_logits(m, rep, obs, a, det, stride)
        lp2, _ = act.heads_logprob_entropy(m, lg, a, ava)
    assert lg.dtype == lp.dtype == torch.float64
    assert (lp2 - lp).abs().max().item() < 1e-12, (lp2 - lp).abs().max().item()
    std = None if kind == "Discrete" else m.action_std()
    st, fails = check_decode(kind, A, L, lg, lg, a, lp, ava, rand, std, det)
    assert not fails, fails


@pytest.mark.parametrize("kind,A", [("Discrete", 5), ("Semi_Discrete", 2), ("Continuous", 3), ("Available_Continuous", 4)])
def test_replay_at_stride_1_is_the_teacher_forced_pass(kind, A):
    L = 9
    m, obs, rep, ava, rand = _cpu_case(kind, A, L)
    with eager_in_fp64():
        a, _ = act.autoregressive_act(m, rep, obs, ava, False, 1, rand)
        lg = replay_logits(m, rep, obs, a)
        tf = m.decoder(act.shifted_from_actions(m, a).double(), rep, obs)
    assert (lg - tf).abs().max().item() < 1e-12, (lg - tf).abs().max().item()


def test_stride_replay_differs_from_the_teacher_forced_pass():
    """The stride replay is its own computation (in-block rows see zero inputs): not the parallel pass."""
    m, obs, rep, ava, rand = _cpu_case("Discrete", 5, 9)
    with eager_in_fp64():
        a, _ = act.autoregressive_act(m, rep, obs, ava, True, 3, rand)
        lg = replay_logits(m, rep, obs, a, True, 3)
        tf = m.decoder(act.shifted_from_actions(m, a).double(), rep, obs)
    assert (lg - tf).abs().max().item() > 0.1


def _noisy(ref, sigma, seed):
    g = torch.Generator().manual_seed(seed)
    return ref + sigma * torch.randn(ref.shape, generator=g, dtype=torch.float64)


def test_checkers_reject_planted_errors():
    """The unperturbed outputs pass; one log-prob moved by 20 x the bound, one sampled action replaced by its neighbour
    where u is far from the CDF edge, one argmax replaced by the runner-up at a clear gap each fail, and so does one
    unavailable action, one Normal mean off by 20 x its bound and one Normal log-prob of another dimension's std."""
    kind, A, L, B = "Discrete", 5, 9, 6
    m, obs, rep, ava, rand = _cpu_case(kind, A, L, B)
    for det in (False, True):
        with eager_in_fp64():
            a, lp = act.autoregressive_act(m, rep, obs, ava, det, 1, rand)
            lg = replay_logits(m, rep, obs, a, det)
        yard = _noisy(lg, 2.0 ** -9, 5)
        st, fails = check_decode(kind, A, L, lg, yard, a, lp, ava, rand, None, det)
        assert not fails and st["lp"][0] < 1e-12 and st["lp"][2] == token_bound(st["lp"][1]), (st, fails)
        d = st["lp"][2]
        bad = lp.clone()
        bad[3, 4, 0] += 20 * d * (1 + lp[3, 4, 0].abs())
        _, fails = check_decode(kind, A, L, lg, yard, a, bad, ava, rand, None, det)
        assert len(fails) == 1 and fails[0].startswith("log-prob") and " 1 tokens" in fails[0], fails
        # a decision with a clear margin: u at least 0.05 inside its CDF interval / a gap of 0.5 nats to the runner-up
        z = lg.masked_fill(ava == 0, act.MASK_LOGIT)
        lsm = torch.log_softmax(z, -1)
        cdf = torch.cumsum(lsm.exp(), -1)
        found = None
        for b in range(B):
            for i in range(L):
                k = int(a[b, i, 0])
                if det:
                    top = lsm[b, i].topk(2)
                    if ava[b, i].sum() >= 2 and top.values[0] - top.values[1] > 0.5:
                        found = (b, i, int(top.indices[1]))
                else:
                    lo = cdf[b, i, k - 1].item() if k > 0 else 0.0
                    nb_ = k + 1 if k + 1 < A and ava[b, i, k + 1] == 1 else k - 1
                    if 0 <= nb_ < A and ava[b, i, nb_] == 1 and lo + 0.05 < rand["u"][b, i] < cdf[b, i, k] - 0.05:
                        found = (b, i, nb_)
        assert found is not None
        b, i, other = found
        a2, lp2 = a.clone(), lp.clone()
        a2[b, i, 0] = other
        # the replay is forced onto the changed prefix, as it would be for a kernel that took this action
        with eager_in_fp64():
            lg2 = replay_logits(m, rep, obs, a2, det)
            lp2, _ = act.heads_logprob_entropy(m, lg2, a2, ava)
        _, fails = check_decode(kind, A, L, lg2, _noisy(lg2, 2.0 ** -9, 5), a2, lp2, ava, rand, None, det)
        assert len(fails) == 1 and fails[0].startswith("argmax: 1 " if det else "sampling: 1 "), fails
        a3 = a.clone()
        b3 = 0
        a3[b3, (b3 + 1) % L, 0] = 1.0          # the row that allows only action 0
        _, fails = check_decode(kind, A, L, lg, yard, a3, lp, ava, rand, None, det)
        assert any(f.startswith("masking: 1 ") for f in fails), fails
    # Normal rows: Continuous, per-dimension std
    kind, A, L = "Continuous", 3, 5
    m, obs, rep, ava, rand = _cpu_case(kind, A, L, B)
    std = m.action_std()
    assert len(set(std.tolist())) == A
    for det in (False, True):
        with eager_in_fp64():
            a, lp = act.autoregressive_act(m, rep, obs, None, det, 1, rand)
            lg = replay_logits(m, rep, obs, a, det)
        yard = _noisy(lg, 2.0 ** -9, 6)
        st, fails = check_decode(kind, A, L, lg, yard, a, lp, None, rand, std, det)
        assert not fails and st["mean"][0] < 1e-12 and st["normal_lp_identity"] < 1e-12, (st, fails)
        bad = a.clone()
        bad[2, 3, 1] += 20 * st["mean"][2] * (1 + lg[2, 3, 1].abs())
        with eager_in_fp64():
            lg2 = replay_logits(m, rep, obs, bad, det)
        lpb = act.normal_logprob(bad, bad if det else bad - std * rand["n"], std)
        _, fails = check_decode(kind, A, L, lg2, _noisy(lg2, 2.0 ** -9, 6), bad, lpb, None, rand, std, det)
        assert len(fails) == 1 and fails[0].startswith("Normal mean") and " 1 entries" in fails[0], fails
        lpw = lp.clone()
        lpw[1, 2, 0] = act.normal_logprob(a[1, 2, 0], lg[1, 2, 0], std[1])   # dimension 0 with dimension 1's std
        _, fails = check_decode(kind, A, L, lg, yard, a, lpw, None, rand, std, det)
        assert len(fails) == 1 and fails[0].startswith("Normal log-prob identity") and " 1 entries" in fails[0], fails


def test_top_draws_choose_the_last_available_action():
    """u of u01_open's maximum is 1.0 in fp32 and above every fp32 CDF: the explained-decision check accepts exactly the
    last available action there, and the inputs carry such draws on rows whose last action is unavailable."""
    assert U_TOP == 1.0 and 0 < 1.0 - U_NEAR < 1e-7
    kind, A, L, B = "Discrete", 5, 9, 6
    m, obs, rep, ava, rand = _cpu_case(kind, A, L, B)
    rows = [(b, (b + 3) % L) for b in range(B)]
    assert all(rand["u"][b, i] == 1.0 and ava[b, i, A - 1] == 0 and ava[b, i, :A - 1].sum() == A - 1 for b, i in rows)
    assert all(ava[b, (b + 1) % L].tolist() == [1] + [0] * (A - 1) for b in range(B))
    assert all(ava[b, (b + 2) % L].tolist() == [0] * (A - 1) + [1] for b in range(B))
    lp64 = torch.log_softmax(torch.randn(1, A, dtype=torch.float64).masked_fill(ava[0, 3:4] == 0, act.MASK_LOGIT), -1)
    u = torch.ones(1, dtype=torch.float64)
    assert not decision_failures(lp64, torch.tensor([A - 2]), u, 2.5e-3, False)
    assert decision_failures(lp64, torch.tensor([A - 3]), u, 2.5e-3, False)


def test_weight_sets():
    """Both sets keep the orthogonal initialisation of the matrices and move every bias, LayerNorm parameter and
    log_std off its constant; the sharp set's logits span roughly +-10."""
    kind, A, L, B = "Discrete", 36, 9, 8
    for sharp in (False, True):
        m = make_model(kind, A, L, 2, sharp=sharp)
        for n, p in m.named_parameters():
            if p.dim() == 1:
                assert p.numel() == 1 or p.std().item() > 0.02, n
        w = m.decoder.blocks[0].mlp[2].weight
        assert (w @ w.T - 1e-4 * torch.eye(64)).abs().max().item() < 1e-6
        w = m.decoder.blocks[0].attn1.key.weight
        assert (w @ w.T - (0.25 if sharp else 1e-4) * torch.eye(64)).abs().max().item() < 1e-5
        obs, rep, ava, rand = make_inputs(m, B, L, A, "cpu")
        a, _ = act.autoregressive_act(m, rep, obs, ava, False, 1, rand)
        lg = replay_logits(m, rep, obs, a)
        span = (lg.max() - lg.min()).item()
        assert (12 < span < 40) if sharp else span < 1.0, span
    m = make_model("Semi_Discrete", 2, 5, 1)
    assert len(set(m.action_std().tolist())) == 2


def test_4wave_plan_query_agrees_with_the_geometry():
    """mdl_decode_4wave_plan answers for exactly the L that mdl_mat_decode_geometry accepts: 269 / 134 / 88."""
    lib = native_lib()
    for nb, top in ((1, 269), (2, 134), (3, 88)):
        fits = [L for L in range(1, L_SCAN + 1) if lib.mdl_mat_decode_geometry(nb, L, 1) > 0]
        assert fits == list(range(1, top + 1)), (nb, fits[-1])
        assert [L for L in range(1, L_SCAN + 1) if plan_4wave(lib, nb, L, 2, "Semi_Discrete") is not None] == fits
    assert plan_4wave(lib, 2, 6, 2, "Semi_Discrete") == (1, 1) and plan_4wave(lib, 2, 134, 36) == (0, 0)


# smallest (n_block, L, A) per instantiation: what enumerate_dispatch finds (profiles/decode_edges/README.md)
DISPATCH_TABLE = {'4wave': {'4wave<NB=1, STAGE=0> q2pre=0': (1, 213, 1),
           '4wave<NB=1, STAGE=0> q2pre=1': (1, 30, 64),
           '4wave<NB=1, STAGE=1> q2pre=0': (1, 26, 64),
           '4wave<NB=1, STAGE=1> q2pre=1': (1, 1, 1),
           '4wave<NB=2, STAGE=0> q2pre=0': (2, 105, 1),
           '4wave<NB=2, STAGE=0> q2pre=1': (2, 21, 64),
           '4wave<NB=2, STAGE=1> q2pre=0': (2, 17, 63),
           '4wave<NB=2, STAGE=1> q2pre=1': (2, 1, 1),
           '4wave<NB=3, STAGE=0> q2pre=0': (3, 68, 6),
           '4wave<NB=3, STAGE=0> q2pre=1': (3, 16, 64),
           '4wave<NB=3, STAGE=1> q2pre=0': (3, 11, 64),
           '4wave<NB=3, STAGE=1> q2pre=1': (3, 1, 1)},
 'default': {'4wave<NB=1, STAGE=0> q2pre=0': (1, 213, 1),
             '4wave<NB=1, STAGE=0> q2pre=1': (1, 164, 64),
             '4wave<NB=2, STAGE=0> q2pre=0': (2, 105, 5),
             '4wave<NB=2, STAGE=0> q2pre=1': (2, 34, 64),
             '4wave<NB=2, STAGE=1> q2pre=0': (2, 61, 28),
             '4wave<NB=3, STAGE=0> q2pre=0': (3, 68, 6),
             '4wave<NB=3, STAGE=0> q2pre=1': (3, 16, 64),
             '4wave<NB=3, STAGE=1> q2pre=0': (3, 11, 64),
             '4wave<NB=3, STAGE=1> q2pre=1': (3, 1, 1),
             'spec<NB=2, MA=1, 16-candidate, NREG=0, plain>': (2, 1, 3),
             'spec<NB=2, MA=1, 16-candidate, NREG=6, IND+Q2F>': (2, 109, 4),
             'spec<NB=2, MA=1, 16-candidate, NREG=6, IND>': (2, 100, 4),
             'spec<NB=2, MA=1, 16-candidate, NREG=8, plain>': (2, 49, 4),
             'spec<NB=2, MA=1, pair, NREG=0, plain>': (2, 1, 1),
             'spec<NB=2, MA=1, pair, NREG=6, IND+Q2F>': (2, 111, 2),
             'spec<NB=2, MA=1, pair, NREG=6, IND>': (2, 102, 2),
             'spec<NB=2, MA=1, pair, NREG=8, plain>': (2, 51, 2),
             'spec<NB=2, NS=1, MA=3, NREG=6, plain>': (2, 1, 5),
             'spec<NB=2, NS=2, MA=3, NREG=6, plain>': (2, 1, 17),
             'spec<NB=2, NS=3, MA=3, NREG=6, plain>': (2, 1, 33),
             'wave<NB=1, NREG=0, MA=1>': (1, 1, 1),
             'wave<NB=1, NREG=0, MA=3>': (1, 1, 5),
             'wave<NB=1, NREG=0, MA=4>': (1, 1, 49),
             'wave<NB=1, NREG=2, MA=1>': (1, 147, 4),
             'wave<NB=1, NREG=2, MA=3>': (1, 123, 47),
             'wave<NB=1, NREG=2, MA=4>': (1, 113, 64),
             'wave<NB=1, NREG=4, MA=1>': (1, 172, 4),
             'wave<NB=1, NREG=4, MA=3>': (1, 148, 48),
             'wave<NB=1, NREG=4, MA=4>': (1, 139, 63),
             'wave<NB=2, NREG=2, MA=4>': (2, 1, 49),
             'wave<NB=2, NREG=4, MA=4>': (2, 9, 62),
             'wave<NB=2, NREG=6, MA=4>': (2, 22, 61)},
 'wave': {'4wave<NB=1, STAGE=0> q2pre=0': (1, 213, 1),
          '4wave<NB=1, STAGE=0> q2pre=1': (1, 164, 64),
          '4wave<NB=2, STAGE=0> q2pre=0': (2, 105, 1),
          '4wave<NB=2, STAGE=0> q2pre=1': (2, 34, 64),
          '4wave<NB=2, STAGE=1> q2pre=0': (2, 40, 44),
          '4wave<NB=2, STAGE=1> q2pre=1': (2, 43, 34),
          '4wave<NB=3, STAGE=0> q2pre=0': (3, 68, 6),
          '4wave<NB=3, STAGE=0> q2pre=1': (3, 16, 64),
          '4wave<NB=3, STAGE=1> q2pre=0': (3, 11, 64),
          '4wave<NB=3, STAGE=1> q2pre=1': (3, 1, 1),
          'wave<NB=1, NREG=0, MA=1>': (1, 1, 1),
          'wave<NB=1, NREG=0, MA=3>': (1, 1, 5),
          'wave<NB=1, NREG=0, MA=4>': (1, 1, 49),
          'wave<NB=1, NREG=2, MA=1>': (1, 147, 4),
          'wave<NB=1, NREG=2, MA=3>': (1, 123, 47),
          'wave<NB=1, NREG=2, MA=4>': (1, 113, 64),
          'wave<NB=1, NREG=4, MA=1>': (1, 172, 4),
          'wave<NB=1, NREG=4, MA=3>': (1, 148, 48),
          'wave<NB=1, NREG=4, MA=4>': (1, 139, 63),
          'wave<NB=2, NREG=0, MA=1>': (2, 1, 1),
          'wave<NB=2, NREG=0, MA=3>': (2, 1, 5),
          'wave<NB=2, NREG=2, MA=1>': (2, 13, 3),
          'wave<NB=2, NREG=2, MA=3>': (2, 1, 46),
          'wave<NB=2, NREG=2, MA=4>': (2, 1, 49),
          'wave<NB=2, NREG=4, MA=1>': (2, 26, 3),
          'wave<NB=2, NREG=4, MA=3>': (2, 14, 45),
          'wave<NB=2, NREG=4, MA=4>': (2, 9, 62),
          'wave<NB=2, NREG=6, MA=1>': (2, 38, 4),
          'wave<NB=2, NREG=6, MA=3>': (2, 26, 48),
          'wave<NB=2, NREG=6, MA=4>': (2, 22, 61)}}


def test_dispatch_enumeration_table():
    """The committed table of instantiation -> smallest (n_block, L, A), for the default switches, for the one-wave
    kernel (speculative path off) and for the 4-wave kernel (one-wave path off)."""
    lib = native_lib()
    got = {"default": enumerate_dispatch(lib), "wave": enumerate_dispatch(lib, spec=False),
           "4wave": enumerate_dispatch(lib, wave=False)}
    assert got == DISPATCH_TABLE


def test_launch_cases_reach_their_instantiations_at_the_smallest_L():
    """Every launch case's path string is what the library's plan functions report, and its L is the smallest that
    selects the instantiation (L = 5 standing in for L = 1), apart from the stated largest-L cases."""
    lib = native_lib()
    cases = launch_cases()
    assert len(cases) == 31 + 42 + 18 + 4
    seen = {}
    for cid, c in cases.items():
        wave, spec = MODES[c["mode"]]
        lib.mdl_decode_spec_layout(c["layout"])
        try:
            path = plan_path(lib, c["nb"], c["L"], c["A"], c["kind"], wave=wave, spec=spec)
            inst = instantiation(lib, c["nb"], c["L"], c["A"], c["kind"], wave=wave, spec=spec)
            below = c["L"] > 1 and instantiation(lib, c["nb"], c["L"] - 1, c["A"], c["kind"], wave=wave, spec=spec)
        finally:
            lib.mdl_decode_spec_layout(0)
        assert path == c["path"], (cid, path)
        assert c.get("inst", inst) == inst, (cid, inst)
        key = (c["mode"], c["layout"], c["A"], inst)
        if key not in seen and c["L"] > 12:
            assert below != inst, (cid, "not the smallest L")
        seen.setdefault(key, c["L"])
    # the largest L of the 4-wave cases: the geometry rejects the next
    for nb, top in ((1, 269), (2, 134), (3, 88)):
        assert max(c["L"] for c in cases.values() if c["mode"] == "4wave" and c["nb"] == nb) == top
        assert lib.mdl_mat_decode_geometry(nb, top, 1) > 0 and lib.mdl_mat_decode_geometry(nb, top + 1, 1) <= 0
    # the largest L of the one-wave cases: the next L is the 4-wave kernel's, per (n_block, A)
    for (nb, A), ls in WV_L.items():
        top = ls[-1][0]
        assert plan_path(lib, nb, top, A, _kind(A), spec=False).startswith("wave"), (nb, A)
        assert plan_path(lib, nb, top + 1, A, _kind(A), spec=False) == "4wave", (nb, A, top)
