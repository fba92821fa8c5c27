"""The RL-side kernels (csrc/ppo.hip, csrc/rl_ops.hip, csrc/gather_rows.h) at their branch edges.

Every reference here is plain torch in float64 on the CPU, computed from the same fp32 inputs the kernel gets; no
reference calls a project kernel.  Inputs are drawn on the CPU (seeded) and copied to the device.  Each test prints the
largest error it saw (``pytest -s``) before it asserts.
"""
import ctypes
import itertools
import types

import pytest
import torch

from mat_dcml_amd.algos.valuenorm import ValueNorm
from mat_dcml_amd.ops import kernels, rl_ops
from mat_dcml_amd.utils.philox import feistel_randperm

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _report(name, **figs):
    print(f"[edges] {name}: " + ", ".join(f"{k} {float(v):.3e}" for k, v in figs.items()))


def _maxerr(a, b):
    return float((a - b).abs().max()) if a.numel() else 0.0


# ====================================================================================================== PPO loss
L_SEQ = 33
VN_BETA, VN_EPS = 0.99999, 1e-5
FLAG_NAMES = ("_use_huber_loss", "_use_clipped_value_loss", "_use_value_active_masks", "_use_policy_active_masks")
ALL_FLAGS = [dict(zip(FLAG_NAMES, bits)) for bits in itertools.product((True, False), repeat=4)]
OBJ_LP = [(1, 1), (2, 1), (1, 3), (2, 3)]


def _trainer(vn, **flags):
    d = dict(clip_param=0.2, value_loss_coef=0.5, entropy_coef=0.01, huber_delta=0.5, value_normalizer=vn)
    d.update({k: True for k in FLAG_NAMES})
    d.update(flags)
    return types.SimpleNamespace(**d)


def _ppo_inputs(seed, N, n_obj, n_lp):
    """The distribution of test_gpu_ppo.test_ppo_loss_grads_match_autograd, fp32 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    v, lp, ent = r(N, n_obj), r(N, n_lp) * 0.3 - 0.7, r(N, n_lp).abs()
    return {"v": v, "lp": lp, "ent": ent, "old_logp": lp + 0.3 * r(N, n_lp), "adv": r(N, n_obj),
            "value_preds": v + 0.3 * r(N, n_obj), "returns": 3 * r(N, n_obj) + 1,
            "active": (torch.rand(N, 1, generator=g) > 0.2).float()}


def _huber64(e, d):
    """The symmetric Huber of both project paths (algos/mat_trainer.py huber_loss, csrc/ppo.hip huber): the one
    place to change when the parity question of the reference's Huber is decided."""
    return torch.where(e.abs() <= d, 0.5 * e * e, d * (e.abs() - 0.5 * d))


def _vn_zero(n_obj):
    return {"m": torch.zeros(n_obj, dtype=F64), "sq": torch.zeros(n_obj, dtype=F64), "deb": torch.zeros((), dtype=F64)}


def _vn_update64(vn, ret):
    """algos/valuenorm.py update (per_element_update False): every minibatch weighs 1 - beta."""
    w = VN_BETA
    return {"m": vn["m"] * w + ret.mean(0) * (1.0 - w), "sq": vn["sq"] * w + (ret * ret).mean(0) * (1.0 - w),
            "deb": vn["deb"] * w + (1.0 - w)}


def _vn_mean_var64(m, sq, deb, eps=VN_EPS):
    """algos/valuenorm.py running_mean_var."""
    d = deb.clamp(min=eps)
    mean = m / d
    return mean, (sq / d - mean ** 2).clamp(min=1e-2)


def _ppo_ref(tr, inp, adv, vn):
    """Loss scalars, d/dv, d/dlogp, d/dent (autograd) and the ValueNorm update in float64.

    inp: the fp32 CPU inputs; adv: (N, n_obj) float64 standardised advantages; vn: float64 moments or None.
    The surrogate is summed over the log-prob entries and over the objectives (for (n_obj, n_lp) = (1, 1), (2, 1) and
    (1, 3) that is mat_trainer.ppo_update's ``min(...).sum(-1)``); the value loss is the mean over the objectives too.
    Also returns the share of entries in each branch and the tokens within reach of a discontinuous branch."""
    d = {k: t.double() for k, t in inp.items()}
    v, lp, ent = (d[k].clone().requires_grad_() for k in ("v", "lp", "ent"))
    act, ret, vpred = d["active"], d["returns"], d["value_preds"]
    n_obj = v.shape[1]
    clip, delta = tr.clip_param, tr.huber_delta
    imp = torch.exp(lp - d["old_logp"])
    ic = imp.clamp(1.0 - clip, 1.0 + clip)
    s1, s2 = imp[:, :, None] * adv[:, None, :], ic[:, :, None] * adv[:, None, :]   # (N, n_lp, n_obj)
    surr = torch.min(s1, s2).sum((1, 2)).unsqueeze(-1)
    den = act.sum().clamp(min=1.0)
    if tr._use_policy_active_masks:
        pl, e = -(surr * act).sum() / den, (ent * act).sum() / den
    else:
        pl, e = -surr.mean(), ent.mean()
    if vn is not None:
        vn = _vn_update64(vn, ret)
        mean, var = _vn_mean_var64(vn["m"], vn["sq"], vn["deb"])
        tgt = (ret - mean) / var.sqrt()
    else:
        tgt = ret
    dvc = v - vpred
    eo, ec = tgt - v, tgt - (vpred + dvc.clamp(-clip, clip))
    h = (lambda x: _huber64(x, delta)) if tr._use_huber_loss else (lambda x: 0.5 * x * x)
    lo, lc = h(eo), h(ec)
    vl_e = torch.max(lo, lc) if tr._use_clipped_value_loss else lo
    if tr._use_value_active_masks:   # (vl * am).sum() / am.sum() with am = active expanded over the objectives
        vl = (vl_e * act).sum() / (den * n_obj)
    else:
        vl = vl_e.mean()
    (pl - e * tr.entropy_coef + vl * tr.value_loss_coef).backward()
    with torch.no_grad():
        clipped = dvc.abs() > clip
        outside = (imp < 1.0 - clip) | (imp > 1.0 + clip)
        frac = lambda m: float(m.double().mean())  # noqa: E731
        shares = {"e > delta": frac(eo > delta), "e < -delta": frac(eo < -delta), "clipped value chosen": frac(lc > lo),
                  "original chosen while clipped": frac(clipped & (lo >= lc)),
                  "zero-gradient surrogate": frac(outside[:, :, None] & (s1 > s2))}
        near = ((imp - (1.0 - clip)).abs() < 1e-4) | ((imp - (1.0 + clip)).abs() < 1e-4)
        near = (near | (outside[:, :, None] & ((s1 - s2).abs() < 1e-5)).any(-1)).any(-1)
        if tr._use_clipped_value_loss:
            near = near | (((dvc.abs() - clip).abs() < 1e-4) | (clipped & ((lo - lc).abs() < 1e-4))).any(-1)
    return {"scalars": torch.stack([pl, vl, e, imp.mean()]).detach(), "dv": v.grad, "dlp": lp.grad, "dent": ent.grad,
            "vn": vn, "shares": shares, "near": near}


def _check_shares(tr, ref, what):
    """On the reference alone: the inputs populate every branch the flags enable."""
    need = ["zero-gradient surrogate"]
    if tr._use_huber_loss:
        need += ["e > delta", "e < -delta"]
    if tr._use_clipped_value_loss:
        need += ["clipped value chosen", "original chosen while clipped"]
    for k in need:
        assert ref["shares"][k] >= 0.10, (what, k, ref["shares"])


def _check_ppo(fused, grads, ref, what):
    """Tolerances of test_ppo_loss_grads_match_autograd.  Tokens near a discontinuous branch are left out of the
    per-element comparison only (at most 2 % of them); they stay in the four scalars."""
    N = ref["dv"].shape[0]
    dv, dlp, dent = (t.detach().cpu().double().reshape(N, -1) for t in grads)
    out = fused.out.cpu().double()
    keep = ~ref["near"]
    excl = 1.0 - float(keep.double().mean())
    errs = {"dv": _maxerr(dv[keep], ref["dv"][keep]), "dlogp": _maxerr(dlp[keep], ref["dlp"][keep]),
            "dent": _maxerr(dent, ref["dent"]), "scalars": _maxerr(out, ref["scalars"]), "excluded": excl}
    _report(what, **errs)
    assert excl <= 0.02, (what, excl)
    for t in (dv, dlp, dent, out):
        assert bool(torch.isfinite(t).all()), what
    assert torch.allclose(dlp[keep], ref["dlp"][keep], atol=1e-7, rtol=1e-4), (what, errs)
    assert torch.allclose(dent, ref["dent"], atol=1e-9, rtol=1e-4), (what, errs)
    assert torch.allclose(dv[keep], ref["dv"][keep], atol=1e-7, rtol=1e-4), (what, errs)
    assert torch.allclose(out, ref["scalars"], rtol=1e-4, atol=1e-5), (what, out, ref["scalars"])
    return errs


def _check_vn(vnm, ref_vn, what):
    got = [t.detach().cpu().double().reshape(-1) for t in (vnm.running_mean, vnm.running_mean_sq, vnm.debiasing_term)]
    want = [ref_vn["m"], ref_vn["sq"], ref_vn["deb"].reshape(-1)]
    assert torch.allclose(got[0], want[0], rtol=1e-5, atol=1e-10), (what, got[0], want[0])
    assert torch.allclose(got[1], want[1], rtol=1e-5, atol=1e-10), (what, got[1], want[1])
    assert torch.allclose(got[2], want[2], rtol=1e-6, atol=0.0), (what, got[2], want[2])


_DP_PAIR = types.SimpleNamespace(world_size=2, all_reduce_sum_=lambda t: t)   # mdl_ppo_reduce + mdl_ppo_finish


def _dense_case(gpu, entry, N, n_obj, n_lp, flags_list, use_vn=True, zero_active=False, shares=True, seed=0):
    """mdl_ppo_loss (``dense``) or the mdl_ppo_reduce / mdl_ppo_finish pair (``pair``), twice on one object."""
    from mat_dcml_amd.ops.ppo_fused import PPOLossFused
    inp = _ppo_inputs(seed, N, n_obj, n_lp)
    if zero_active:
        inp["active"].zero_()
    dev = {k: t.to(gpu) for k, t in inp.items()}
    mb = {k: dev[k] for k in ("old_logp", "adv", "value_preds", "returns", "active")}
    for flags in flags_list:
        tr = _trainer(ValueNorm(n_obj, device=gpu) if use_vn else None, **flags)
        fused = PPOLossFused(tr, gpu)
        vn = _vn_zero(n_obj) if use_vn else None
        for call in range(2):   # the second call starts from the moments the first one wrote
            what = f"{entry} N={N} n_obj={n_obj} n_lp={n_lp} vn={use_vn} call={call} " + \
                   "".join("01"[flags.get(k, True)] for k in FLAG_NAMES)
            ref = _ppo_ref(tr, inp, inp["adv"].double(), vn)
            vn = ref["vn"]
            if shares:
                _check_shares(tr, ref, what)
            fused.out.zero_()
            grads = fused.run(dev["v"], dev["lp"], dev["ent"], mb, comm=_DP_PAIR if entry == "pair" else None)
            torch.cuda.synchronize()
            _check_ppo(fused, grads, ref, what)
            if use_vn:
                _check_vn(tr.value_normalizer, vn, what)
            if zero_active:
                for t in grads:
                    assert bool((t == 0).all()), what
                assert bool((fused.out[:3] == 0).all()), (what, fused.out)


@pytest.mark.parametrize("n_obj,n_lp", OBJ_LP)
@pytest.mark.parametrize("N", [231, 3168])
@pytest.mark.parametrize("entry", ["dense", "pair"])
def test_ppo_loss_matches_fp64_autograd_in_every_branch(gpu, entry, N, n_obj, n_lp):
    """7 and 96 sequences of 33 tokens (one workgroup; 13 with a partial last one), huber_delta 0.5 so that both
    linear Huber branches, both sides of the value clip and the zero-gradient surrogate tokens are populated, under
    all 16 settings of the Huber / clipped-value / value-mask / policy-mask flags."""
    _dense_case(gpu, entry, N, n_obj, n_lp, ALL_FLAGS)


def _production_case(gpu, B, L, n_obj, n_lp, flags_list, zero_active=False, use_vn=True, shares=True, seed=10):
    """The trainer's call: rows of 4x larger source buffers read through a slice of the epoch permutation (``idx``),
    raw advantages standardised in-kernel from ``adv_sums``, and (with a value normaliser) the minibatch statistics
    precomputed by mb_stats (``pre_stats``: mdl_ppo_finish_fused, one launch, arrival counter).  Two different
    minibatches of the permutation in a row on one object."""
    from mat_dcml_amd.ops.ppo_fused import PPOLossFused
    S, N, n_mb = 4 * B, B * L, 4
    perm = torch.randperm(S, generator=torch.Generator().manual_seed(seed))
    sets = [_ppo_inputs(seed + 1 + c, N, n_obj, n_lp) for c in range(2)]
    src = {k: t.view(S, L, -1).clone() for k, t in _ppo_inputs(seed + 3, S * L, n_obj, n_lp).items()
           if k in ("old_logp", "adv", "value_preds", "returns", "active")}
    mbs = (1, 2)
    for c, m in enumerate(mbs):
        if zero_active:
            sets[c]["active"].zero_()
        for k in src:
            src[k][perm[m * B:(m + 1) * B]] = sets[c][k].view(B, L, -1)
    src["adv"] = src["adv"] * 3 + 1   # raw advantages
    # (x - mean) / (std + 1e-5) over the active entries of the whole buffer (mat_trainer.py advantage normalisation)
    x = src["adv"].double()
    sel = x[(src["active"] != 0).expand_as(x)]
    cnt = max(sel.numel(), 1)
    mean = sel.sum() / cnt
    adv64 = (x - mean) / (((sel * sel).sum() / cnt - mean * mean).clamp(min=0).sqrt() + 1e-5)
    dsrc = {k: t.to(gpu) for k, t in src.items()}
    dperm = perm.to(gpu)
    stats = kernels.mb_stats(dsrc["returns"], dsrc["active"], dperm, n_mb).float() if use_vn else None
    adv_sums = kernels.masked_sums(dsrc["adv"], dsrc["active"])
    dsets = [{k: s[k].view(B, L, -1).to(gpu) for k in ("v", "lp", "ent")} for s in sets]
    for flags in flags_list:
        tr = _trainer(ValueNorm(n_obj, device=gpu) if use_vn else None, **flags)
        fused = PPOLossFused(tr, gpu)
        vn = _vn_zero(n_obj) if use_vn else None
        for c, m in enumerate(mbs):
            what = f"production B={B} L={L} n_obj={n_obj} n_lp={n_lp} vn={use_vn} call={c} " + \
                   "".join("01"[flags.get(k, True)] for k in FLAG_NAMES)
            idx = perm[m * B:(m + 1) * B]
            ref = _ppo_ref(tr, sets[c], adv64[idx].reshape(N, n_obj), vn)
            vn = ref["vn"]
            if shares:
                _check_shares(tr, ref, what)
            mb = dict(dsrc, idx=dperm[m * B:(m + 1) * B], adv_sums=adv_sums)
            fused.out.zero_()
            grads = fused.run(dsets[c]["v"], dsets[c]["lp"], dsets[c]["ent"], mb,
                              pre_stats=stats[m] if use_vn else None)
            torch.cuda.synchronize()
            _check_ppo(fused, grads, ref, what)
            assert int(fused._ctr) == 0, what   # the last workgroup re-zeroed the arrival counter
            if use_vn:
                _check_vn(tr.value_normalizer, vn, what)
            if zero_active:
                for t in grads:
                    assert bool((t == 0).all()), what
                assert bool((fused.out[:3] == 0).all()), (what, fused.out)


@pytest.mark.parametrize("n_obj,n_lp", OBJ_LP)
@pytest.mark.parametrize("B", [7, 96])
def test_ppo_loss_production_entry_matches_fp64_autograd(gpu, B, n_obj, n_lp):
    _production_case(gpu, B, L_SEQ, n_obj, n_lp, ALL_FLAGS)


_MASKED = [{}, {"_use_huber_loss": False}, {"_use_clipped_value_loss": False}]   # both mask flags on


@pytest.mark.parametrize("n_obj,n_lp", [(2, 1), (1, 3)])
def test_ppo_loss_all_inactive_gives_exact_zeros(gpu, n_obj, n_lp):
    """Every active mask 0 under both mask flags: max(Σ active, 1) divides, so the losses and every gradient are
    exactly 0 and nothing is NaN; the ValueNorm update still happens (it does not look at the mask)."""
    for entry in ("dense", "pair"):
        _dense_case(gpu, entry, 231, n_obj, n_lp, _MASKED, zero_active=True, shares=False)
    _production_case(gpu, 7, L_SEQ, n_obj, n_lp, _MASKED, zero_active=True, shares=False)


@pytest.mark.parametrize("n_obj,n_lp", [(2, 1), (1, 3)])
def test_ppo_loss_without_value_normalizer(gpu, n_obj, n_lp):
    """value_normalizer None: raw returns are the target and no moments are written (dense, and the indexed
    mdl_ppo_loss the trainer uses when there are no precomputed statistics)."""
    _dense_case(gpu, "dense", 231, n_obj, n_lp, ALL_FLAGS, use_vn=False, shares=False)
    _production_case(gpu, 7, L_SEQ, n_obj, n_lp, ALL_FLAGS, use_vn=False, shares=False)


@pytest.mark.parametrize("n_obj,n_lp", [(1, 1), (2, 1), (1, 3)])
def test_ppo_loss_single_token(gpu, n_obj, n_lp):
    """N = 1: one thread of one workgroup does everything; the first ValueNorm update leaves variance 0, clamped."""
    flags = [{}, {k: False for k in FLAG_NAMES}]
    for entry in ("dense", "pair"):
        _dense_case(gpu, entry, 1, n_obj, n_lp, flags, shares=False)
    _dense_case(gpu, "dense", 1, n_obj, n_lp, flags, use_vn=False, shares=False)
    _production_case(gpu, 1, 1, n_obj, n_lp, flags, shares=False)


# ====================================================================================================== FlatAdam
def _adam_case(gpu, n, wd, max_norm, bad=None, bad_steps=(), norm_ready=False):
    """5 attempted steps vs torch.optim.Adam + clip_grad_norm_ in float64, which never sees a step in ``bad_steps``
    (one non-finite gradient entry: the kernel must leave parameters and moments untouched and count the step)."""
    from mat_dcml_amd.ops import mat_train
    from mat_dcml_amd.ops.ppo_fused import FlatAdam
    g = torch.Generator().manual_seed(n + len(bad_steps))
    p0 = torch.randn(n, generator=g)
    p_ref = torch.nn.Parameter(p0.double())
    opt = torch.optim.Adam([p_ref], lr=5e-4, eps=1e-5, weight_decay=wd)
    flat_p, flat_g = p0.to(gpu), torch.zeros(n, device=gpu)
    fa = FlatAdam(flat_p, flat_g, lr=5e-4, eps=1e-5, weight_decay=wd, max_grad_norm=max_norm)
    copies = 32
    if norm_ready:
        model = types.SimpleNamespace()
        ws = mat_train.attach_grad_workspace(model, flat_g, copies=copies)
        stride = ws.numel() // copies
    errs = {"p": 0.0, "m": 0.0, "v": 0.0, "norm_rel": 0.0}
    for it in range(5):
        grad = torch.randn(n, generator=g) * (0.01 if it % 2 else 1.0)
        is_bad = it in bad_steps
        if is_bad:
            grad[n - 1] = bad
        else:
            p_ref.grad = grad.double()
            norm = torch.nn.utils.clip_grad_norm_([p_ref], max_norm) if max_norm is not None else p_ref.grad.norm()
            opt.step()
        before = [t.clone() for t in (flat_p, fa.m, fa.v)]
        skipped = float(fa.skipped_steps)
        if norm_ready:   # the single-GPU path: Σ g² partials left by the workspace reduction, no norm launch
            k = it % copies
            ws[k * stride:k * stride + n].copy_(grad.to(gpu))
            flat_g.zero_()
            assert mat_train.reduce_grad_workspace(model, norm_into=fa.scratch) is True
        else:
            flat_g.copy_(grad.to(gpu))
        fa.step(norm_ready=norm_ready)
        torch.cuda.synchronize()
        what = (n, wd, max_norm, bad, norm_ready, it)
        if is_bad:
            for t, b in zip((flat_p, fa.m, fa.v), before):
                assert torch.equal(t, b), what
            assert float(fa.skipped_steps) == skipped + 1, what
            continue
        assert float(fa.skipped_steps) == skipped, what
        st = opt.state[p_ref]
        got = [t.cpu().double() for t in (flat_p, fa.m, fa.v)]
        errs["p"] = max(errs["p"], _maxerr(got[0], p_ref.detach()))
        errs["m"] = max(errs["m"], _maxerr(got[1], st["exp_avg"]))
        errs["v"] = max(errs["v"], _maxerr(got[2], st["exp_avg_sq"]))
        errs["norm_rel"] = max(errs["norm_rel"], abs(float(fa.grad_norm) - float(norm)) / float(norm))
        assert torch.allclose(fa.grad_norm.cpu().double(), norm, rtol=1e-4), (what, fa.grad_norm, norm)
        assert torch.allclose(got[0], p_ref.detach(), atol=1e-6, rtol=1e-5), (what, errs)
        # five fp32 accumulations: relative error ~1e-6, far inside these
        assert torch.allclose(got[1], st["exp_avg"], atol=1e-7, rtol=1e-4), (what, errs)
        assert torch.allclose(got[2], st["exp_avg_sq"], atol=1e-7, rtol=1e-4), (what, errs)
    assert fa.applied_steps() == 5 - len(bad_steps)
    _report(f"adam n={n} wd={wd} max_norm={max_norm} bad={bad}@{bad_steps} norm_ready={norm_ready}", **errs)


@pytest.mark.parametrize("wd,max_norm", [(1e-2, 1.0), (0.0, None), (1e-2, None)])
@pytest.mark.parametrize("n", [16, 1000, 151469])
def test_flat_adam_weight_decay_no_clip_small_n_match_fp64_adam(gpu, n, wd, max_norm):
    """n = 16 and 1000 leave most of the 128 norm workgroups empty; max_norm 1.0 clips the large-gradient steps and
    not the small ones (n = 16, 1000), so both sides of the min(1, ·) are taken."""
    _adam_case(gpu, n, wd, max_norm)


@pytest.mark.parametrize("norm_ready", [False, True])
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("n", [16, 1000, 151469])
def test_flat_adam_skips_non_finite_steps_and_keeps_applied_step_count(gpu, n, bad, norm_ready):
    """Attempted steps 0 and 3 carry one inf / nan (the last element: the norm pass's scalar tail at n = 151469):
    nothing moves, skipped_steps counts, and the finite steps after them match an Adam that never saw them — the
    bias corrections use the APPLIED step count, including after a skipped first step."""
    _adam_case(gpu, n, 1e-2, 1.0, bad=bad, bad_steps=(0, 3), norm_ready=norm_ready)


# ====================================================================================================== gather
GATHER_SRC_ROWS = 64
_WIDE = {}


def _wide_src(w):
    """(64, w) fp32 on the CPU, drawn once per width and never modified."""
    if w not in _WIDE:
        _WIDE[w] = torch.randn(GATHER_SRC_ROWS, w, generator=torch.Generator().manual_seed(w))
    return _WIDE[w]


def _gather_idx(rows, seed=0):
    """Row indices with repeats, in non-monotone order, touching the first and the last source row."""
    idx = torch.randint(0, GATHER_SRC_ROWS, (rows,), generator=torch.Generator().manual_seed(rows + seed))
    if rows >= 3:
        idx[0], idx[1], idx[-1] = GATHER_SRC_ROWS - 1, 0, GATHER_SRC_ROWS - 1
        assert idx.unique().numel() < rows and bool((idx[1:] < idx[:-1]).any())
    return idx


@pytest.mark.parametrize("rows", [1, 7, 300])
@pytest.mark.parametrize("w", [1024, 1027, 4096, 4100, 5001, 34776])
def test_gather_wide_rows_equal_index_select(gpu, w, rows):
    """Rows of >= 1024 floats go as (row, 4096-float chunk) items: exactly one chunk (1024, 4096), a partial last
    chunk of one float4 (4100) or of 2008 floats (34776 = 27 x 1288, 9 chunks), and widths not divisible by 4
    (1027, 5001: the scalar lanes)."""
    src, idx = _wide_src(w), _gather_idx(rows)
    out = kernels.gather_rows({"x": src.to(gpu)}, idx.to(gpu))["x"]
    assert out.shape == (rows, w)
    assert torch.equal(out.cpu(), src[idx])


def test_gather_wide_misaligned_source_takes_scalar_path(gpu):
    w = 4096
    src = torch.empty(GATHER_SRC_ROWS * w + 1, device=gpu)[1:].view(GATHER_SRC_ROWS, w)
    src.copy_(_wide_src(w))
    assert src.is_contiguous() and src.data_ptr() % 16 == 4
    for rows in (1, 7, 300):
        idx = _gather_idx(rows)
        assert torch.equal(kernels.gather_rows({"x": src}, idx.to(gpu))["x"].cpu(), _wide_src(w)[idx])


def test_gather_narrow_and_wide_entries_in_one_call_with_wide_norm(gpu):
    """blockIdx.y picks the entry: a narrow (33 x 7) one, plain wide ones and standardised wide ones (float4 lanes at
    4100, scalar lanes at 5001) in the same launch."""
    g = torch.Generator().manual_seed(5)
    narrow = torch.randn(GATHER_SRC_ROWS, 33, 7, generator=g)
    srcs = {"narrow": narrow, "wide": _wide_src(4096), "adv4": _wide_src(4100) * 3 + 1, "adv1": _wide_src(5001) * 3 + 1}
    active = (torch.rand(GATHER_SRC_ROWS, 4100, generator=g) < 0.8).float()
    sums = rl_ops.masked_sums(srcs["adv4"], active)   # plain torch, float64
    idx = _gather_idx(7)
    out = kernels.gather_rows({k: t.to(gpu) for k, t in srcs.items()}, idx.to(gpu), sums.to(gpu), ("adv4", "adv1"))
    assert torch.equal(out["narrow"].cpu(), narrow[idx]) and torch.equal(out["wide"].cpu(), srcs["wide"][idx])
    for k in ("adv4", "adv1"):
        torch.testing.assert_close(out[k].cpu(), rl_ops.normalize_from_sums(srcs[k], sums)[idx], rtol=1e-6, atol=1e-6)


def test_gather_writes_nothing_outside_its_destination_rows(gpu):
    """Hand-built GatherArgs whose destinations are slices of one sentinel-filled buffer: a chunk tail written past a
    row's end, or past the last row, would overwrite the sentinel between and after the slices."""
    sentinel, gap, rows = -777.0, 64, 7
    widths = [231, 1024, 4100, 5001, 34776]
    idx = _gather_idx(rows, seed=1)
    offs, total = [], gap
    for w in widths:
        offs.append(total)               # multiples of 4 floats where the width allows the float4 lanes
        total += (rows * w + 3) // 4 * 4 + gap
    buf = torch.full((total,), sentinel, device=gpu)
    assert buf.data_ptr() % 16 == 0
    srcs = [(_wide_src(w) if w >= 1024 else torch.randn(GATHER_SRC_ROWS, w, generator=torch.Generator().manual_seed(w)))
            for w in widths]
    dsrcs = [s.to(gpu) for s in srcs]
    didx = idx.to(gpu)
    a = kernels.GatherArgs()
    for k, (w, off) in enumerate(zip(widths, offs)):
        assert off % 4 == 0 and off + rows * w + gap <= total
        a.e[k] = kernels.GatherEnt(dsrcs[k].data_ptr(), buf.data_ptr() + 4 * off, w, 0)
    a.idx, a.sums, a.rows, a.n, a.eps = didx.data_ptr(), 0, rows, len(widths), 1e-5
    kernels.check(kernels.lib().mdl_gather_rows(ctypes.byref(a), kernels._stream()), "gather_rows")
    torch.cuda.synchronize()
    got = buf.cpu()
    outside = torch.ones(total, dtype=torch.bool)
    for w, off, s in zip(widths, offs, srcs):
        assert torch.equal(got[off:off + rows * w].view(rows, w), s[idx]), w
        outside[off:off + rows * w] = False
    assert int(outside.sum()) >= gap * (len(widths) + 1)
    assert bool((got[outside] == sentinel).all())


# ====================================================================================================== GAE
def _gae_ref64(rew, vp, masks, mean, sd, gamma, lam):
    """shared_buffer.py compute_returns' recurrence on denormalised values, float64."""
    T = rew.shape[0]
    v = vp * sd + mean
    g = torch.zeros_like(rew[0])
    adv, ret = torch.empty_like(rew), torch.empty_like(rew)
    for t in reversed(range(T)):
        delta = rew[t] + gamma * v[t + 1] * masks[t + 1] - v[t]
        g = delta + gamma * lam * masks[t + 1] * g
        adv[t], ret[t] = g, g + v[t]
    return adv, ret


@pytest.mark.parametrize("T", [1, 7, 8, 9, 16, 17, 50])
@pytest.mark.parametrize("K,nvn", [(1, 1), (2, 2), (2, 1), (1, 0)])
def test_gae_scans_match_fp64_recurrence(gpu, K, nvn, T):
    """Both scans at every position of the 8-step prefetch loop's block / tail split (T < 8, = 8, 8 + 1, 2 x 8,
    2 x 8 + 1, 50) and at lane counts that are no multiple of the 256-thread block: E·A·K = 5, 257 and 33·8·2 for one
    objective, 10, 514 and 33·8·2 for two.  Mask variants: one time slice all zero; one sequence all ones."""
    gamma, lam = 0.99, 0.95
    worst = {"adv": 0.0, "ret": 0.0}
    for E, A in ((5, 1), (257, 1), (16 // K, 33)):
        g = torch.Generator().manual_seed(100 * T + 10 * K + nvn + E)
        rew = torch.randn(T, E, A, K, generator=g) * 10
        vp = torch.randn(T + 1, E, A, K, generator=g)
        nv = torch.randn(E, A, K, generator=g)
        vn = None
        mean, sd = torch.zeros(1, dtype=F64), torch.ones(1, dtype=F64)
        if nvn:
            vn = ValueNorm(nvn, device=gpu)
            vn.update((torch.randn(1000, nvn, generator=g) * 20 + 3).to(gpu))
            mean, var = _vn_mean_var64(*(t.cpu().double() for t in (vn.running_mean, vn.running_mean_sq,
                                                                      vn.debiasing_term)), eps=vn.epsilon)
            sd = var.sqrt()
        for variant in ("zero slice", "ones sequence"):
            masks = (torch.rand(T + 1, E, A, 1, generator=g) > 0.2).float()
            if variant == "zero slice":
                masks[max(1, T // 2)] = 0.0
            else:
                masks[:, 0, 0] = 1.0
            vp_full = vp.clone()
            vp_full[-1] = nv
            adv_ref, ret_ref = _gae_ref64(rew.double(), vp_full.double(), masks.double(), mean, sd, gamma, lam)
            d_rew, d_masks, d_nv = rew.to(gpu), masks.to(gpu), nv.to(gpu)
            outs = {}
            # gae_reverse_scan: statistics handed in as [means | stds], V(T) already in the last slot
            ms = torch.cat([mean.expand(K), sd.expand(K)]).float().to(gpu)
            adv, ret = torch.zeros(T, E, A, K, device=gpu), torch.zeros(T + 1, E, A, K, device=gpu)
            kernels.gae_reverse_scan(d_rew, vp_full.to(gpu), d_masks, ms, gamma, lam, adv, ret)
            outs["scan"] = (adv, ret)
            # gae_reverse_scan_vn: statistics from the running moments, V(T) from next_value
            d_vp = vp.to(gpu)
            adv, ret = torch.zeros(T, E, A, K, device=gpu), torch.zeros(T + 1, E, A, K, device=gpu)
            kernels.gae_reverse_scan_vn(d_rew, d_vp, d_masks, d_nv.reshape(-1).contiguous(), vn, gamma, lam, adv, ret)
            outs["scan_vn"] = (adv, ret)
            torch.cuda.synchronize()
            assert torch.equal(d_vp[-1], d_nv) and torch.equal(d_vp[:-1].cpu(), vp[:-1])
            for name, (adv, ret) in outs.items():
                a, r = adv.cpu().double(), ret[:T].cpu().double()
                worst["adv"], worst["ret"] = max(worst["adv"], _maxerr(a, adv_ref)), max(worst["ret"], _maxerr(r, ret_ref))
                assert torch.allclose(a, adv_ref, atol=1e-3, rtol=1e-4), (name, variant, E, A, _maxerr(a, adv_ref))
                assert torch.allclose(r, ret_ref, atol=1e-3, rtol=1e-4), (name, variant, E, A, _maxerr(r, ret_ref))
    _report(f"gae T={T} K={K} nvn={nvn}", **worst)


# ====================================================================================================== statistics
@pytest.mark.parametrize("mdiv", [1, 2])
@pytest.mark.parametrize("n", [3, 255, 61441])
def test_masked_sums_small_and_boundary_sizes(gpu, n, mdiv):
    """n mask entries (x has mdiv per mask entry): 3 and 255 leave all but one of the 240 blocks empty, 61441 is one
    element past 240 x 256 (the grid-stride loop's second trip)."""
    g = torch.Generator().manual_seed(n + mdiv)
    x = torch.randn(n, mdiv, generator=g) * 3 + 1
    mask = (torch.rand(n, 1, generator=g) < 0.8).float()
    mask[0], mask[-1] = 1.0, 1.0
    sel = x.double()[(mask != 0).expand_as(x)]
    ref = torch.stack([sel.sum(), (sel * sel).sum(), torch.tensor(float(sel.numel()), dtype=F64)])
    dx, dm = x.to(gpu), mask.to(gpu)
    sums = kernels.masked_sums(dx, dm)
    _report(f"masked_sums n={n} mdiv={mdiv}", err=_maxerr(sums.cpu(), ref))
    torch.testing.assert_close(sums.cpu(), ref, rtol=1e-12, atol=1e-9)
    assert torch.equal(sums, kernels.masked_sums(dx, dm))


@pytest.mark.parametrize("n", [3, 61441])
def test_masked_sums_all_masked_then_gather_clamps_count_to_one(gpu, n):
    """No active entry: (0, 0, 0); the standardisation then divides by max(count, 1) = 1, so mean 0, std 0 and the
    gathered advantage is x / eps, as normalize_from_sums."""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, 2, generator=g) * 3 + 1
    dx = x.to(gpu)
    sums = kernels.masked_sums(dx, torch.zeros(n, 1, device=gpu))
    assert torch.equal(sums.cpu(), torch.zeros(3, dtype=F64))
    idx = torch.randint(0, n, (5,), generator=g)
    out = kernels.gather_rows({"adv": dx}, idx.to(gpu), sums, ("adv",))["adv"].cpu()
    ref = rl_ops.normalize_from_sums(x, torch.zeros(3, dtype=F64))[idx]
    assert bool(torch.isfinite(out).all())
    torch.testing.assert_close(out, ref, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("n_mb,mb,width", [(1, 301, 1), (4, 77, 1), (1, 100, 33), (4, 100, 33)])
def test_mb_stats_width_one_and_ragged_minibatches(gpu, n_mb, mb, width, K):
    """Token width 1 and minibatches whose token counts (301, 77, 3300) are no multiple of the 256-thread block, over a
    permutation slice of a larger buffer."""
    g = torch.Generator().manual_seed(n_mb * 1000 + mb + width + K)
    N = n_mb * mb + 13
    ret = torch.randn(N, width, K, generator=g) * 7
    act = (torch.rand(N, width, 1, generator=g) > 0.1).float()
    perm = torch.randperm(N, generator=g)[:n_mb * mb].contiguous()
    out = kernels.mb_stats(ret.to(gpu), act.to(gpu), perm.to(gpu), n_mb).cpu()
    assert out.shape == (n_mb, 2 * K + 2)
    for m, idx in enumerate(perm.view(n_mb, mb)):
        r = ret[idx].double().reshape(-1, K)
        ref = torch.cat([r.sum(0), (r * r).sum(0), torch.tensor([float(r.shape[0])], dtype=F64),
                         act[idx].double().sum().reshape(1)])
        assert torch.allclose(out[m], ref, rtol=1e-10, atol=1e-8), (m, out[m], ref)


@pytest.mark.parametrize("n", [3, 4, 5, 16, 17, 255, 256, 257, 65536, 65537])
def test_randperm_matches_feistel_reference_at_boundary_sizes(gpu, n):
    """Around the powers of 4 where the Feistel half-width changes and around the 256-thread block."""
    for key in ((12345, 678), (2 ** 31 - 2, n)):
        p = kernels.randperm(n, gpu, key=key).cpu()
        assert torch.equal(torch.sort(p).values, torch.arange(n)), (n, key)
        assert torch.equal(p, feistel_randperm(n, *key)), (n, key)
