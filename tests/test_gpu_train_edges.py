"""Discrete / Semi_Discrete fused training kernels (csrc/mat_enc_ct.hip, csrc/mat_dec_ct.hip) against fp64 autograd of
the eager model at the edges tests/test_gpu_train.py leaves out: n_block 1 and 3, workgroups that walk several chunks,
two objectives, one 16-row tile plus a row, all-first tokens.  Per case: per-token forward outputs, every parameter
gradient, per-row checks of the token-indexed gradients, chunk attribution, bitwise repeats with the gradient
workspace poisoned.  Measurements: profiles/train_edges/README.md."""
import copy
import functools

import pytest
import torch

from mat_dcml_amd.models.mat import MultiAgentTransformer
from mat_dcml_amd.ops import mat_train, ppo_fused
from test_gpu_avail_cont_train import _float_keeps_fp64, _loss_grads
from test_train_edges_helper import (YARD_FACTOR, chunk_map, describe_sequences, launch_grid, rel, row_stats,
                                     token_check, token_errors)

pytestmark = pytest.mark.gpu

# key: (action type, A, L, B, n_block, n_objective, obs_dim): the edge each case pins.  B = ("cu", a, b): a n_CU + b
CASES = {
    "nb1_dcml": ("Semi_Discrete", 2, 33, 40, 1, 1, 7),       # <1, ...> instantiations; small-gradient LDS slots at 11
    "nb3_dcml": ("Semi_Discrete", 2, 33, 40, 3, 1, 7),       # <3, ...>; block-2 LN slots; small_wg_slot0 == -1, A <= 2
    "nb3_long": ("Semi_Discrete", 2, 129, 3, 3, 1, 7),       # SQ = 1, largest LDS tile, three blocks of saves
    "nb1_mpe": ("Discrete", 5, 3, 40, 1, 1, 18),             # train_mpe.py: wide observations, one block, tiny L
    "nobj2": ("Semi_Discrete", 2, 33, 40, 2, 2, 7),          # both value columns and their head gradients
    "chunks_bench": ("Semi_Discrete", 2, 33, ("cu", 13, 0), 2, 1, 7),   # backward chunks (5, 5, 3) / (3, 5, 5)
    "chunks_ragged": ("Semi_Discrete", 2, 33, ("cu", 5, 7), 3, 1, 7),   # a few workgroups walk a second chunk, NB = 3
    "tile_plus_1": ("Discrete", 5, 17, 1, 1, 1, 7),          # one 16-row tile plus one row; KP (32) below NRP (64)
    "first_only": ("Discrete", 5, 1, 40, 3, 1, 7),           # every token is a first token
}
CHUNK_CASES = ("chunks_bench", "chunks_ragged")
MODEL_SEED, INPUT_SEED = 2, 3   # tests/test_gpu_train.py::test_full_mat_fused_grads
EMB_W, HEAD_W, LOG_STD = "decoder.action_encoder.0.weight", "decoder.head.3.weight", "decoder.log_std"


def n_cu(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _shape(dev, key):
    kind, A, L, B, nb, nobj, od = CASES[key]
    if isinstance(B, tuple):
        B = B[1] * n_cu(dev) + B[2]
    return kind, A, L, B, nb, nobj, od


def make_model(kind, A, L, od, n_block, nobj, dev, seed=MODEL_SEED, scale=0.2):
    """tests/test_gpu_train.py's ``make`` (Semi_Discrete) / ``make_discrete`` with n_block and n_objective: weights at
    scale 0.2, LayerNorm parameters perturbed."""
    torch.manual_seed(seed)
    if kind == "Semi_Discrete":
        m = MultiAgentTransformer(L + 1, od, A, L, n_block, 64, 2, action_type=kind, semi_index=-1, n_objective=nobj)
    else:
        m = MultiAgentTransformer(L, od, A, L, n_block, 64, 2, action_type=kind, n_objective=nobj)
    m = m.to(dev)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "ln" in n or "head.2" in n or "obs_encoder.0" in n:
                p.copy_((1.0 + 0.1 * torch.randn(p.shape, generator=g)).to(dev) if n.endswith("weight")
                        else (0.1 * torch.randn(p.shape, generator=g)).to(dev))
            else:
                s = scale if kind == "Semi_Discrete" or p.shape[-1] < 100 else scale / 4.0
                p.copy_((torch.randn(p.shape, generator=g) * s).to(dev))
    return m


def make_inputs(kind, A, L, B, nobj, od, dev, seed=INPUT_SEED):
    """test_full_mat_fused_grads's inputs: action 1 (Discrete: every odd action) unavailable on every fourth agent,
    the stored action an available one; Semi_Discrete: the last agent's action a fraction in [0, 1)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    obs = torch.rand(B, L, od, device=dev, generator=g)
    ava = torch.ones(B, L, A, device=dev)
    ava[:, 1::4, 1::2] = 0
    if kind == "Semi_Discrete":
        actions = (torch.rand(B, L, 1, device=dev, generator=g) < 0.5).float()
    else:
        actions = torch.randint(0, A, (B, L, 1), device=dev, generator=g).float()
    actions[ava.gather(-1, actions.long()) == 0] = 0
    if kind == "Semi_Discrete":
        actions[:, -1, 0] = torch.rand(B, device=dev, generator=g)
    w1 = torch.randn(B, L, 1, device=dev, generator=g)
    w2 = torch.randn(B, L, nobj, device=dev, generator=g)
    w3 = torch.randn(B, L, 1, device=dev, generator=g)
    return obs, actions, ava, w1, w2, w3


class Case:
    """One case (tests/test_gpu_avail_cont_train.py's Case): inputs, the fp64 reference and the bf16-autocast yardstick
    of the eager model, and the fused kernels behind ``mat_train.evaluate_actions`` writing a private gradient
    workspace."""

    def __init__(self, dev, kind, A, L, B, nb, nobj, od):
        self.dims = (kind, A, L, B, nb, nobj, od)
        m = self.m = make_model(kind, A, L, od, nb, nobj, dev)
        self.inputs = make_inputs(kind, A, L, B, nobj, od, dev)
        m64 = copy.deepcopy(m).double()
        with _float_keeps_fp64():
            self.ref, (lp, v) = _loss_grads(m64, *(t.double() for t in self.inputs))
            with torch.no_grad():
                _, _, ent = m64(None, *(t.double() for t in self.inputs[:3]))
        assert all(r.dtype == torch.float64 for r in self.ref.values())
        assert lp.dtype == v.dtype == ent.dtype == torch.float64
        self.out_ref = {"logp": lp, "ent": ent, "v": v}
        del m64
        with torch.autocast("cuda", dtype=torch.bfloat16):
            self.yard, (lp, v) = _loss_grads(m, *self.inputs)
            with torch.no_grad():
                _, _, ent = m(None, *self.inputs[:3])
        self.out_yard = {"logp": lp, "ent": ent, "v": v}
        m.zero_grad()
        self.wide = od > mat_train.MAX_FUSED_OBS
        ppo_fused.flatten_params(m)
        self.fg = torch.zeros_like(m._mdl_flat_params)
        self.offsets = ppo_fused.param_offsets(m)
        for p, off in self.offsets:
            p.grad = self.fg[off:off + p.numel()].view_as(p)
        self.ws = mat_train.attach_grad_workspace(m, self.fg, mode="private")
        self.grads = self.out = None

    def poison(self):
        """NaN in every workspace slot of every copy that a backward launch is to write (Case.poison of
        tests/test_gpu_avail_cont_train.py)."""
        assert not self.wide
        _, _, stride, copies = self.m._mdl_gws_buf
        ws = self.ws.view(copies, stride)
        for (name, p), (_, off) in zip(self.m.named_parameters(), self.offsets):
            if name in self.ref:
                ws[:, off:off + p.numel()] = float("nan")

    def run(self):
        """evaluate_actions + backward of the weighted-sum loss + reduction -> (flat gradient, logp, ent, v)."""
        m = self.m
        obs, actions, ava, w1, w2, w3 = self.inputs
        self.fg.zero_()
        m._mdl_gws_active = True
        try:
            v, logp, ent = mat_train.evaluate_actions(m, obs, actions, ava)
            ((logp * w1).sum() + (v * w2).sum() + (ent * w3).sum()).backward()
        finally:
            m._mdl_gws_active = False
        # wide observations: the flat buffer already holds the embedding's gradients (the trainer's _direct_grads)
        mat_train.reduce_grad_workspace(m, accumulate=self.wide)
        torch.cuda.synchronize()
        return self.fg.clone(), logp.detach().clone(), ent.detach().clone(), v.detach().clone()

    def fused(self):
        if self.grads is None:
            flat, logp, ent, v = self.run()
            self.out = {"logp": logp, "ent": ent, "v": v}
            self.grads = {n: flat[off:off + p.numel()].view_as(p) for (n, p), (_, off)
                          in zip(self.m.named_parameters(), self.offsets)}
        return self.grads


@functools.lru_cache(maxsize=None)
def case(dev, key):
    return Case(dev, *_shape(dev, key))


def _geometry(dev, key):
    """(SQ, backward grid) with the case's edge asserted from the library."""
    kind, A, L, B, nb, nobj, od = _shape(dev, key)
    SQ = mat_train.geometry(L)[0]
    assert SQ > 0, (key, L)
    grid = int(mat_train.lib().mdl_ct_bwd_grid(B, SQ))
    if key in CHUNK_CASES:
        assert grid < -(-B // SQ), f"{key}: no workgroup walks a second chunk (grid {grid}, B {B}, SQ {SQ})"
        assert grid == launch_grid(B, SQ, n_cu(dev), True), (grid, B, SQ, n_cu(dev))
    if key == "chunks_bench":
        assert B // grid >= 11, f"{key}: {B // grid} sequences per workgroup fit two SQ = {SQ} chunks"
    if key == "chunks_ragged":
        walks = [x[2] for x in chunk_map(B, SQ, L, grid, True)]
        assert 1 in walks and 2 in walks, f"{key}: chunks per workgroup {sorted(set(walks))}"
    return SQ, grid


# ------------------------------------------------------------------------------------------------ 1, 3. outputs
@pytest.mark.parametrize("key", list(CASES))
def test_per_token_outputs_match_fp64(gpu, key):
    """logp, entropy and v of ``mat_train.evaluate_actions`` element by element against the fp64 eager model:
    max_t |k - ref| / (1 + |ref|) within 2.5 x the same statistic of the bf16-autocast eager model (floored at 2.5e-3
    where that yardstick is below 1e-3).  The chunk cases name the workgroup and chunk of every sequence over the
    bound.  Measured: profiles/train_edges/README.md."""
    c = case(gpu, key)
    kind, A, L, B, nb, nobj, od = _shape(gpu, key)
    assert mat_train.supported(c.m), mat_train.decoder_unsupported_reasons(c.m) + mat_train.encoder_unsupported_reasons(c.m)
    assert c.m.n_block == nb and c.m.n_objective == nobj
    SQ, grid = _geometry(gpu, key)
    c.fused()
    assert c.out["logp"].shape == (B, L, 1) and c.out["ent"].shape == (B, L, 1) and c.out["v"].shape == (B, L, nobj)
    bad = []
    for name in ("logp", "ent", "v"):
        s, y, b, ok = token_check(c.out[name], c.out_ref[name], c.out_yard[name])
        print(f"[train-edges] {key} {name}: kernel {s:.3e} yardstick {y:.3e} bound {b:.3e}"
              f"{' (floor)' if y < 1e-3 else ''}")
        if not ok:
            per_seq = token_errors(c.out[name], c.out_ref[name]).amax(dim=(1, 2))
            seqs = (~(per_seq <= b)).nonzero().flatten().tolist()
            bad.append(f"{name}: {s:.3e} > {b:.3e} (yardstick {y:.3e}) at " + describe_sequences(seqs[:8], B, SQ, L, n_cu(gpu)))
    if key in CHUNK_CASES:   # the same bound on every chunk of a workgroup's walk, forward and backward
        per_seq = token_errors(c.out["logp"], c.out_ref["logp"]).amax(dim=(1, 2))
        for backward in (False, True):
            cm = chunk_map(B, SQ, L, launch_grid(B, SQ, n_cu(gpu), backward), backward)
            steps = max(x[1] for x in cm) + 1
            worst = [max(float(per_seq[s]) for s in range(B) if cm[s][1] == it) for it in range(steps)]
            print(f"[train-edges] {key} logp by {'backward' if backward else 'forward'} chunk of the walk:",
                  " ".join(f"{w:.3e}" for w in worst))
    assert not bad, "; ".join(bad)


# ------------------------------------------------------------------------------------------------ 2. gradients
@pytest.mark.parametrize("key", list(CASES))
def test_every_gradient_and_token_rows_match_fp64(gpu, key):
    """Every parameter gradient through the private workspace against fp64 autograd: rel() within max(6e-2, 2.5 x
    rel(bf16-autocast, fp64)); key.bias by test_full_mat_fused_grads's absolute rule (8e-2 of the key weight's
    largest gradient); log_std by test_full_mat_fused_grads's rule for it, max(0.1, 10 x yardstick).  Gradients that
    are exactly zero in fp64 (only at L = 1) have their own test below.  Each row of the token-indexed gradients (the
    action embedding's column per token id, the action head's row per action) by its own norm ratio, denominator
    floored at 1e-3 of the tensor's norm, within max(6e-2, 2.5 x the same ratio of the bf16-autocast row); a row that
    is exactly zero in fp64 exactly zero."""
    c = case(gpu, key)
    _geometry(gpu, key)
    g = c.fused()
    assert all(bool(torch.isfinite(x).all()) for x in g.values())
    zeros = _fp64_zero_gradients(c)
    assert bool(zeros) == (key in ZERO_GRADIENT_CASES), zeros   # every such parameter is in the test below
    bad, margins = [], []
    for n, r in c.ref.items():
        yd = rel(c.yard[n], r)
        if n in zeros:
            continue
        if "key.bias" in n:
            e = (g[n] - r).abs().max().item() / (c.ref[n.replace("key.bias", "key.weight")].abs().max().item() + 1e-6)
            lim = 8e-2
        elif n == LOG_STD:
            e, lim = rel(g[n], r), max(0.1, 10 * yd)
        else:
            e, lim = rel(g[n], r), max(6e-2, YARD_FACTOR * yd)
        margins.append((e / lim, n))
        if not e <= lim:
            bad.append((n, float(f"{e:.4g}"), float(f"{lim:.4g}")))
    for n, x in g.items():   # parameters the forward does not use
        if n not in c.ref:
            assert torch.count_nonzero(x) == 0, n
    print(f"[train-edges] {key} worst gradient error / limit:",
          [(round(x, 3), n) for x, n in sorted(margins, reverse=True)[:3]])
    for n, dim in ((EMB_W, 1), (HEAD_W, 0)):
        rows, yrows = row_stats(g[n], c.ref[n], dim), row_stats(c.yard[n], c.ref[n], dim)
        other = tuple(d for d in range(2) if d != dim)
        zero = c.ref[n].abs().amax(dim=other) == 0
        for i in range(rows.numel()):
            lim = max(6e-2, YARD_FACTOR * float(yrows[i]))
            if bool(zero[i]):   # a token id no sequence feeds: not one product may reach its row
                e, lim = float(g[n].select(dim, i).abs().max()), 0.0
            else:
                e = float(rows[i])
            if not e <= lim:
                bad.append((f"{n} row {i}", float(f"{e:.4g}"), float(f"{lim:.4g}")))
        print(f"[train-edges] {key} {n} rows: worst {float(rows.max()):.3e} (yardstick rows {float(yrows.max()):.3e})")
    if key == "first_only":   # no token has a previous action: only column 0 of dW_a is non-zero
        assert float(c.ref[EMB_W][:, 1:].abs().max()) == 0 and float(g[EMB_W][:, 0].abs().max()) > 0
    assert not bad, bad


ZERO_GRADIENT_CASES = ("first_only",)


def _fp64_zero_gradients(c):
    return [n for n, r in c.ref.items() if float(r.abs().max()) == 0]


@pytest.mark.parametrize("key", ZERO_GRADIENT_CASES)
def test_gradients_that_are_zero_in_fp64_are_exactly_zero(gpu, key):
    """A parameter whose fp64 gradient is exactly zero must get exactly zero.  Over ONE key (L = 1) the softmax is the
    constant 1, so the query / key weights and biases of every attention (encoder, decoder self and cross attention,
    three blocks: 36 parameters) have exactly zero gradients in fp64 — and in bf16-autocast eager, whose softmax
    backward computes p (g - Σ p g) = g - g.

    This test found the kernels returning rounding-sized values there (largest |g| 1.5e-6 beside value-weight
    gradients of 3 to 13; per parameter: profiles/train_edges/README.md): the attention backward (csrc/mat_train_ct.h)
    forms dS = P (dP - delta) with dP = dO Vᵀ from an MFMA over bf16 operands and delta = rowsum(dO O) from the saved
    hi / lo output (attn_delta_ct) — the same products summed in two orders, which cancel to rounding, not to zero,
    and Adam turns a rounding-sized gradient into a full-size step.  attn_bwd_q_ct / attn_bwd_kv_ct now store dQ and
    dK as zeros at L = 1."""
    c = case(gpu, key)
    g = c.fused()
    zeros = _fp64_zero_gradients(c)
    assert len(zeros) == 4 * 3 * c.m.n_block, zeros
    assert all(n.rsplit(".", 2)[1] in ("query", "key") for n in zeros), zeros
    assert all(float(c.yard[n].abs().max()) == 0 for n in zeros)   # the yardstick is exactly zero as well
    worst = {n: float(g[n].abs().max()) for n in zeros}
    for n in zeros:
        scale = c.ref[n.rsplit(".", 2)[0] + ".value.weight"].abs().max().item()
        print(f"[train-edges] {key} {n}: largest |g| {worst[n]:.3e} (fp64 0; value-weight gradient up to {scale:.3e})")
    bad = {n: w for n, w in worst.items() if w != 0}
    assert not bad, f"{len(bad)} of {len(zeros)} gradients that are exactly zero in fp64 are not: largest |g| " \
                    f"{max(bad.values()):.3e} ({max(bad, key=bad.get)})"


# ------------------------------------------------------------------------------------------------ 4. bitwise repeat
@pytest.mark.parametrize("key", ["nb3_dcml", "chunks_ragged"])
def test_bitwise_repeat_with_poisoned_workspace(gpu, key):
    """Two runs give the same flat gradient bit for bit, the second with NaN in every workspace slot beforehand: at
    NB = 3 the small gradients (dW_a, dW_h2, db_h2) leave through the per-chunk flush, and every slot the reduction
    reads was written by that launch (first-chunk stores, then load-add-store)."""
    c = case(gpu, key)
    _geometry(gpu, key)
    a = c.run()[0]
    c.poison()
    b = c.run()[0]
    assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
    assert not bool(torch.isnan(b).any()), f"{int(torch.isnan(b).sum())} NaN survive the reduction"
    assert torch.equal(a, b), f"{int((a != b).sum())} elements differ"
