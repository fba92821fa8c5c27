"""Continuous action type (MA-MuJoCo): the decoder's action-embedding backward as an MFMA weight-gradient product
(csrc/mat_dec_ct.hip, the CONT branch of dec_bwd_tile) — fp64 parity of every parameter gradient, bitwise repeats with
the gradient workspace poisoned, bit-reproducible MuJoCo trainers with wide and narrow observations, the atomic
opt-out's report, and a cost guard.  Measurements behind the limits: profiles/cont_emb_det/README.md."""
import contextlib
import copy
import functools
import warnings

import pytest
import torch

from conftest import median_us, perf_record
from mat_dcml_amd.models.mat import MultiAgentTransformer
from mat_dcml_amd.ops import mat_train, ppo_fused

pytestmark = pytest.mark.gpu

# (L, B, A, obs_dim, action scale): the edge each shape pins
SHAPES = {
    "base": (6, 50, 3, 11, 1.0),        # the existing Continuous gradient test's shape
    "first_only": (1, 40, 2, 11, 1.0),  # every token is a sequence's first: dW_a exactly zero, db_a not (LDS slots, A <= 2)
    "tile_plus_1": (17, 1, 1, 11, 1.0),  # one sequence, one workgroup: a full 16-row tile plus one row, A = 1
    "A16": (5, 7, 16, 11, 1.0),         # exactly one full 16-column tile of X
    "A17": (5, 7, 17, 11, 1.0),         # a second column tile of one column (the 4-tile head instantiation)
    "A64": (4, 6, 64, 11, 1.0),         # MAX_ACTION_DIM: all four column tiles, waves 4-7 flush too
    "chunks": (33, 3200, 3, 11, 1.0),   # workgroups walk 5, 5, 3 sequences: first-chunk store, then load-add-store
    "wide_obs": (6, 50, 3, 18, 1.0),    # observations through csrc/obs_embed.hip (direct .grad writes next to the copies)
    "x37": (6, 50, 3, 11, 37.3),        # large actions (a missing X lo tile: see test_x_lo_tile_is_used)
}

# action_encoder.{weight,bias} against fp64: 4 x the largest error of the fp32 LDS-atomic path this one replaces, over
# these shapes (same inputs, parent build; profiles/cont_emb_det/README.md), floored at 1e-5 relative.  The factor 4
# covers a different but equally valid fp32 summation tree plus the dropped Ylo.Xlo term (<= 2^-16 relative).
PARENT_WORST_EMB_ERR = 4.2334e-2   # the bias at the base shape (the upstream bf16 error of d pre, not the product's)
EMB_LIMIT = max(1e-5, 4.0 * PARENT_WORST_EMB_ERR)
EMB = ("decoder.action_encoder.0.weight", "decoder.action_encoder.0.bias")


def rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-300)).item()


def make_cont(L, A, od, dev):
    """tests/test_gpu_train.py::test_full_mat_fused_grads_continuous's model: weights at scale 0.2, LN / log_std
    perturbed."""
    torch.manual_seed(3)
    m = MultiAgentTransformer(L, od, A, L, 2, 64, 2, action_type="Continuous").to(dev)
    g0 = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "ln" in n or "head.2" in n or "obs_encoder.0" in n:
                p.copy_((1.0 + 0.1 * torch.randn(p.shape, generator=g0)).to(dev) if n.endswith("weight")
                        else (0.1 * torch.randn(p.shape, generator=g0)).to(dev))
            elif n.endswith("log_std"):
                p.copy_((0.3 * torch.randn(p.shape, generator=g0)).to(dev))
            else:
                p.copy_((torch.randn(p.shape, generator=g0) * 0.2).to(dev))
    return m


@contextlib.contextmanager
def _float_keeps_fp64():
    """The eager model casts logits / attention scores with ``.float()``; an fp64 reference must not round there."""
    orig = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self if self.dtype == torch.float64 else orig(self, *a, **k)
    try:
        yield
    finally:
        torch.Tensor.float = orig


def _loss_grads(m, obs, actions, w1, w2, w3):
    m.zero_grad()
    lp, v, ent = m(None, obs, actions, None)
    ((lp.to(w1.dtype) * w1).sum() + (v.to(w2.dtype) * w2).sum() + (ent.to(w3.dtype) * w3).sum()).backward()
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


class Case:
    """One shape: inputs, the fp64 and bf16-autocast references of the eager model, and the fused kernels wired to a
    private gradient workspace (tests/test_gpu_train.py::test_private_workspace_grads_match_direct)."""

    def __init__(self, dev, L, B, A, od, scale):
        m = self.m = make_cont(L, A, od, dev)
        g = torch.Generator(device=dev).manual_seed(7)
        self.obs = torch.rand(B, L, od, device=dev, generator=g)
        self.actions = torch.randn(B, L, A, device=dev, generator=g) * 0.5 * scale
        self.w1, self.w3 = (torch.randn(B, L, A, device=dev, generator=g) for _ in range(2))
        self.w2 = torch.randn(B, L, 1, device=dev, generator=g)
        m64 = copy.deepcopy(m).double()
        with _float_keeps_fp64():
            self.ref = _loss_grads(m64, self.obs.double(), self.actions.double(), self.w1.double(), self.w2.double(),
                                   self.w3.double())
        assert all(r.dtype == torch.float64 for r in self.ref.values())
        del m64
        ref32 = _loss_grads(m, self.obs, self.actions, self.w1, self.w2, self.w3)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            refb = _loss_grads(m, self.obs, self.actions, self.w1, self.w2, self.w3)
        self.bf16_err = {n: rel(refb[n], ref32[n]) for n in ref32}   # the existing tests' yardstick
        m.zero_grad()
        self.wide = od > mat_train.MAX_FUSED_OBS
        ppo_fused.flatten_params(m)
        self.fg = torch.zeros_like(m._mdl_flat_params)
        self.offsets = ppo_fused.param_offsets(m)
        for p, off in self.offsets:
            p.grad = self.fg[off:off + p.numel()].view_as(p)
        self.enc, self.dec = mat_train.EncoderFused(m), mat_train.DecoderFused(m)
        self.ws = mat_train.attach_grad_workspace(m, self.fg, mode="private")
        self.grads = None

    def poison(self):
        """NaN in every workspace slot of every copy that a backward launch is to write: every parameter the model's
        forward uses (the unused state encoder has no gradient, in autograd or here), except the observation
        embedding's with wide observations (csrc/obs_embed.hip adds those straight into .grad)."""
        _, _, stride, copies = self.m._mdl_gws_buf
        ws = self.ws.view(copies, stride)
        for (name, p), (_, off) in zip(self.m.named_parameters(), self.offsets):
            if name in self.ref and not (self.wide and name.startswith("encoder.obs_encoder")):
                ws[:, off:off + p.numel()] = float("nan")

    def run(self):
        """Fused forward + backward + reduction -> the flat gradient."""
        m = self.m
        self.fg.zero_()
        m._mdl_gws_active = True
        try:
            v, rep = self.enc.forward(self.obs)
            self.dec.forward(rep, self.actions, None)
            drep = self.dec.backward(self.w1, self.w3)
            self.enc.backward(drep, self.w2)
        finally:
            m._mdl_gws_active = False
        # wide observations: the flat buffer already holds the embedding's gradients (the trainer's _direct_grads)
        mat_train.reduce_grad_workspace(m, accumulate=self.wide)
        torch.cuda.synchronize()
        return self.fg.clone()

    def fused(self):
        if self.grads is None:
            flat = self.run()
            self.grads = {n: flat[off:off + p.numel()].view_as(p) for (n, p), (_, off)
                          in zip(self.m.named_parameters(), self.offsets)}
        return self.grads

    def emb_errors(self):
        """Relative error of action_encoder.{weight,bias} against fp64 (None where the reference is exactly zero)."""
        g = self.fused()
        return {n: (rel(g[n], self.ref[n]) if float(self.ref[n].abs().max()) > 0 else None) for n in EMB}


@functools.lru_cache(maxsize=None)
def case(dev, key):
    return Case(dev, *SHAPES[key])


# ------------------------------------------------------------------------------------------------ a. fp64 parity
@pytest.mark.parametrize("key", list(SHAPES))
def test_every_gradient_matches_fp64_autograd(gpu, key):
    """Fused forward / backward through the private workspace against fp64 autograd of the eager model.
    action_encoder.{weight,bias} are held to EMB_LIMIT (4 x the replaced fp32-atomic path's worst error, floored at
    1e-5); every other parameter to the existing tests' max(6e-2, 2.5 x bf16-autocast error).  Shapes: see SHAPES.
    Measured (profiles/cont_emb_det/README.md): 1.2e-2 .. 4.2e-2 for both the replaced path and this one — the bf16
    error of d pre arriving from the blocks — so a build without the X lo tile still passes here (x37: 3.33e-2
    against 3.30e-2); test_x_lo_tile_is_used is the check that fails for it."""
    c = case(gpu, key)
    g = c.fused()
    errs = c.emb_errors()
    print(f"[cont-emb] {key}: " + ", ".join(f"{n.split('.')[-1]} {e:.3e}" if e is not None else f"{n.split('.')[-1]} ref=0"
                                          for n, e in errs.items()) + f" (limit {EMB_LIMIT:.3e})")
    assert all(bool(torch.isfinite(x).all()) for x in g.values())
    bad = []
    for n, r in c.ref.items():
        if n in EMB:
            if errs[n] is None:   # no token has a previous action: not one product may reach dW_a
                assert torch.count_nonzero(g[n]) == 0, n
                continue
            e, lim = errs[n], EMB_LIMIT
        elif "key.bias" in n or float(r.abs().max()) == 0:
            # an exactly zero gradient (softmax is shift-invariant: every key bias; over ONE key, L = 1, it is constant:
            # the query / key weights and biases too): the absolute error against the attention's key-weight gradient
            # as in the existing tests, or its value-weight gradient where that is zero as well
            att = n.rsplit(".", 2)[0]
            scale = max(c.ref[att + ".key.weight"].abs().max().item(), 0.0) or c.ref[att + ".value.weight"].abs().max().item()
            e, lim = (g[n] - r).abs().max().item() / (scale + 1e-6), 8e-2
        else:
            e, lim = rel(g[n], r), max(6e-2, 2.5 * c.bf16_err[n])
        if not e <= lim:
            bad.append((n, e, lim))
    assert not bad, bad
    if key == "first_only":
        assert float(c.ref[EMB[0]].abs().max()) == 0 and torch.count_nonzero(g[EMB[0]]) == 0
        assert float(g[EMB[1]].abs().max()) > 0


def x_lo_check(dev, A):
    """Every previous action is the constant (37.3, 1.0, ...): column 0 of dW_a is then 37.3 x column 1, both summed
    over the same d pre rows in the same MFMA order.  bf16(1.0) is exact; bf16(37.3) = 37.25 is off by 1.3e-3, which
    only the X lo tile brings back.  Returns the relative distance of dW_a[:, 0] / 37.3 from dW_a[:, 1]."""
    c = Case(dev, 6, 50, A, 11, 1.0)
    c.actions[...] = 1.0
    c.actions[..., 0] = 37.3
    w = c.fused()[EMB[0]]
    return rel(w[:, 0] / c.actions[0, 0, 0], w[:, 1])


# what separates the two columns with the lo tile in place: the dropped Ylo.Xlo term and the bf16 rounding of Xlo, each
# <= 2^-18 of a product, plus fp32 accumulation order — 2^-17 with a 16-fold allowance for cancellation in the signed
# sum over tokens.  Without the lo tile the distance is 1.3e-3.
X_LO_LIMIT = 2.0 ** -13


@pytest.mark.parametrize("A", [2, 3])
def test_x_lo_tile_is_used(gpu, A):
    """The fp64 comparison above cannot see a missing X lo tile (the upstream bf16 error of d pre is 20 x larger:
    profiles/cont_emb_det/README.md); this one isolates the product.  A = 2: the LDS-slot flush (wgrad_g_vacc);
    A = 3: the private-copy flush (wgrad_g)."""
    d = x_lo_check(gpu, A)
    print(f"[cont-emb] dW_a column ratio distance {d:.3e} (limit {X_LO_LIMIT:.3e})")
    assert d <= X_LO_LIMIT, d


# ------------------------------------------------------------------------------------------------ b. bitwise repeat
@pytest.mark.parametrize("key", ["chunks", "wide_obs"])
def test_bitwise_repeat_with_poisoned_workspace(gpu, key):
    """Two runs give the same flat gradient bit for bit, the second with NaN in every workspace slot beforehand: each
    slot the reduction reads was written by that launch (first-chunk stores, not read-modify-writes of stale values)."""
    c = case(gpu, key)
    a = c.run()
    c.poison()
    b = c.run()
    assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
    assert torch.equal(a, b), f"{int((a != b).sum())} elements differ (NaN: {int(torch.isnan(b).sum())})"


# ------------------------------------------------------------------------------------------------ c. trainers
def _mujoco_runner(gpu, conf, obsk):
    from mat_dcml_amd.config import _MUJOCO_FLAGS, get_config, parse_args
    from mat_dcml_amd.runner.mujoco_runner import MujocoRunner
    args = parse_args(["--env_name", "mujoco", "--scenario", "HalfCheetah-v2", "--agent_conf", conf, "--agent_obsk",
                       str(obsk), "--n_rollout_threads", "8", "--episode_length", "10", "--ppo_epoch", "2",
                       "--num_mini_batch", "2", "--seed", "2"], get_config(), extra=_MUJOCO_FLAGS, warn=False)
    assert args.cuda_deterministic is True   # store_false, not passed: on, as in the reference's scripts
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = MujocoRunner({"all_args": args, "device": gpu, "run_dir": None})
    return r, [str(x.message) for x in w if "cuda_deterministic" in str(x.message)]


def _snapshot(r):
    opt = r.policy.optimizer
    return {"params": torch.cat([p.detach().reshape(-1) for p in r.policy.transformer.parameters()]).clone(),
            "exp_avg": opt.m.clone(), "exp_avg_sq": opt.v.clone(), "scratch": opt.scratch[:4].clone()}


ROLLOUT = ("obs", "actions", "action_log_probs", "value_preds", "rewards", "masks")


def _train_twice(gpu, conf, obsk, wide):
    """Two PPO iterations of a fresh runner: [rollout 1, update 1, rollout 2, update 2] snapshots."""
    r, warned = _mujoco_runner(gpu, conf, obsk)
    tr, m = r.trainer, r.policy.transformer
    assert m.action_type == "Continuous"
    assert (m.encoder.obs_dim > mat_train.MAX_FUSED_OBS) == wide, m.encoder.obs_dim
    assert tr.fused, tr.fused_reason
    assert tr.deterministic is True, tr.nondeterministic_writer
    assert tr.nondeterministic_writer is None
    assert not warned, warned
    r.warmup()
    snaps = []
    for _ in range(2):
        r.rollout()
        snaps.append({k: getattr(r.buffer, k).clone() for k in ROLLOUT})
        r.compute()
        r.train()
        snaps.append(_snapshot(r))
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in snaps[-1].values())
    return snaps


@pytest.mark.parametrize("conf,obsk,wide", [("6x1", 2, True), ("2x3", 1, False)])
def test_mujoco_trainer_deterministic_and_bitwise_repeatable(gpu, conf, obsk, wide):
    """HalfCheetah 6x1 with agent_obsk 2 (obs 17 > 16: csrc/obs_embed.hip; A = 1: the LDS-slot flush) and 2x3 with
    agent_obsk 1 (obs 14; A = 3: the private-copy flush): the fused trainer claims determinism without a warning, and
    two same-seed runs agree bit for bit on parameters, both Adam moments and the optimizer scratch."""
    a, b = _train_twice(gpu, conf, obsk, wide), _train_twice(gpu, conf, obsk, wide)
    for i, (sa, sb) in enumerate(zip(a, b)):
        what = f"rollout {i // 2 + 1}" if i % 2 == 0 else f"update {i // 2 + 1}"
        for k in sa:
            assert torch.equal(sa[k], sb[k]), f"{what}: {k} differs by {(sa[k] - sb[k]).abs().max().item():.3e}"


# ------------------------------------------------------------------------------------------------ d. opt-out
def test_atomic_grad_mode_still_reports_its_writer(gpu, monkeypatch):
    monkeypatch.setenv("MAT_DCML_GRAD_MODE", "atomic")
    r, warned = _mujoco_runner(gpu, "2x3", 1)
    tr = r.trainer
    assert tr.fused and tr.deterministic is False
    assert "gradient workspace" in tr.nondeterministic_writer and "atomic" in tr.nondeterministic_writer
    assert len(warned) == 1 and "gradient workspace" in warned[0], warned


# ------------------------------------------------------------------------------------------------ e. cost guard
# 1.25 x the measured median (profiles/cont_emb_det/README.md; the replaced fp32-atomic backward measured there too)
DEC_BWD_MUJOCO_US = 151.6   # the replaced fp32-atomic backward: 184.5
DEC_BWD_MUJOCO_BOUND_US = round(1.25 * DEC_BWD_MUJOCO_US, 1)


def dec_bwd_mujoco_us(gpu):
    """DecoderFused.backward at a MuJoCo-like training shape (L = 6, A = 1, 4,000 sequences), private workspace."""
    c = Case(gpu, 6, 4000, 1, 11, 1.0)
    m = c.m
    m._mdl_gws_active = True
    try:
        _, rep = c.enc.forward(c.obs)
        c.dec.forward(rep, c.actions, None)
        for _ in range(20):   # clocks ramp after a suite of small launches
            c.dec.backward(c.w1, c.w3)
        return median_us(lambda: c.dec.backward(c.w1, c.w3), iters=20)
    finally:
        m._mdl_gws_active = False
        m._mdl_gws_grid = None


def test_decoder_backward_cost_guard(gpu):
    us = dec_bwd_mujoco_us(gpu)
    perf_record("dec_bwd_continuous_6x1_4000_us", us, DEC_BWD_MUJOCO_BOUND_US)
    assert us <= DEC_BWD_MUJOCO_BOUND_US, us
