"""Available_Continuous action type on the fused decoder training kernels (csrc/mat_dec_ct.hip, the AV instantiation
of mat_dec_fwd_ct / mat_dec_bwd_ct; MAT_DCML_AVAIL_CONT_TRAIN=fused): fp64 parity of the forward outputs and of every
parameter gradient, the X lo tile of the embedding weight gradient, the in-kernel minibatch index, bitwise repeats
with the gradient workspace poisoned, a bit-reproducible trainer, rollout-vs-learner log-probs, and a cost guard
against the hybrid path it replaces.  Measurements: profiles/avail_cont_fused/README.md."""
import contextlib
import copy
import functools
import warnings

import pytest
import torch

from conftest import median_us, perf_record
from mat_dcml_amd.models.mat import MultiAgentTransformer
from mat_dcml_amd.ops import mat_fused, mat_train, ppo_fused

pytestmark = pytest.mark.gpu

ENV = "MAT_DCML_AVAIL_CONT_TRAIN"

# (L, B, A, obs_dim, availability): the edge each shape pins.  B = None: 5 n_CU + 7 sequences (see _shape).
# availability: "mask" = one of the two choices masked on about a third of the tokens (the stored choice is the
# available one, never both masked), "ones" = everything available, None = no availability tensor
SHAPES = {
    "base": (6, 40, 4, 9, "mask"),          # the hybrid test's shape
    "first_only": (1, 40, 3, 9, None),      # every token is a first token: only column 0 of dW_a is non-zero
    "tile_plus_1": (17, 1, 3, 9, "ones"),   # one full 16-row tile plus one row; the smallest A (one Normal dimension)
    "A15": (5, 7, 15, 9, "ones"),           # A + 1 = 16: exactly one X column tile
    "A16": (5, 7, 16, 9, None),             # A + 1 = 17: a second X tile of one column; the largest A
    "chunks": (33, None, 4, 9, "mask"),     # some workgroups walk two chunks (store, then load-add-store), last partial
    "wide_obs": (6, 40, 4, 18, "mask"),     # observations through csrc/obs_embed.hip
}
EMB_W = "decoder.action_encoder.0.weight"
LOG_STD = "decoder.log_std"


def rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-300)).item()


def _shape(dev, key):
    L, B, A, od, av = SHAPES[key]
    if B is None:
        B = 5 * torch.cuda.get_device_properties(dev).multi_processor_count + 7
    return L, B, A, od, av


def make_av(L, A, od, dev):
    """tests/test_gpu_train.py::test_hybrid_available_continuous_grads's model: weights at scale 0.2, LN / log_std
    perturbed."""
    torch.manual_seed(4)
    m = MultiAgentTransformer(L + 1, od, A, L, 2, 64, 2, action_type="Available_Continuous").to(dev)
    g0 = torch.Generator().manual_seed(4)
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


def _loss_grads(m, obs, actions, ava, w1, w2, w3):
    """(gradients, (logp, v)) of the weighted-sum loss through the eager model."""
    m.zero_grad()
    lp, v, ent = m(None, obs, actions, ava)
    ((lp.to(w1.dtype) * w1).sum() + (v.to(w2.dtype) * w2).sum() + (ent.to(w3.dtype) * w3).sum()).backward()
    return ({n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None},
            (lp.detach().clone(), v.detach().clone()))


INPUT_SEED = 7   # the input stream of tests/test_gpu_continuous_det.py's Case, for every shape of this file


def make_inputs(dev, L, B, A, od, av, seed=INPUT_SEED):
    g = torch.Generator(device=dev).manual_seed(seed)
    obs = torch.rand(B, L, od, device=dev, generator=g)
    pick = torch.randint(0, 2, (B, L), device=dev, generator=g)
    actions = torch.cat([torch.nn.functional.one_hot(pick, 2).float(),
                         torch.randn(B, L, A - 2, device=dev, generator=g) * 0.5], -1)
    ava = None
    if av is not None:
        ava = torch.ones(B, L, A, device=dev)
    if av == "mask":
        hide = torch.rand(B, L, device=dev, generator=g) < 1.0 / 3.0
        ava[..., 0] = torch.where(hide & (pick == 1), 0.0, 1.0)   # the choice NOT taken; never both
        ava[..., 1] = torch.where(hide & (pick == 0), 0.0, 1.0)
        assert bool((ava[..., :2].sum(-1) >= 1).all()) and bool((ava[..., :2].gather(-1, pick[..., None]) == 1).all())
        frac = float((ava[..., :2].sum(-1) == 1).float().mean())
        assert 0.15 < frac < 0.5 or B * L < 100, frac
    w1, w3 = (torch.randn(B, L, A - 1, device=dev, generator=g) for _ in range(2))
    w2 = torch.randn(B, L, 1, device=dev, generator=g)
    return obs, actions, ava, w1, w2, w3


class Case:
    """One shape: inputs, the fp64 and bf16-autocast references of the eager model, and the fused kernels wired to a
    private gradient workspace (tests/test_gpu_continuous_det.py)."""

    def __init__(self, dev, L, B, A, od, av, actions=None, seed=INPUT_SEED):
        m = self.m = make_av(L, A, od, dev)
        self.obs, self.actions, self.ava, self.w1, self.w2, self.w3 = make_inputs(dev, L, B, A, od, av, seed)
        if actions is not None:
            self.actions = actions(self.actions)
        d = lambda t: None if t is None else t.double()  # noqa: E731
        m64 = copy.deepcopy(m).double()
        with _float_keeps_fp64():
            self.ref, self.out_ref = _loss_grads(m64, d(self.obs), d(self.actions), d(self.ava), d(self.w1), d(self.w2),
                                                 d(self.w3))
        assert all(r.dtype == torch.float64 for r in self.ref.values())
        del m64
        args = (self.obs, self.actions, self.ava, self.w1, self.w2, self.w3)
        ref32, out32 = _loss_grads(m, *args)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            refb, outb = _loss_grads(m, *args)
        self.bf16_err = {n: rel(refb[n], ref32[n]) for n in ref32}   # the existing tests' yardstick
        self.bf16_out_err = tuple(rel(b.float(), r) for b, r in zip(outb, out32))
        m.zero_grad()
        self.wide = od > mat_train.MAX_FUSED_OBS
        ppo_fused.flatten_params(m)
        self.fg = torch.zeros_like(m._mdl_flat_params)
        self.offsets = ppo_fused.param_offsets(m)
        for p, off in self.offsets:
            p.grad = self.fg[off:off + p.numel()].view_as(p)
        self.enc, self.dec = mat_train.EncoderFused(m), mat_train.DecoderFused(m)
        self.ws = mat_train.attach_grad_workspace(m, self.fg, mode="private")
        self.grads = self.out = None

    def poison(self):
        """NaN in every workspace slot of every copy that a backward launch is to write: every parameter the model's
        forward uses, except the observation embedding's with wide observations (csrc/obs_embed.hip adds those straight
        into .grad)."""
        _, _, stride, copies = self.m._mdl_gws_buf
        ws = self.ws.view(copies, stride)
        for (name, p), (_, off) in zip(self.m.named_parameters(), self.offsets):
            if name in self.ref and not (self.wide and name.startswith("encoder.obs_encoder")):
                ws[:, off:off + p.numel()] = float("nan")

    def run(self, obs=None, actions=None, ava=None, idx=None):
        """Fused forward + backward + reduction -> (flat gradient, logp, ent, v).  ``idx``: the inputs are buffer rows
        read through the index in-kernel."""
        m = self.m
        if obs is None:
            obs, actions, ava = self.obs, self.actions, self.ava
        self.fg.zero_()
        m._mdl_gws_active = True
        try:
            v, rep = self.enc.forward(obs, idx=idx)
            logp, ent = self.dec.forward(rep, actions, ava, idx=idx)
            drep = self.dec.backward(self.w1, self.w3)
            self.enc.backward(drep, self.w2)
        finally:
            m._mdl_gws_active = False
        # wide observations: the flat buffer already holds the embedding's gradients (the trainer's _direct_grads)
        mat_train.reduce_grad_workspace(m, accumulate=self.wide)
        torch.cuda.synchronize()
        return self.fg.clone(), logp.clone(), ent.clone(), v.clone()

    def fused(self):
        if self.grads is None:
            flat, logp, ent, v = self.run()
            self.out = (logp, ent, v)
            self.grads = {n: flat[off:off + p.numel()].view_as(p) for (n, p), (_, off)
                          in zip(self.m.named_parameters(), self.offsets)}
        return self.grads


@functools.lru_cache(maxsize=None)
def case(dev, key):
    return Case(dev, *_shape(dev, key))


@pytest.fixture(autouse=True)
def _fused_switch(monkeypatch):
    monkeypatch.setenv(ENV, "fused")


# ------------------------------------------------------------------------------------------------ a. fp64 parity
@pytest.mark.parametrize("key", list(SHAPES))
def test_outputs_and_every_gradient_match_fp64_autograd(gpu, key):
    """Fused forward / backward through the private workspace against fp64 autograd of the eager model: logp / v within
    max(3e-2, 2.5 x bf16-autocast error), every gradient within max(6e-2, 2.5 x bf16-autocast error), exactly zero
    gradients by the key.bias rule at 8e-2 (tests/test_gpu_continuous_det.py).  Shapes: see SHAPES.
    Measured worst error / limit per shape (profiles/avail_cont_fused/README.md): 0.25 .. 0.89, the largest always an
    attention query / key gradient (the attention backward every instantiation shares).  The one-sequence shape (17
    tokens, nothing averages the bf16 rounding) moves with the input draw: over input seeds 0-7 and 9 its worst error
    / limit was 0.45, 0.37, 0.90, 0.58, 0.26, 2.08, 0.78, 0.54 and 1.07 — two draws miss the limit — and the
    Continuous instantiation at (17, 1, A, od) for A in 1-5, od in {9, 11} gave 0.32 .. 0.81 with one draw at 1.28.
    This file uses INPUT_SEED for every shape."""
    c = case(gpu, key)
    L, B, A, od, av = _shape(gpu, key)
    assert mat_train.supported(c.m)
    g = c.fused()
    logp, ent, v = c.out
    assert logp.shape == (B, L, A - 1) and ent.shape == (B, L, A - 1) and v.shape == (B, L, 1)
    assert all(bool(torch.isfinite(x).all()) for x in (logp, ent, v))
    e_lp, e_v = rel(logp, c.out_ref[0]), rel(v, c.out_ref[1])
    lim_lp, lim_v = max(3e-2, 2.5 * c.bf16_out_err[0]), max(3e-2, 2.5 * c.bf16_out_err[1])
    print(f"[avail-cont] {key}: logp {e_lp:.3e} (limit {lim_lp:.3e}), v {e_v:.3e} (limit {lim_v:.3e})")
    assert e_lp <= lim_lp and e_v <= lim_v, (e_lp, lim_lp, e_v, lim_v)
    assert all(bool(torch.isfinite(x).all()) for x in g.values())
    bad, margins = [], []
    for n, r in c.ref.items():
        if "key.bias" in n or float(r.abs().max()) == 0:
            # an exactly zero gradient (softmax is shift-invariant: every key bias; over ONE key, L = 1, it is constant:
            # the query / key weights and biases too): the absolute error against the attention's key-weight gradient
            # as in the existing tests, or its value-weight gradient where that is zero as well
            att = n.rsplit(".", 2)[0]
            scale = max(c.ref[att + ".key.weight"].abs().max().item(), 0.0) or c.ref[att + ".value.weight"].abs().max().item()
            e, lim = (g[n] - r).abs().max().item() / (scale + 1e-6), 8e-2
        else:
            e, lim = rel(g[n], r), max(6e-2, 2.5 * c.bf16_err[n])
        margins.append((e / lim, n))
        if not e <= lim:
            bad.append((n, e, lim))
    print("[avail-cont] worst error / limit:", [(round(x, 3), n) for x, n in sorted(margins, reverse=True)[:4]])
    assert not bad, bad
    # d log_std: the two categorical slots receive exactly zero, the Normal dimensions match fp64
    assert torch.count_nonzero(g[LOG_STD][:2]) == 0, g[LOG_STD]
    assert float(c.ref[LOG_STD][:2].abs().max()) == 0
    e = rel(g[LOG_STD][2:], c.ref[LOG_STD][2:])
    assert e <= max(6e-2, 2.5 * c.bf16_err[LOG_STD]), e
    if key == "first_only":   # no token has a previous action: not one product may reach columns 1 .. A of dW_a
        assert torch.count_nonzero(g[EMB_W][:, 1:]) == 0
        assert float(c.ref[EMB_W][:, 1:].abs().max()) == 0 and float(g[EMB_W][:, 0].abs().max()) > 0
    if key == "chunks":       # fewer workgroups than tiles: some walk a second chunk
        SQ = mat_train.geometry(L)[0]
        grid = int(mat_train.lib().mdl_ct_bwd_grid(B, SQ))
        assert grid < -(-B // SQ), (grid, B, SQ)


# ------------------------------------------------------------------------------------------------ b. X lo tile
# what separates the two columns with the lo tile in place: the dropped Ylo.Xlo term and the bf16 rounding of Xlo, each
# <= 2^-18 of a product, plus fp32 accumulation order — 2^-17 with a 16-fold allowance for cancellation in the signed
# sum over tokens (tests/test_gpu_continuous_det.py).  Without the lo tile the distance is 1.3e-3.
X_LO_LIMIT = 2.0 ** -13


def test_x_lo_tile_is_used(gpu):
    """Every stored action has the continuous dimensions (37.3, 1.0) at A = 4: column 3 of dW_a is then 37.3 x column
    4, both summed over the same d pre rows in the same MFMA order.  bf16(1.0) is exact; bf16(37.3) = 37.25 is off by
    1.3e-3, which only the X lo tile brings back."""
    def const_tail(a):
        a = a.clone()
        a[..., 2], a[..., 3] = 37.3, 1.0
        return a
    c = Case(gpu, 6, 40, 4, 9, "mask", actions=const_tail)
    w = c.fused()[EMB_W]
    d = rel(w[:, 3] / c.actions[0, 0, 2], w[:, 4])
    print(f"[avail-cont] dW_a column ratio distance {d:.3e} (limit {X_LO_LIMIT:.3e})")
    assert float(w[:, 4].abs().max()) > 0
    assert d <= X_LO_LIMIT, d


# ------------------------------------------------------------------------------------------------ c. sidx
def test_minibatch_index_equals_gathered_rows(gpu):
    """Forward and backward through idx (a permutation of the buffer rows: actions and availability read in-kernel
    through the sequence index, log-probs and entropies written at the minibatch token) are bitwise the same call on
    the gathered rows."""
    c = case(gpu, "base")
    B = c.obs.shape[0]
    idx = torch.randperm(B, device=gpu, generator=torch.Generator(device=gpu).manual_seed(1))
    assert not torch.equal(idx, torch.arange(B, device=gpu))
    a = c.run(c.obs, c.actions, c.ava, idx=idx)
    b = c.run(c.obs[idx].contiguous(), c.actions[idx].contiguous(), c.ava[idx].contiguous())
    for name, x, y in zip(("gradient", "logp", "ent", "v"), a, b):
        assert bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0, name
        assert torch.equal(x, y), f"{name}: {int((x != y).sum())} elements differ"
    dense = c.run()   # and the index matters: the un-permuted rows give other values
    assert not torch.equal(a[1], dense[1])


# ------------------------------------------------------------------------------------------------ d. bitwise repeat
@pytest.mark.parametrize("key", ["chunks", "wide_obs"])
def test_bitwise_repeat_with_poisoned_workspace(gpu, key):
    """Two runs give the same flat gradient bit for bit, the second with NaN in every workspace slot beforehand: each
    slot the reduction reads was written by that launch (first-chunk stores, not read-modify-writes of stale values)."""
    c = case(gpu, key)
    a = c.run()[0]
    c.poison()
    b = c.run()[0]
    assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
    assert torch.equal(a, b), f"{int((a != b).sum())} elements differ (NaN: {int(torch.isnan(b).sum())})"


# ------------------------------------------------------------------------------------------------ e. trainer
class Available_Continous_Space:   # the reference's class name (transformer_policy.py:36)
    def __init__(self, n):
        self.shape = (n,)


def _trainer(gpu):
    """TransformerPolicy + MATTrainer + a rollout buffer filled by the fused decode: L = 7, 8 envs x 10 steps, 2 epochs x
    2 minibatches, act_out = 4, logp_dim = 3.  No env in the tree emits this action space."""
    from mat_dcml_amd.algos.buffer import RolloutBuffer
    from mat_dcml_amd.algos.mat_trainer import MATTrainer
    from mat_dcml_amd.algos.policy import TransformerPolicy
    from mat_dcml_amd.config import get_config, parse_args
    from mat_dcml_amd.parallel.comm import Comm
    L, E, T, od, A = 7, 8, 10, 10, 4
    args = parse_args(["--env_name", "DCML", "--n_block", "2", "--ppo_epoch", "2", "--num_mini_batch", "2", "--seed", "2"],
                      get_config(), warn=False)
    assert args.cuda_deterministic is True   # store_false, not passed: on, as in the reference's scripts
    torch.manual_seed(0)
    pol = TransformerPolicy(args, [od], [od], Available_Continous_Space(A), L, device=gpu)
    comm = Comm(device=gpu)
    comm.attach_flat_grads(pol.transformer.parameters())
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        tr = MATTrainer(args, pol, L, device=gpu, comm=comm)
    warned = [str(x.message) for x in w if "cuda_deterministic" in str(x.message)]
    buf = RolloutBuffer(T, E, L, od, od, A, act_out=A, logp_dim=A - 1, device=gpu)
    return pol, tr, buf, warned


def _fill(pol, buf, gpu):
    T, E, L = buf.T, buf.E, buf.A
    g = torch.Generator(device=gpu).manual_seed(11)
    buf.obs.copy_(torch.rand(buf.obs.shape, device=gpu, generator=g))
    hide = torch.rand(T + 1, E, L, device=gpu, generator=g) < 1.0 / 3.0
    which = torch.randint(0, 2, (T + 1, E, L), device=gpu, generator=g)
    buf.available_actions[..., 0] = torch.where(hide & (which == 0), 0.0, 1.0)   # never both
    buf.available_actions[..., 1] = torch.where(hide & (which == 1), 0.0, 1.0)
    buf.rewards.copy_(torch.randn(buf.rewards.shape, device=gpu, generator=g))
    mat_fused.set_sampling_key(pol.transformer, 2)
    for t in range(T):
        v, a, lp = pol.get_actions(None, buf.obs[t], buf.available_actions[t])
        assert a.shape == (E, L, 4) and lp.shape == (E, L, 3)
        buf.actions[t].copy_(a)
        buf.action_log_probs[t].copy_(lp)
        buf.value_preds[t].copy_(v)
    # the fused decode honours the masks: the stored one-hot choice is an available one
    chosen = (buf.actions[..., :2] * buf.available_actions[:-1, ..., :2]).sum(-1)
    assert bool((chosen == 1).all())


def _train_twice(gpu):
    pol, tr, buf, warned = _trainer(gpu)
    m = pol.transformer
    assert m.action_type == "Available_Continous"
    assert tr.fused, tr.fused_reason
    assert tr.deterministic is True and tr.nondeterministic_writer is None
    assert not warned, warned
    before = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).clone()
    snaps = []
    tr.prep_training()
    for _ in range(2):
        _fill(pol, buf, gpu)
        snaps.append({"actions": buf.actions.clone(), "logp": buf.action_log_probs.clone()})
        tr.train(buf)
        opt = pol.optimizer
        snaps.append({"params": torch.cat([p.detach().reshape(-1) for p in m.parameters()]).clone(),
                      "exp_avg": opt.m.clone(), "exp_avg_sq": opt.v.clone(), "scratch": opt.scratch[:4].clone()})
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in snaps[-1].values())
    assert not torch.equal(before, snaps[-1]["params"])
    assert float(snaps[-1]["scratch"][2]) == 0   # no skipped (non-finite) step
    return snaps, tr


def test_trainer_is_fused_deterministic_and_bitwise_repeatable(gpu):
    """The fused trainer accepts the action type, claims determinism without a cuda_deterministic warning, and two
    same-seed constructions agree bit for bit after each of two updates on parameters, both Adam moments and the
    optimizer scratch."""
    (a, tr), (b, _) = _train_twice(gpu), _train_twice(gpu)
    for i, (sa, sb) in enumerate(zip(a, b)):
        what = f"rollout {i // 2 + 1}" if i % 2 == 0 else f"update {i // 2 + 1}"
        for k in sa:
            assert torch.equal(sa[k], sb[k]), f"{what}: {k} differs by {(sa[k] - sb[k]).abs().max().item():.3e}"
    from mat_dcml_amd.ops.paths import kernel_report

    class _R:
        policy, trainer, envs, buffer = tr.policy, tr, None, None
    assert kernel_report(_R())["train"].startswith("hip:")


def test_trainer_without_the_switch_stays_hybrid(gpu, monkeypatch):
    monkeypatch.delenv(ENV)
    pol, tr, buf, warned = _trainer(gpu)
    assert tr.fused is False and "Available_Continuous" in tr.fused_reason and ENV in tr.fused_reason
    assert not warned


# ------------------------------------------------------------------------------------------------ f. rollout vs learner
DECODE_FACTOR = 1.5   # the project's factor for decode bounds


def test_rollout_logprobs_match_the_fused_training_forward(gpu):
    """Stochastic decode (production kernel) at B = 64, L = 7, A = 4, its own actions re-evaluated by the fused training
    forward.  Yardstick: the distance of the same decode output from the eager fp32 teacher-forced evaluation (both
    exist without this feature); the fused forward may be at most 1.5 x as far, per statistic — both forwards round
    through bf16, so their difference cannot be held below the decode's own.
    Measured (profiles/avail_cont_fused/README.md)."""
    L, B, A, od = 7, 64, 4, 9
    m = make_av(L, A, od, gpu)
    obs, _, ava, _, _, _ = make_inputs(gpu, L, B, A, od, "mask", seed=21)
    mat_fused.set_sampling_key(m, 5)
    _, a, lp_dec = mat_fused.get_actions(m, obs, ava)
    assert a.shape == (B, L, A) and lp_dec.shape == (B, L, A - 1)
    assert bool(((a[..., :2] * ava[..., :2]).sum(-1) == 1).all())
    with torch.no_grad():
        lp_eager, _, _ = m(None, obs, a, ava)
    enc, dec = mat_train.EncoderFused(m), mat_train.DecoderFused(m)
    with torch.no_grad():
        _, rep = enc.forward(obs, save=False)
        lp_fused, _ = dec.forward(rep, a, ava, save=False)
    torch.cuda.synchronize()
    d_eager, d_fused = (lp_dec - lp_eager).abs(), (lp_dec - lp_fused).abs()
    yard = (d_eager.mean().item(), d_eager.max().item())
    got = (d_fused.mean().item(), d_fused.max().item())
    print(f"[avail-cont] |d logp| decode vs eager fp32: mean {yard[0]:.3e} max {yard[1]:.3e}; "
          f"decode vs fused forward: mean {got[0]:.3e} max {got[1]:.3e}")
    assert yard[0] > 0
    assert got[0] <= DECODE_FACTOR * yard[0] and got[1] <= DECODE_FACTOR * yard[1], (got, yard)


# ------------------------------------------------------------------------------------------------ g. cost guard
def test_fused_path_is_no_slower_than_the_hybrid_path(gpu, monkeypatch):
    """evaluate_actions + backward at L = 33, B = 1600, A = 4, in one process: the hybrid path (switch unset: fused
    encoder under autograd, eager bf16 decoder) against the fused path.  The bound is the existing path's time."""
    L, B, A, od = 33, 1600, 4, 9
    m = make_av(L, A, od, gpu)
    obs, actions, ava, w1, w2, w3 = make_inputs(gpu, L, B, A, od, "mask")

    def step():
        v, lp, ent = mat_fused.evaluate_actions(m, obs, actions, ava)
        ((lp * w1).sum() + (v * w2).sum() + (ent * w3).sum()).backward()

    def measure():
        for _ in range(20):   # clocks ramp after a suite of small launches
            step()
        return median_us(step, iters=10)

    monkeypatch.delenv(ENV)
    assert not mat_train.decoder_supported(m)
    hybrid = measure()
    monkeypatch.setenv(ENV, "fused")
    assert mat_train.supported(m)
    fused = measure()
    perf_record("avail_cont_eval_bwd_hybrid_33x1600_us", hybrid, None)
    perf_record("avail_cont_eval_bwd_fused_33x1600_us", fused, round(hybrid, 1))
    print(f"[avail-cont] evaluate_actions + backward: hybrid {hybrid:.1f} us, fused {fused:.1f} us, "
          f"ratio {fused / hybrid:.3f}")
    assert fused <= hybrid, (fused, hybrid)
