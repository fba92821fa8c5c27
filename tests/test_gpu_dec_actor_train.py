"""MAT-Dec's shared actor on the fused actor kernels (csrc/mat_actor_ct.hip: mat_actor_fwd_ct / mat_actor_bwd_ct;
MAT_DCML_DEC_ACTOR_TRAIN=fused): fp64 parity of the forward outputs and of every parameter gradient through the private
gradient workspace, exact zeros (encoder gradients under dv = 0, log_std), the in-kernel minibatch index, bitwise
repeats with the workspace and the saved activations poisoned, a fused bit-reproducible trainer, rollout-vs-learner
log-probs, and a cost guard against the hybrid path's eager actor.  Measurements: profiles/dec_actor_fused/README.md."""
import contextlib
import copy
import functools
import warnings

import pytest
import torch

from conftest import median_us, perf_record
from mat_dcml_amd.models.mat import MultiAgentTransformer
from mat_dcml_amd.ops import mat_fused, mat_train, ppo_fused
from test_train_edges_helper import BWD_NW, chunk_plan, launch_grid, rel, token_stat, workgroup_walk

pytestmark = pytest.mark.gpu

ENV = "MAT_DCML_DEC_ACTOR_TRAIN"

# key: (L, B, obs_dim, A, action type, n_block, availability).  B = None: the multi-chunk count (_ragged_B).
# availability: "half" = half the rows with one (not the stored) action masked, "random" = random masks that keep the
# stored action (so never all-masked), "ones", None = no availability tensor
CASES = {
    "one_token": (1, 1, 7, 2, "Semi_Discrete", 2, "ones"),       # one token, which is the continuous agent
    "tile_plus_1": (17, 1, 7, 2, "Semi_Discrete", 2, "ones"),    # 16-row tile plus one
    "dcml": (33, 40, 7, 2, "Semi_Discrete", 2, "half"),
    "od5": (5, 24, 5, 5, "Discrete", 2, "ones"),                 # od not a multiple of 4
    "od16_A17": (3, 24, 16, 17, "Discrete", 2, "ones"),          # full od; second logit tile of one column
    "A36": (27, 8, 16, 36, "Discrete", 2, "random"),             # three logit tiles
    "A64": (4, 16, 9, 64, "Discrete", 2, "ones"),                # four logit tiles
    "cont_A1": (6, 24, 11, 1, "Continuous", 2, None),
    "cont_A17": (6, 24, 11, 17, "Continuous", 2, None),
    "ragged": (33, None, 7, 2, "Semi_Discrete", 2, "half"),      # every backward workgroup walks >= 2 chunks
    "nb1": (33, 40, 7, 2, "Semi_Discrete", 1, "half"),           # encoder depth only
}
LOG_STD = "decoder.log_std"
INPUT_SEED = 7


def n_cu(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _ragged_B(dev, L=33):
    """6 n_CU + 7 sequences: every backward workgroup owns 6 or 7 sequences = two chunks (3 + 3 or 3 + 4; SQ = 5), the
    odd groups of 8 workgroups walk theirs reversed, and the chunks end inside a 16-row tile (99 / 132 rows)."""
    return 6 * n_cu(dev) + 7


def _shape(dev, key):
    L, B, od, A, kind, nb, av = CASES[key]
    return L, (_ragged_B(dev, L) if B is None else B), od, A, kind, nb, av


def make_actor(L, od, A, kind, n_block, dev, seed=4, scale=0.2):
    """A MAT-Dec model away from its initialisation: Linear weights / biases N(0, scale²), LayerNorm gains 1 + 0.1 N,
    LayerNorm biases and log_std 0.1 / 0.3 N (the sibling tests' recipe)."""
    torch.manual_seed(seed)
    m = MultiAgentTransformer(od, od, A, L, n_block, 64, 2, action_type=kind, dec_actor=True, share_actor=True).to(dev)
    g0 = torch.Generator().manual_seed(seed)
    lns = {id(p) for mod in m.modules() if isinstance(mod, torch.nn.LayerNorm) for p in mod.parameters()}
    with torch.no_grad():
        for n, p in m.named_parameters():
            r = torch.randn(p.shape, generator=g0)
            if id(p) in lns:
                p.copy_((1.0 + 0.1 * r if n.endswith("weight") else 0.1 * r).to(dev))
            elif n.endswith("log_std"):
                p.copy_((0.3 * r).to(dev))
            else:
                p.copy_((scale * r).to(dev))
    return m


def n_disc_of(kind, L):
    return L if kind == "Discrete" else 0 if kind == "Continuous" else L - 1


def make_inputs(dev, L, B, od, A, kind, av, seed=INPUT_SEED):
    g = torch.Generator(device=dev).manual_seed(seed)
    obs = torch.rand(B, L, od, device=dev, generator=g)
    nd = n_disc_of(kind, L)
    if kind == "Continuous":
        actions = torch.randn(B, L, A, device=dev, generator=g) * 0.5
    else:
        actions = torch.randint(0, A, (B, L, 1), device=dev, generator=g).float()
        if nd < L:
            actions[:, nd:] = torch.randn(B, L - nd, 1, device=dev, generator=g) * 0.5
    ava = None
    if av is not None and kind != "Continuous":
        ava = torch.ones(B, L, A, device=dev)
        pick = actions[:, :nd, 0].long()
        if av == "half" and nd > 0:   # one action that is not the stored one, on half of the sequences
            other = (pick + 1 + torch.randint(0, A - 1, pick.shape, device=dev, generator=g)) % A
            hide = (torch.arange(B, device=dev) % 2 == 0).view(B, 1).expand(B, nd)
            ava[:, :nd].scatter_(-1, other.unsqueeze(-1), torch.where(hide, 0.0, 1.0).unsqueeze(-1))
            assert float(ava[:, :nd].sum(-1).min()) == A - 1 and float(ava[1::2].min() if B > 1 else 1.0) == 1.0
        if av == "random" and nd > 0:
            ava[:, :nd] = (torch.rand(B, nd, A, device=dev, generator=g) < 0.5).float()
            ava[:, :nd].scatter_(-1, pick.unsqueeze(-1), 1.0)
            assert 0.2 < float(ava[:, :nd].mean()) < 0.8
        if nd > 0:
            assert bool((ava[:, :nd].gather(-1, pick.unsqueeze(-1)) == 1).all())
    nlp = A if kind == "Continuous" else 1
    w1, w3 = (torch.randn(B, L, nlp, device=dev, generator=g) for _ in range(2))
    w2 = torch.randn(B, L, 1, device=dev, generator=g)
    return obs, actions, ava, w1, w2, w3


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
    """(gradients, (logp, ent, v)) of the weighted-sum loss through the eager model."""
    m.zero_grad()
    lp, v, ent = m(None, obs, actions, ava)
    ((lp.to(w1.dtype) * w1).sum() + (v.to(w2.dtype) * w2).sum() + (ent.to(w3.dtype) * w3).sum()).backward()
    return ({n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None},
            (lp.detach().clone(), ent.detach().clone(), v.detach().clone()))


class Case:
    """One shape: inputs, the fp64 and bf16-autocast references of the eager model (computed once), and the fused
    kernels wired to a private gradient workspace."""

    def __init__(self, dev, L, B, od, A, kind, nb, av, refs=True):
        m = self.m = make_actor(L, od, A, kind, nb, dev)
        self.kind, self.L = kind, L
        self.obs, self.actions, self.ava, self.w1, self.w2, self.w3 = make_inputs(dev, L, B, od, A, kind, av)
        args = (self.obs, self.actions, self.ava, self.w1, self.w2, self.w3)
        if refs:
            d = lambda t: None if t is None else t.double()  # noqa: E731
            m64 = copy.deepcopy(m).double()
            with _float_keeps_fp64():
                self.ref, self.out_ref = _loss_grads(m64, *[d(t) for t in args])
                # the loss without its value term (dv = 0): which gradients fp64 autograd gives as exactly zero
                self.ref_nov, _ = _loss_grads(m64, *[d(t) for t in args[:4]], torch.zeros_like(self.w2).double(), d(self.w3))
            assert all(r.dtype == torch.float64 for r in self.ref.values())
            del m64
            with torch.autocast("cuda", dtype=torch.bfloat16):
                refb, outb = _loss_grads(m, *args)
            self.bf16_err = {n: rel(refb[n], self.ref[n]) for n in self.ref}
            self.bf16_out_err = tuple(token_stat(b.float(), r) for b, r in zip(outb, self.out_ref))
        m.zero_grad()
        ppo_fused.flatten_params(m)
        self.fg = torch.zeros_like(m._mdl_flat_params)
        self.offsets = ppo_fused.param_offsets(m)
        for p, off in self.offsets:
            p.grad = self.fg[off:off + p.numel()].view_as(p)
        self.enc = mat_train.EncoderFused(m)
        self.act = mat_train.ActorFused(m, self.enc)
        self.ws = mat_train.attach_grad_workspace(m, self.fg, mode="private")
        self.grads = self.out = None

    def poison(self):
        """NaN in every workspace slot of every copy that a backward launch is to write, and in the saved activations
        of the last forward (the next forward must rewrite every record its backward reads)."""
        _, _, stride, copies = self.m._mdl_gws_buf
        ws = self.ws.view(copies, stride)
        for (name, p), (_, off) in zip(self.m.named_parameters(), self.offsets):
            if name in self.ref:
                ws[:, off:off + p.numel()] = float("nan")
        for ctx in (self.last_saves or ()):
            for t in ctx:
                t.fill_(float("nan"))

    last_saves = None

    def run(self, obs=None, actions=None, ava=None, idx=None, dv=None):
        """Fused forward + backward + reduction -> (flat gradient, logp, ent, v)."""
        m = self.m
        if obs is None:
            obs, actions, ava = self.obs, self.actions, self.ava
        self.fg.zero_()
        m._mdl_gws_active = True
        try:
            v, rep = self.enc.forward(obs, idx=idx)
            logp, ent = self.act.forward(rep, actions, ava, idx=idx)
            self.last_saves = (self.enc.ctx.saves, self.act.ctx.saves)
            drep = self.act.backward(self.w1, self.w3)
            assert drep.shape == rep.shape and float(drep.abs().max()) == 0
            self.enc.backward(drep, self.w2 if dv is None else dv)
        finally:
            m._mdl_gws_active = False
        mat_train.reduce_grad_workspace(m, accumulate=False)
        torch.cuda.synchronize()
        return self.fg.clone(), logp.clone(), ent.clone(), v.clone()

    def named(self, flat):
        return {n: flat[off:off + p.numel()].view_as(p) for (n, p), (_, off) in zip(self.m.named_parameters(), self.offsets)}

    def fused(self):
        if self.grads is None:
            flat, logp, ent, v = self.run()
            self.out = (logp, ent, v)
            self.grads = self.named(flat)
        return self.grads


@functools.lru_cache(maxsize=None)
def case(dev, key):
    return Case(dev, *_shape(dev, key))


@pytest.fixture(autouse=True)
def _fused_switch(monkeypatch):
    monkeypatch.setenv(ENV, "fused")


def test_ragged_case_walks_two_chunks_everywhere(gpu):
    """The multi-chunk count does what its case is for (the helper's mirror of FOR_TILES / chunk_plan / stagger)."""
    L, B = 33, _ragged_B(gpu)
    SQ = mat_train.geometry(L)[0]
    grid = launch_grid(B, SQ, n_cu(gpu), True)
    assert grid == int(mat_train.lib().mdl_ct_bwd_grid(B, SQ)) == n_cu(gpu)
    walks = [workgroup_walk(B, SQ, L, grid, w, True) for w in range(grid)]
    assert all(len(w) >= 2 for w in walks), min(len(w) for w in walks)
    assert grid > 8 and walks[0][0][0] < walks[0][-1][0] and walks[8][0][0] > walks[8][-1][0]   # group 1 reversed
    last = walks[-1][-1] if not ((grid - 1) >> 3) & 1 else walks[-1][0]
    assert (last[1] * L) % 16 != 0 and last[0] + last[1] == B
    assert abs(chunk_plan(B * 1 // grid, SQ, L, BWD_NW)) >= 2


# ------------------------------------------------------------------------------------------------ a. fp64 parity
@pytest.mark.parametrize("key", list(CASES))
def test_outputs_and_every_gradient_match_fp64_autograd(gpu, key):
    """mat_train's fused forward / backward (encoder + actor kernels, gradients through the private workspace) against
    fp64 autograd of the eager model.  Outputs by max |k - ref| / (1 + |ref|) within max(3e-2, 2.5 x the bf16-autocast
    eager model's figure); gradients by rel() within max(6e-2, 2.5 x autocast's); gradients that are exactly zero in
    fp64 (attention key biases; query / key weights at L = 1) by the absolute rule of the sibling tests (8e-2 of the
    key- or value-weight gradient).  Worst error / limit per case: profiles/dec_actor_fused/README.md."""
    c = case(gpu, key)
    L, B, od, A, kind, nb, av = _shape(gpu, key)
    assert mat_train.supported(c.m) and mat_train.dec_actor_fused(c.m)
    g = c.fused()
    nlp = A if kind == "Continuous" else 1
    assert c.out[0].shape == (B, L, nlp) and c.out[1].shape == (B, L, nlp) and c.out[2].shape == (B, L, 1)
    margins = []
    for name, k, r, y in zip(("logp", "ent", "v"), c.out, c.out_ref, c.bf16_out_err):
        assert bool(torch.isfinite(k).all()), name
        e, lim = token_stat(k, r), max(3e-2, 2.5 * y)
        margins.append((e / lim, name, e, lim))
    bad = [x for x in margins if not x[2] <= x[3]]
    for n, r in c.ref.items():
        assert bool(torch.isfinite(g[n]).all()), n
        if "key.bias" in n or float(r.abs().max()) == 0:
            if ".attn" in n:
                att = n.rsplit(".", 2)[0]
                scale = c.ref[att + ".key.weight"].abs().max().item() or c.ref[att + ".value.weight"].abs().max().item()
            else:
                scale = max(x.abs().max().item() for x in c.ref.values())
            e, lim = (g[n] - r).abs().max().item() / (scale + 1e-6), 8e-2
        else:
            e, lim = rel(g[n], r), max(6e-2, 2.5 * c.bf16_err[n])
        margins.append((e / lim, n, e, lim))
        if not e <= lim:
            bad.append((e / lim, n, e, lim))
    worst = sorted(margins, reverse=True)[:3]
    print(f"[dec-actor] {key}: worst error / limit", [(round(x[0], 3), x[1]) for x in worst])
    assert not bad, bad
    # every parameter of the actor has a gradient in the reference, and nothing else of the decoder exists
    assert {n for n in c.ref if n.startswith("decoder.")} == {n for n, _ in c.m.decoder.named_parameters(prefix="decoder")}


# ------------------------------------------------------------------------------------------------ b. exact zeros
@pytest.mark.parametrize("key", ["dcml", "one_token", "cont_A17", "A36"])
def test_exact_zeros(gpu, key):
    """A loss of log-prob and entropy only (dv = 0): the actor does not read rep, so every encoder parameter gradient is
    exactly 0.0 (a garbage d rep would show here).  And every log_std.grad entry that fp64 autograd gives as exactly
    zero is exactly zero (Semi_Discrete: all but the last)."""
    c = case(gpu, key)
    g = c.named(c.run(dv=torch.zeros_like(c.w2))[0])
    for n, t in g.items():
        if n.startswith("encoder."):
            assert torch.count_nonzero(t) == 0, (n, float(t.abs().max()))
    assert all(float(r.abs().max()) == 0 for n, r in c.ref_nov.items() if n.startswith("encoder."))
    assert any(float(g[n].abs().max()) > 0 for n in g if n.startswith("decoder.mlp"))
    if LOG_STD in c.ref:
        zero = c.ref[LOG_STD] == 0
        full = c.fused()[LOG_STD]
        assert torch.count_nonzero(full[zero]) == 0 and torch.count_nonzero(g[LOG_STD][zero]) == 0, full
        assert bool((full[~zero] != 0).all())
        if c.kind == "Semi_Discrete":
            assert zero.tolist() == [True] * (zero.numel() - 1) + [False]
        if c.kind == "Continuous":
            assert not bool(zero.any())


# ------------------------------------------------------------------------------------------------ c. sidx
@pytest.mark.parametrize("key", ["dcml", "cont_A17", "A36"])
def test_minibatch_index_equals_gathered_rows(gpu, key):
    """Observations, actions and availability read in-kernel through the sequence index give bit for bit the call on
    the gathered rows."""
    c = case(gpu, key)
    B = c.obs.shape[0]
    idx = torch.randperm(B, device=gpu, generator=torch.Generator(device=gpu).manual_seed(1))
    assert not torch.equal(idx, torch.arange(B, device=gpu))
    gat = lambda t: None if t is None else t[idx].contiguous()  # noqa: E731
    a = c.run(c.obs, c.actions, c.ava, idx=idx)
    b = c.run(gat(c.obs), gat(c.actions), gat(c.ava))
    for name, x, y in zip(("gradient", "logp", "ent", "v"), a, b):
        assert bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0, name
        assert torch.equal(x, y), f"{name}: {int((x != y).sum())} elements differ"
    assert not torch.equal(a[1], c.run()[1])   # and the index matters


# ------------------------------------------------------------------------------------------------ d. bitwise repeat
@pytest.mark.parametrize("key", ["dcml", "ragged"])
def test_bitwise_repeat_with_poisoned_workspace_and_saves(gpu, key):
    c = case(gpu, key)
    a = c.run()[0]
    c.poison()
    b = c.run()[0]
    assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
    assert torch.equal(a, b), f"{int((a != b).sum())} elements differ (NaN: {int(torch.isnan(b).sum())})"


# ------------------------------------------------------------------------------------------------ e. trainer
def _runner(gpu):
    from mat_dcml_amd.config import get_config, parse_args
    from mat_dcml_amd.parallel.comm import Comm
    from mat_dcml_amd.runner.dcml_runner import DCMLRunner
    args = parse_args(["--env_name", "DCML", "--algorithm_name", "mat_dec", "--n_workers", "8", "--n_rollout_threads",
                       "4", "--episode_length", "4", "--ppo_epoch", "2", "--num_mini_batch", "2", "--use_valuenorm"],
                      get_config(), warn=False)
    args.dec_actor, args.share_actor = True, True
    assert args.cuda_deterministic is True
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = DCMLRunner({"all_args": args, "device": gpu, "run_dir": None, "comm": Comm(device=gpu)})
    return r, [str(x.message) for x in w if "cuda_deterministic" in str(x.message)]


def _train_twice(gpu):
    from mat_dcml_amd.ops.paths import kernel_report
    r, warned = _runner(gpu)
    tr, m = r.trainer, r.policy.transformer
    assert r.policy._fused(), mat_fused.unsupported_reasons(m)
    assert tr.fused, tr.fused_reason
    assert tr.deterministic is True and tr.nondeterministic_writer is None
    assert not warned, warned
    rep = kernel_report(r)
    assert rep["train"] == "hip:mat_enc_fwd/bwd+mat_actor_fwd/bwd+ppo_loss+adam", rep
    assert rep["decode"] == "hip:mat_actor_fwd", rep
    before = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).clone()
    r.warmup()
    for _ in range(2):
        infos = r.train_iteration()
        assert all(torch.isfinite(torch.as_tensor(float(v))) for v in infos.values()), infos
    torch.cuda.synchronize()
    opt = r.policy.optimizer
    snap = {"params": torch.cat([p.detach().reshape(-1) for p in m.parameters()]).clone(), "exp_avg": opt.m.clone(),
            "exp_avg_sq": opt.v.clone(), "scratch": opt.scratch[:4].clone()}
    assert all(bool(torch.isfinite(v).all()) for v in snap.values())
    assert not torch.equal(before, snap["params"])
    actor = [p for n, p in m.named_parameters() if n.startswith("decoder.mlp")]
    assert opt.m.numel() == m._mdl_flat_params.numel()
    assert all(float(opt.m[off:off + p.numel()].abs().max()) > 0 for p, off in ppo_fused.param_offsets(m)
               if any(p is q for q in actor)), "an actor parameter never received a gradient"
    assert m._mdl_train_state[0].ctx is None and m._mdl_train_state[1].ctx is None
    assert isinstance(m._mdl_train_state[1], mat_train.ActorFused)
    return snap


def test_trainer_is_fused_deterministic_and_bitwise_repeatable(gpu):
    """The DCML runner with --algorithm_name mat_dec: a fused trainer that claims determinism without a
    cuda_deterministic warning, reports the actor kernels, and two same-seed constructions agree bit for bit after two
    train_iteration()s on parameters, both Adam moments and the optimizer scratch."""
    a, b = _train_twice(gpu), _train_twice(gpu)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k} differs by {(a[k] - b[k]).abs().max().item():.3e}"


def test_trainer_without_the_switch_stays_hybrid(gpu, monkeypatch):
    monkeypatch.delenv(ENV)
    r, warned = _runner(gpu)
    assert r.trainer.fused is False and ENV in r.trainer.fused_reason and not r.policy._fused() and not warned


# ------------------------------------------------------------------------------------------------ f. rollout vs learner
def test_rollout_logprobs_match_the_learner(gpu):
    """get_actions (logits from mat_actor_fwd_ct, heads on keyed draws) and the learner's forward on the same actions at
    33 x 64, weights away from init: mean |d log p| between them is at most the learner's own mean distance from the
    fp32 eager model (both numbers: profiles/dec_actor_fused/README.md).  Sampled discrete actions respect the mask."""
    L, B, od, A = 33, 64, 7, 2
    m = make_actor(L, od, A, "Semi_Discrete", 2, gpu)
    obs, _, ava, _, _, _ = make_inputs(gpu, L, B, od, A, "Semi_Discrete", "half", seed=21)
    ava[::2, : L - 1, 1] = 0.0   # half of the sequences: action 1 unavailable to every discrete agent
    ava[::2, : L - 1, 0] = 1.0
    assert mat_fused.supports(m)
    mat_fused.set_sampling_key(m, 5)
    v, a, lp_roll = mat_fused.get_actions(m, obs, ava)
    assert a.shape == (B, L, 1) and lp_roll.shape == (B, L, 1) and v.shape == (B, L, 1)
    pick = a[:, : L - 1, 0].long()
    assert bool((ava[:, : L - 1].gather(-1, pick.unsqueeze(-1)) == 1).all())
    assert 0 < int(pick[1::2].sum()) < pick[1::2].numel() and int(pick[::2].sum()) == 0
    with torch.no_grad():
        lp_eager, _, _ = m(None, obs, a, ava)
        enc = mat_train.EncoderFused(m)
        act = mat_train.ActorFused(m, enc)
        _, rep = enc.forward(obs, save=False)
        lp_learn, _ = act.forward(rep, a, ava, save=False)
    torch.cuda.synchronize()
    d_roll, yard = (lp_roll - lp_learn).abs().mean().item(), (lp_learn - lp_eager).abs().mean().item()
    print(f"[dec-actor] mean |d logp| rollout vs learner {d_roll:.3e}; learner vs eager fp32 {yard:.3e}")
    assert bool(torch.isfinite(lp_roll).all()) and yard > 0
    assert d_roll <= yard, (d_roll, yard)


# ------------------------------------------------------------------------------------------------ g. cost guard
def test_fused_actor_is_faster_than_the_hybrid_paths_eager_actor(gpu, monkeypatch):
    """Actor forward + backward at 3,200 x 33 (od 7, A 2, Semi_Discrete): the fused kernels (private workspace, as the
    trainer runs them) against the hybrid path's eager bf16-autocast actor with autograd, measured in one process."""
    from mat_dcml_amd.models import act as act_mod
    L, B, od, A = 33, 3200, 7, 2
    c = Case(gpu, L, B, od, A, "Semi_Discrete", 2, "half", refs=False)
    m = c.m
    v, rep = c.enc.forward(c.obs, save=False)

    def fused():
        c.act.forward(rep, c.actions, c.ava, obs=c.obs)
        c.act.backward(c.w1, c.w3)

    def hybrid():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            lp, ent = act_mod.parallel_act(m, rep, c.obs, c.actions, c.ava)
        ((lp.float() * c.w1).sum() + (ent.float() * c.w3).sum()).backward()

    def measure(fn):
        for _ in range(20):   # clocks ramp after a suite of small launches
            fn()
        return median_us(fn, iters=10)

    assert mat_train.dec_actor_fused(m)
    m._mdl_gws_active = True
    try:
        t_fused = measure(fused)
    finally:
        m._mdl_gws_active = False
        m._mdl_gws_grid = None
    monkeypatch.setenv(ENV, "hybrid")
    assert not mat_train.decoder_supported(m)
    t_hybrid = measure(hybrid)
    perf_record("dec_actor_fwd_bwd_hybrid_33x3200_us", t_hybrid, None)
    perf_record("dec_actor_fwd_bwd_fused_33x3200_us", t_fused, round(t_hybrid, 1))
    print(f"[dec-actor] actor forward + backward: hybrid {t_hybrid:.1f} us, fused {t_fused:.1f} us, "
          f"ratio {t_fused / t_hybrid:.3f}")
    assert t_fused < t_hybrid, (t_fused, t_hybrid)
