"""MAT-Dec's shared actor on wide observations (obs_dim > 16; MAT_DCML_DEC_ACTOR_TRAIN=fused and
MAT_DCML_DEC_ACTOR_WIDE_OBS=fused): csrc/obs_embed.hip computes the actor's embedding pre-activation and the W_1 / b_1 /
LN_obs gradients, the WIDE instantiations of csrc/mat_actor_ct.hip (mat_actor_fwd_ct_wide / mat_actor_bwd_ct_wide) the
rest.  fp64 parity of the outputs and of every parameter gradient, exact zeros, the minibatch index, bitwise repeats
with every workspace poisoned (the partial workspace the encoder's and the actor's embedding share included), fused
bit-reproducible SMAC and MPE trainers, rollout-vs-learner log-probs, and a cost guard against the hybrid path's eager
actor.  Measurements: profiles/dec_actor_wide/README.md.

The kernel-level cases read fp32 observations (mat_train.WIDE_OBS_BF16 off for the call) unless they say bf16; the
trainers run the default (bf16 wide observations)."""
import functools
import warnings

import pytest
import torch

from conftest import median_us, perf_record
from mat_dcml_amd.ops import mat_fused, mat_train, ppo_fused
from test_gpu_dec_actor_train import ENV, LOG_STD, Case, _ragged_B, make_actor, make_inputs
from test_train_edges_helper import rel, token_stat

pytestmark = pytest.mark.gpu

WIDE = "MAT_DCML_DEC_ACTOR_WIDE_OBS"

# key: (L, B, obs_dim, A, action type, n_block, availability) as in tests/test_gpu_dec_actor_train.py
CASES = {
    "one_token": (1, 1, 17, 2, "Semi_Discrete", 2, "ones"),     # a single token
    "od17": (3, 24, 17, 5, "Discrete", 2, "ones"),              # one column past the in-kernel limit
    "mpe": (3, 24, 18, 5, "Discrete", 1, "ones"),               # MPE's width, one block
    "od33": (17, 2, 33, 2, "Semi_Discrete", 2, "half"),         # second 32-wide k-step of one column; 16-row tile + rows
    "od65_A36": (27, 8, 65, 36, "Discrete", 2, "random"),       # second 64-column block of one column; three logit tiles
    "smac": (27, 4, 1288, 36, "Discrete", 2, "random"),         # SMAC (fp32 observations; once more with bf16)
    "cont": (6, 24, 23, 17, "Continuous", 2, None),             # Continuous head
    "ragged": (33, None, 17, 2, "Semi_Discrete", 2, "half"),    # every backward workgroup walks two chunks
}
# the parameters whose gradients csrc/obs_embed.hip adds straight into .grad, outside the private workspace
ACTOR_EMB = ("decoder.mlp.0.weight", "decoder.mlp.0.bias", "decoder.mlp.1.weight", "decoder.mlp.1.bias")
DIRECT = ACTOR_EMB + ("encoder.obs_encoder.0.weight", "encoder.obs_encoder.0.bias", "encoder.obs_encoder.1.weight",
                      "encoder.obs_encoder.1.bias")


@pytest.fixture(autouse=True)
def _both_switches(monkeypatch):
    monkeypatch.setenv(ENV, "fused")
    monkeypatch.setenv(WIDE, "fused")


def _shape(dev, key):
    L, B, od, A, kind, nb, av = CASES[key]
    return L, (_ragged_B(dev, L) if B is None else B), od, A, kind, nb, av


class WCase(Case):
    """The sibling file's Case with the wide paths' two differences: the obs-embedding backwards add into .grad
    directly (so the reduction accumulates onto the zeroed flat buffer, as the trainer's _direct_grads does), and there
    is more to poison."""

    def embeds(self):
        return (self.enc.obs_embed(), self.act.obs_embed())

    def poison(self):
        """NaN in every workspace slot a backward launch is to write (not the obs-embedding parameters', which are
        never read from the copies' sum: see run), the saved activations, ``pre`` / ``stat`` of both embeddings, the
        shared Mp / up partials and each instance's M / u sums."""
        _, _, stride, copies = self.m._mdl_gws_buf
        ws = self.ws.view(copies, stride)
        for (name, p), (_, off) in zip(self.m.named_parameters(), self.offsets):
            if name in self.ref and name not in DIRECT:
                ws[:, off:off + p.numel()] = float("nan")
        for t in self.last_saves:
            t.fill_(float("nan"))
        e, a = self.embeds()
        assert e.Mp is not None and e.Mp is a.Mp and e.up is a.up and e.M is not a.M   # one partial workspace
        for t in (e.Mp, e.up, e.M, e.ud, a.M, a.ud):
            t.fill_(float("nan"))

    def run(self, obs=None, actions=None, ava=None, idx=None, dv=None, bf16=False, emb_mode="partials"):
        """Fused forward + backward + reduction -> (flat gradient, logp, ent, v)."""
        m = self.m
        if obs is None:
            obs, actions, ava = self.obs, self.actions, self.ava
        if bf16:
            obs = obs.to(torch.bfloat16)
        self.fg.zero_()
        m._mdl_gws_active = True
        was = mat_train.WIDE_OBS_BF16
        mat_train.WIDE_OBS_BF16 = bf16
        for e in self.embeds():
            e.grad_mode = emb_mode
        try:
            v, rep = self.enc.forward(obs, idx=idx)
            logp, ent = self.act.forward(rep, actions, ava, idx=idx)
            ec, ac = self.enc.ctx, self.act.ctx
            assert ec.obs.dtype == ac.obs.dtype == (torch.bfloat16 if bf16 else torch.float32)
            assert ac.pre is not None and ac.pre.shape == (rep.shape[0] * rep.shape[1], 64) and ac.pre is not ec.pre
            self.last_saves = list(ec.saves) + list(ac.saves) + [ec.pre, ec.stat, ac.pre, ac.stat]
            drep = self.act.backward(self.w1, self.w3)
            assert drep.shape == rep.shape and torch.count_nonzero(drep) == 0
            self.enc.backward(drep, self.w2 if dv is None else dv)
        finally:
            m._mdl_gws_active = False
            mat_train.WIDE_OBS_BF16 = was
            for e in self.embeds():
                e.grad_mode = "partials"
        mat_train.reduce_grad_workspace(m, accumulate=True)   # onto the embeddings' direct .grad writes
        torch.cuda.synchronize()
        return self.fg.clone(), logp.clone(), ent.clone(), v.clone()


@functools.lru_cache(maxsize=None)
def case(dev, key):
    return WCase(dev, *_shape(dev, key))


# ------------------------------------------------------------------------------------------------ a. fp64 parity
def _parity(c, key, flat, out, shape):
    L, B, od, A, kind, nb, av = shape
    g = c.named(flat)
    nlp = A if kind == "Continuous" else 1
    assert out[0].shape == (B, L, nlp) and out[1].shape == (B, L, nlp) and out[2].shape == (B, L, 1)
    margins = []
    for name, k, r, y in zip(("logp", "ent", "v"), out, c.out_ref, c.bf16_out_err):
        assert bool(torch.isfinite(k).all()), name
        e, lim = token_stat(k, r), max(3e-2, 2.5 * y)
        margins.append((e / lim, name, e, lim))
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
    worst = sorted(margins, reverse=True)[:3]
    print(f"[dec-actor-wide] {key}: worst error / limit", [(round(x[0], 3), x[1]) for x in worst])
    return [x for x in margins if not x[2] <= x[3]]


def _emb_rule(c, key, part, atom):
    """tests/test_gpu_obs_embed_det.py's rule for the four obs-embedding gradients: against fp64 the fixed-order
    partial sums are no worse than the fp32 atomics (+ 1e-5), and differ from them by a pure fp32 summation-order
    difference (< 1e-5); every error over norm + 1e-3 x the four gradients' global norm."""
    ref = [c.ref[n] for n in ACTOR_EMB]
    floor = 1e-3 * torch.stack([r.norm() for r in ref]).norm()
    bad = []
    for n, r in zip(ACTOR_EMB, ref):
        err = {k: ((g[n].double() - r).norm() / (r.norm() + floor)).item() for k, g in (("partials", part), ("atomic", atom))}
        a = atom[n].double()
        d = ((part[n].double() - a).norm() / (a.norm() + floor)).item()
        print(f"[dec-actor-wide] {key} {n}: vs fp64 partials {err['partials']:.3e} atomic {err['atomic']:.3e}; "
              f"partials vs atomic {d:.3e}")
        if not (err["partials"] <= err["atomic"] + 1e-5 and d < 1e-5):
            bad.append((n, err, d))
    return bad


@pytest.mark.parametrize("key", list(CASES))
def test_outputs_and_every_gradient_match_fp64_autograd(gpu, key):
    """The fused forward / backward (encoder, actor and both obs-embedding kernels, gradients through the private
    workspace) against fp64 autograd of the eager model, by the sibling file's rules: outputs within max(3e-2, 2.5 x the
    bf16-autocast eager figure), gradients within max(6e-2, 2.5 x autocast's), the absolute rule for fp64-exact zeros;
    ``decoder.mlp.0.*`` / ``decoder.mlp.1.*`` by those and by tests/test_gpu_obs_embed_det.py's rule (_emb_rule).  Worst error /
    limit per case: profiles/dec_actor_wide/README.md."""
    c = case(gpu, key)
    shape = _shape(gpu, key)
    assert shape[2] > mat_train.MAX_FUSED_OBS
    assert mat_train.supported(c.m) and mat_train.dec_actor_fused(c.m) and mat_fused.supports(c.m)
    flat, *out = c.run()
    c.grads, c.out = c.named(flat), tuple(out)
    bad = _parity(c, key, flat, out, shape)
    atom = c.named(c.run(emb_mode="atomic")[0])
    bad += _emb_rule(c, key, c.grads, atom)
    assert not bad, bad
    # every parameter of the actor has a gradient in the reference, and nothing else of the decoder exists
    assert {n for n in c.ref if n.startswith("decoder.")} == {n for n, _ in c.m.decoder.named_parameters(prefix="decoder")}
    assert set(ACTOR_EMB) <= set(c.ref) and all(float(c.grads[n].abs().max()) > 0 for n in ACTOR_EMB)


def test_smac_bf16_observations_match_fp64_autograd(gpu):
    """SMAC's shape once more on bf16 observations (what the trainer hands over): same reference, same rules."""
    c = case(gpu, "smac")
    flat, *out = c.run(bf16=True)
    bad = _parity(c, "smac[bf16]", flat, out, _shape(gpu, "smac"))
    bad += _emb_rule(c, "smac[bf16]", c.named(flat), c.named(c.run(bf16=True, emb_mode="atomic")[0]))
    assert not bad, bad
    assert not torch.equal(flat, c.run()[0])   # and the rounding of the observations is really there


# ------------------------------------------------------------------------------------------------ b. exact zeros
@pytest.mark.parametrize("key", ["one_token", "od65_A36", "smac", "cont"])
def test_exact_zeros(gpu, key):
    """dv = 0: the actor does not read rep, so every encoder gradient is exactly 0.0 — encoder.obs_encoder included,
    through its obs-embedding backward on an all-zero d pre — and d rep is exactly zero (asserted by run).  log_std.grad
    is exactly zero wherever fp64 autograd says so."""
    c = case(gpu, key)
    g = c.named(c.run(dv=torch.zeros_like(c.w2))[0])
    enc_names = [n for n in g if n.startswith("encoder.")]
    assert any(n.startswith("encoder.obs_encoder") for n in enc_names)
    for n in enc_names:
        assert torch.count_nonzero(g[n]) == 0, (n, float(g[n].abs().max()))
    assert all(float(r.abs().max()) == 0 for n, r in c.ref_nov.items() if n.startswith("encoder."))
    assert all(float(g[n].abs().max()) > 0 for n in ACTOR_EMB)
    if LOG_STD in c.ref:
        zero = c.ref[LOG_STD] == 0
        full = c.named(c.run()[0])[LOG_STD]
        assert torch.count_nonzero(full[zero]) == 0 and torch.count_nonzero(g[LOG_STD][zero]) == 0, full
        assert bool((full[~zero] != 0).all())
        if c.kind == "Semi_Discrete":
            assert zero.tolist() == [True] * (zero.numel() - 1) + [False]
        if c.kind == "Continuous":
            assert not bool(zero.any())


# ------------------------------------------------------------------------------------------------ c. minibatch index
@pytest.mark.parametrize("key", ["od65_A36", "cont"])
def test_minibatch_index_equals_gathered_rows(gpu, key):
    """Under ``idx`` the observations are gathered to dense rows for the obs-embedding kernels while actions and
    availability are read in-kernel through the index: bit for bit the call on the gathered rows."""
    c = case(gpu, key)
    B = c.obs.shape[0]
    idx = torch.randperm(B, device=gpu, generator=torch.Generator(device=gpu).manual_seed(1))
    assert not torch.equal(idx, torch.arange(B, device=gpu))
    gat = lambda t: None if t is None else t[idx].contiguous()  # noqa: E731
    a = c.run(c.obs, c.actions, c.ava, idx=idx)
    assert c.act.ctx.idx is idx and c.enc.ctx.gathered is idx and c.act.ctx.obs is c.enc.ctx.obs   # one gather
    b = c.run(gat(c.obs), gat(c.actions), gat(c.ava))
    for name, x, y in zip(("gradient", "logp", "ent", "v"), a, b):
        assert bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0, name
        assert torch.equal(x, y), f"{name}: {int((x != y).sum())} elements differ"
    assert not torch.equal(a[1], c.run()[1])   # and the index matters


# ------------------------------------------------------------------------------------------------ d. bitwise repeats
@pytest.mark.parametrize("key", ["od33", "ragged", "smac"])
def test_bitwise_repeat_with_every_workspace_poisoned(gpu, key):
    """Same inputs, same bits — with the gradient workspace, the saved activations, ``pre`` and the shared Mp / up
    partials NaN-filled in between: each obs-embedding instance rewrites every partial it reads."""
    c = case(gpu, key)
    a = c.run()
    c.poison()
    b = c.run()
    for name, x, y in zip(("gradient", "logp", "ent", "v"), a, b):
        assert bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0, name
        assert torch.equal(x, y), f"{name}: {int((x != y).sum())} elements differ (NaN: {int(torch.isnan(y).sum())})"


# ------------------------------------------------------------------------------------------------ e. trainers
def _smac_runner(gpu):
    """tests/test_gpu_obs_embed_det._smac_runner on 3m (obs_dim 30) as MAT-Dec with a shared actor."""
    from mat_dcml_amd.config import _SMAC_FLAGS, get_config, parse_args
    from mat_dcml_amd.runner.smac_runner import SMACRunner
    argv = ["--env_name", "StarCraft2", "--algorithm_name", "mat_dec", "--map_name", "3m", "--n_rollout_threads", "8",
            "--episode_length", "6", "--use_value_active_masks", "--seed", "2", "--ppo_epoch", "2", "--num_mini_batch",
            "2"]
    args = parse_args(argv, get_config(), extra=_SMAC_FLAGS, warn=False)
    args.dec_actor, args.share_actor = True, True
    assert args.cuda_deterministic is True
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = SMACRunner({"all_args": args, "device": gpu, "run_dir": None})
    mat_fused.set_sampling_key(r.policy.transformer, 2, env0=0)
    return r, [str(x.message) for x in w if "cuda_deterministic" in str(x.message)]


def _mpe_runner(gpu):
    from mat_dcml_amd.runner.mpe_runner import MPERunner
    from test_mpe import _runner_args
    torch.manual_seed(1)
    a = _runner_args("simple_spread", n_rollout_threads=16, episode_length=10, ppo_epoch=2, algorithm_name="mat_dec")
    a.dec_actor, a.share_actor = True, True
    assert a.cuda_deterministic is True
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = MPERunner({"all_args": a, "device": gpu, "run_dir": None})
    return r, [str(x.message) for x in w if "cuda_deterministic" in str(x.message)]


def _train_twice(make):
    from mat_dcml_amd.ops.paths import kernel_report
    r, warned = make()
    tr, m = r.trainer, r.policy.transformer
    assert m.decoder.dec_actor and m.decoder.share_actor and m.encoder.obs_dim > mat_train.MAX_FUSED_OBS
    assert r.policy._fused(), mat_fused.unsupported_reasons(m)
    assert tr.fused, tr.fused_reason
    assert tr.deterministic is True and tr.nondeterministic_writer is None and tr.obs_embed_grad == "partials"
    assert not warned, warned
    rep = kernel_report(r)
    assert rep["train"] == "hip:mat_enc_fwd/bwd+mat_actor_fwd/bwd+ppo_loss+adam+obs_embed_fwd/bwd[grad=partials]", rep
    assert rep["decode"] == "hip:mat_actor_fwd+obs_embed_fwd", rep
    before = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).clone()
    r.warmup()
    for _ in range(2):
        r.rollout()
        r.compute()
        r.train()
    torch.cuda.synchronize()
    opt = r.policy.optimizer
    snap = {"params": torch.cat([p.detach().reshape(-1) for p in m.parameters()]).clone(), "exp_avg": opt.m.clone(),
            "exp_avg_sq": opt.v.clone(), "scratch": opt.scratch[:4].clone()}
    assert all(bool(torch.isfinite(v).all()) for v in snap.values())
    assert not torch.equal(before, snap["params"])
    actor = [p for n, p in m.named_parameters() if n.startswith("decoder.mlp")]
    assert len(actor) == 12   # three LayerNorms and three Linears
    assert all(float(opt.m[off:off + p.numel()].abs().max()) > 0 for p, off in ppo_fused.param_offsets(m)
               if any(p is q for q in actor)), "an actor parameter never received a gradient"
    enc, act, _ = m._mdl_train_state
    assert isinstance(act, mat_train.ActorFused) and act.emb.Mp is enc.emb.Mp and act.emb.Mp is not None
    return snap


@pytest.mark.parametrize("env", ["smac_3m", "mpe"])
def test_trainer_is_fused_deterministic_and_bitwise_repeatable(gpu, env):
    """--dec_actor --share_actor runners on SMAC 3m (obs 30) and MPE simple_spread (obs 18): a fused trainer that claims
    determinism without a cuda_deterministic warning and reports the actor and obs-embedding kernels; two same-seed
    constructions agree bit for bit after two PPO iterations on parameters, both Adam moments and the optimizer scratch."""
    make = (lambda: _smac_runner(gpu)) if env == "smac_3m" else (lambda: _mpe_runner(gpu))
    a, b = _train_twice(make), _train_twice(make)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k} differs by {(a[k] - b[k]).abs().max().item():.3e}"


def test_atomic_opt_out_reports_and_warns(gpu, monkeypatch):
    monkeypatch.setenv("MAT_DCML_OBS_EMBED_GRAD", "atomic")
    r, warned = _smac_runner(gpu)
    tr = r.trainer
    assert tr.fused and tr.deterministic is False and tr.obs_embed_grad == "atomic"
    assert len(warned) == 1 and "obs_embed" in warned[0] and "atomic" in warned[0], warned
    assert r.policy.transformer._mdl_train_state[1].obs_embed().grad_mode == "atomic"


def test_trainer_with_the_first_switch_alone_stays_hybrid(gpu, monkeypatch):
    monkeypatch.delenv(WIDE)
    r, warned = _smac_runner(gpu)
    assert r.trainer.fused is False and WIDE in r.trainer.fused_reason and not r.policy._fused() and not warned


# ------------------------------------------------------------------------------------------------ f. rollout vs learner
@pytest.mark.parametrize("key", ["od65_A36", "smac"])
def test_rollout_logprobs_match_the_learner(gpu, key, monkeypatch):
    """get_actions (logits from the WIDE logits-only kernel on the obs-embedding pre-activation, heads on keyed draws)
    against the learner's forward on the same actions: mean |d log p| between them is at most the learner's own mean
    distance from the fp32 eager model.  Sampled actions respect the mask."""
    L, B, od, A, kind, nb, av = _shape(gpu, key)
    m = make_actor(L, od, A, kind, nb, gpu)
    obs, _, ava, _, _, _ = make_inputs(gpu, L, B, od, A, kind, av, seed=21)
    assert mat_fused.supports(m)
    mat_fused.set_sampling_key(m, 5)
    lib, calls = mat_train.lib(), []
    real = lib.mdl_mat_actor_fwd_ct_wide

    def spy(p, pre, save, st):
        calls.append((bool(p._obj.logits), bool(pre), save))
        return real(p, pre, save, st)

    monkeypatch.setattr(lib, "mdl_mat_actor_fwd_ct_wide", spy)
    v, a, lp_roll = mat_fused.get_actions(m, obs, ava)
    assert calls == [(True, True, 0)], calls
    assert a.shape == (B, L, 1) and lp_roll.shape == (B, L, 1) and v.shape == (B, L, 1)
    pick = a[..., 0].long()
    assert bool((ava.gather(-1, pick.unsqueeze(-1)) == 1).all()) and pick.unique().numel() > 1
    with torch.no_grad():
        lp_eager, _, _ = m(None, obs, a, ava)
        enc = mat_train.EncoderFused(m)
        act = mat_train.ActorFused(m, enc)
        _, rep = enc.forward(obs, save=False)
        lp_learn, _ = act.forward(rep, a, ava, save=False)
    torch.cuda.synchronize()
    assert calls[1:] == [(False, True, 0)], calls
    d_roll, yard = (lp_roll - lp_learn).abs().mean().item(), (lp_learn - lp_eager).abs().mean().item()
    print(f"[dec-actor-wide] {key}: mean |d logp| rollout vs learner {d_roll:.3e}; learner vs eager fp32 {yard:.3e}")
    assert bool(torch.isfinite(lp_roll).all()) and yard > 0
    assert d_roll <= yard, (d_roll, yard)


# ------------------------------------------------------------------------------------------------ g. cost guard
def test_fused_wide_actor_is_not_slower_than_the_hybrid_paths_eager_actor(gpu, monkeypatch):
    """Actor forward + backward at 320 x 27 (od 1288, A 36, Discrete: SMAC 27m_vs_30m): the fused path — obs-embedding
    forward, WIDE forward, WIDE backward, obs-embedding backward, private workspace, bf16 observations as the trainer
    hands them over — against the hybrid path's eager bf16-autocast actor with autograd, measured in one process."""
    from mat_dcml_amd.models import act as act_mod
    L, B, od, A = 27, 320, 1288, 36
    c = WCase(gpu, L, B, od, A, "Discrete", 2, "random", refs=False)
    m = c.m
    v, rep = c.enc.forward(c.obs, save=False)
    obs16 = c.obs.to(torch.bfloat16)

    def fused():
        c.act.forward(rep, c.actions, c.ava, obs=obs16)
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
    monkeypatch.setenv(WIDE, "hybrid")
    assert not mat_train.decoder_supported(m)
    t_hybrid = measure(hybrid)
    perf_record("dec_actor_wide_fwd_bwd_hybrid_27x320_us", t_hybrid, None)
    perf_record("dec_actor_wide_fwd_bwd_fused_27x320_us", t_fused, round(t_hybrid, 1))
    print(f"[dec-actor-wide] actor forward + backward: hybrid {t_hybrid:.1f} us, fused {t_fused:.1f} us, "
          f"ratio {t_fused / t_hybrid:.3f}")
    assert t_fused <= t_hybrid, (t_fused, t_hybrid)
