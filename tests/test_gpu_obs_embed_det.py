"""Bit-reproducible training with wide observations (obs_dim > 16: SMAC 27m_vs_30m's 1,288 features, MPE's 18).

The wide-observation embedding backward (``csrc/obs_embed.hip``) sums over tokens on many workgroups.  In its default
``"partials"`` mode every workgroup stores its partial (64 token ranges per 64-column block of ``M``, 256 workgroups of
``u`` / ``db``) and one kernel adds the partials in index order; ``MAT_DCML_OBS_EMBED_GRAD=atomic`` keeps the earlier
fp32 atomics for A/B runs.

* kernel parity at the edges of the tiling (empty token ranges, one token per range, a 32-token tile plus one, rows
  not aligned to 4 / 8, exactly one column block, a second block of one column, SMAC's 8-column last block), fp32 and
  bf16 observations, against fp64 autograd, with the atomic mode as the yardstick;
* bitwise repeats with other work interleaved and the partial workspaces poisoned (every slot the reduction reads is
  written by the same call);
* SMAC and MPE trainers: ``deterministic`` is reported, no warning, and two same-seed runs of two PPO iterations are
  ``torch.equal`` on parameters, Adam moments and the optimizer scratch;
* the opt-out reports and warns;
* the deterministic backward costs no more than GUARD_MARGIN x the atomic one at SMAC's training minibatch.
"""
import os
import warnings

import pytest
import torch

from mat_dcml_amd.ops import mat_train

from conftest import GUARD_MARGIN, median_us, perf_record
from test_gpu_train import make_discrete

pytestmark = pytest.mark.gpu

NAMES = ("d_we", "d_be", "d_g", "d_b")
_models = {}


def _embed(od, gpu):
    """One model / ObsEmbed per observation width, shared by the tests (never modified: the gradients are reset)."""
    if od not in _models:
        m = make_discrete(3, 5, od, gpu, seed=4)
        _models[od] = (m, mat_train.ObsEmbed(m))
    return _models[od]


def _params(oe):
    return oe.lin.weight, oe.lin.bias, oe.ln.weight, oe.ln.bias


def _inputs(N, od, dtype, gpu, seed=6):
    g = torch.Generator(device=gpu).manual_seed(seed)
    obs = torch.rand(N, od, device=gpu, generator=g) * (torch.rand(N, od, device=gpu, generator=g) < 0.3)
    obs = obs.to(dtype).contiguous()
    dpre = torch.randn(N, 64, device=gpu, generator=g)
    return obs, dpre


def _backward(oe, obs, stat, dpre, mode, fill):
    """The four parameter gradients of one backward call in ``mode``, on top of ``.grad`` pre-filled with ``fill``."""
    oe.grad_mode = mode
    for p in _params(oe):
        p.grad = torch.full_like(p, fill)
    oe.backward(obs, stat, dpre)
    torch.cuda.synchronize()
    return [p.grad.detach().clone() - fill for p in _params(oe)]


def _reference(oe, obs, dpre):
    """fp64 autograd through LayerNorm -> Linear on the observations as the kernel sees them."""
    w, b, g, bb = (p.detach().double().requires_grad_(True) for p in _params(oe))
    x = obs.double()
    pre = torch.nn.functional.linear(torch.nn.functional.layer_norm(x, (x.shape[1],), g, bb, 1e-5), w, b)
    pre.backward(dpre.double())
    return [w.grad, b.grad, g.grad, bb.grad]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N,od", [(1, 18), (63, 65), (64, 64), (2049, 40), (2112, 1288)])
def test_backward_partials_match_fp64_and_atomic(gpu, N, od, dtype):
    m, oe = _embed(od, gpu)
    obs, dpre = _inputs(N, od, dtype, gpu)   # bf16: rounded here, the reference reads the rounded values
    _, stat = oe.forward(obs)
    try:
        got = {mode: _backward(oe, obs, stat, dpre, mode, 1.0) for mode in ("atomic", "partials")}   # adds into .grad
    finally:
        oe.grad_mode = "partials"
    ref = _reference(oe, obs, dpre)
    # near-zero gradients are measured against a floor of the global norm (tests/test_gpu_determinism.py)
    floor = 1e-3 * torch.stack([r.norm() for r in ref]).norm()
    for i, n in enumerate(NAMES):
        r = ref[i]
        err = {mode: ((got[mode][i].double() - r).norm() / (r.norm() + floor)).item() for mode in got}
        a = got["atomic"][i].double()
        d = ((got["partials"][i].double() - a).norm() / (a.norm() + floor)).item()
        print(f"N {N} od {od} {n}: vs fp64 partials {err['partials']:.3e} atomic {err['atomic']:.3e}; "
              f"partials vs atomic {d:.3e}")
        assert err["partials"] <= err["atomic"] + 1e-5, (n, err)
        assert d < 1e-5, (n, d)   # a pure fp32 summation-order difference


@pytest.mark.parametrize("N,od", [(2112, 1288), (63, 18)])
def test_backward_bitwise_repeatable_and_rewrites_every_partial(gpu, N, od):
    m, oe = _embed(od, gpu)
    obs, dpre = _inputs(N, od, torch.bfloat16 if od > 100 else torch.float32, gpu, seed=7)
    _, stat = oe.forward(obs)
    assert oe.grad_mode == "partials"
    runs = []
    for i in range(3):
        if i == 2:   # stale partials (and stale sums) must not reach the result
            assert oe.Mp.numel() == 64 * 64 * 64 * ((od + 63) // 64) and oe.up.numel() == 256 * 128
            for t in (oe.Mp, oe.up, oe.M, oe.ud):
                t.fill_(float("nan"))
        runs.append(_backward(oe, obs, stat, dpre, "partials", 0.0))
        junk = torch.randn(4096, 4096, device=gpu) @ torch.randn(4096, 4096, device=gpu)   # perturb timing / caches
    torch.cuda.synchronize()
    del junk
    for r in runs:
        assert all(bool(torch.isfinite(t).all()) for t in r)
    for r in runs[1:]:
        for n, a, b in zip(NAMES, runs[0], r):
            assert torch.equal(a, b), (n, (a - b).abs().max().item())


def test_partial_workspaces_are_allocated_by_the_first_backward(gpu):
    m = make_discrete(3, 5, 40, gpu, seed=4)
    oe = mat_train.ObsEmbed(m)
    obs, dpre = _inputs(70, 40, torch.float32, gpu)
    _, stat = oe.forward(obs)
    assert oe.grad_mode == "partials" and oe.Mp is None and oe.up is None   # rollout / eval never allocate them
    _backward(oe, obs, stat, dpre, "partials", 0.0)
    assert oe.Mp is not None and oe.up is not None


# ------------------------------------------------------------------------------------------------ trainers
def _snapshot(r):
    opt = r.policy.optimizer
    return {"params": torch.cat([p.detach().reshape(-1) for p in r.policy.transformer.parameters()]).clone(),
            "exp_avg": opt.m.clone(), "exp_avg_sq": opt.v.clone(), "scratch": opt.scratch[:4].clone()}


ROLLOUT = ("obs", "available_actions", "actions", "action_log_probs", "value_preds", "rewards", "masks")


def _rollout_snapshot(r):
    return {k: getattr(r.buffer, k).clone() for k in ROLLOUT}


def _smac_runner(gpu, num_mini_batch, envs=8, T=6):
    """tests/test_gpu_smac_env._smac_runner with 2 PPO epochs; cuda_deterministic as in the reference argv (the flag is
    store_false and the reference scripts do not pass it: on)."""
    from mat_dcml_amd.config import _SMAC_FLAGS, get_config, parse_args
    from mat_dcml_amd.ops import mat_fused
    from mat_dcml_amd.runner.smac_runner import SMACRunner
    argv = ["--env_name", "StarCraft2", "--algorithm_name", "mat", "--map_name", "27m_vs_30m", "--n_rollout_threads",
            str(envs), "--episode_length", str(T), "--use_value_active_masks", "--seed", "2", "--ppo_epoch", "2",
            "--num_mini_batch", str(num_mini_batch)]
    args = parse_args(argv, get_config(), extra=_SMAC_FLAGS, warn=False)
    assert args.cuda_deterministic is True
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = SMACRunner({"all_args": args, "device": gpu, "run_dir": None})
    mat_fused.set_sampling_key(r.policy.transformer, 2, env0=0)
    return r, [str(x.message) for x in w if "not bit-reproducible" in str(x.message)]


def _mpe_runner(gpu):
    from mat_dcml_amd.runner.mpe_runner import MPERunner
    from test_mpe import _runner_args
    torch.manual_seed(1)
    a = _runner_args("simple_spread", n_rollout_threads=16, episode_length=10, ppo_epoch=2)
    assert a.cuda_deterministic is True
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = MPERunner({"all_args": a, "device": gpu, "run_dir": None})
    return r, [str(x.message) for x in w if "not bit-reproducible" in str(x.message)]


def _train_twice(make):
    """Two PPO iterations of a fresh runner: [rollout 1, update 1, rollout 2, update 2] snapshots."""
    r, warned = make()
    tr = r.trainer
    assert tr.fused, tr.fused_reason
    assert r.policy.transformer.encoder.obs_dim > mat_train.MAX_FUSED_OBS
    assert tr.deterministic, tr.nondeterministic_writer
    assert not warned, warned
    r.warmup()
    snaps = []
    for _ in range(2):
        r.rollout()
        snaps.append(_rollout_snapshot(r))
        r.compute()
        r.train()
        snaps.append(_snapshot(r))
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in snaps[-1].values())
    return snaps


def _assert_same_runs(a, b, rollout_note):
    for i, (sa, sb) in enumerate(zip(a, b)):
        what = f"rollout {i // 2 + 1}" if i % 2 == 0 else f"update {i // 2 + 1}"
        for k in sa:
            note = f" ({rollout_note})" if i % 2 == 0 else ""
            assert torch.equal(sa[k], sb[k]), f"{what}: {k} differs by {(sa[k] - sb[k]).abs().max().item():.3e}{note}"


@pytest.mark.parametrize("num_mini_batch", [1, 2])
def test_smac_trainer_bitwise_repeatable(gpu, num_mini_batch):
    """num_mini_batch 1: the whole buffer in place (bf16 observations); 2: gathered minibatches."""
    a = _train_twice(lambda: _smac_runner(gpu, num_mini_batch))
    b = _train_twice(lambda: _smac_runner(gpu, num_mini_batch))
    _assert_same_runs(a, b, "the rollout of the same parameters differs: the SMAC env / decode, not the update")


def test_mpe_trainer_bitwise_repeatable(gpu):
    a, b = _train_twice(lambda: _mpe_runner(gpu)), _train_twice(lambda: _mpe_runner(gpu))
    _assert_same_runs(a, b, "the two runs' rollout buffers differ although the parameters were equal: the failure "
                            "lies in the torch MPE env / sampling, not in the embedding backward")


def test_atomic_opt_out_reports_and_warns(gpu):
    old = os.environ.get("MAT_DCML_OBS_EMBED_GRAD")
    os.environ["MAT_DCML_OBS_EMBED_GRAD"] = "atomic"
    try:
        r, warned = _smac_runner(gpu, 1)
    finally:
        if old is None:
            os.environ.pop("MAT_DCML_OBS_EMBED_GRAD", None)
        else:
            os.environ["MAT_DCML_OBS_EMBED_GRAD"] = old
    tr = r.trainer
    assert tr.fused and tr.deterministic is False and tr.obs_embed_grad == "atomic"
    assert len(warned) == 1 and "obs_embed" in warned[0] and "atomic" in warned[0], warned


def test_partials_backward_cost_guard(gpu):
    """SMAC's training minibatch (86,400 tokens x 1,288 bf16 features): the deterministic backward against the atomic
    one in the same process.  Extra traffic: the 22 MB of partials written and read once, against 222 MB of
    observations read."""
    N, od = 86400, 1288
    m, oe = _embed(od, gpu)
    obs, dpre = _inputs(N, od, torch.bfloat16, gpu)
    _, stat = oe.forward(obs)
    for p in _params(oe):
        p.grad = torch.zeros_like(p)
    us = {}
    try:
        for mode in ("atomic", "partials"):
            oe.grad_mode = mode
            us[mode] = median_us(lambda: oe.backward(obs, stat, dpre))
    finally:
        oe.grad_mode = "partials"
    perf_record("obs_embed_bwd_atomic_smac_mb", us["atomic"], None)
    perf_record("obs_embed_bwd_partials_smac_mb", us["partials"], round(GUARD_MARGIN * us["atomic"], 3))
    assert us["partials"] <= GUARD_MARGIN * us["atomic"], us
