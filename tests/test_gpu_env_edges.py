"""DCML env kernels (csrc/dcml_env.hip) vs the torch path at the edges of their tiling: one to four waves with a
single-lane or full last wave, periods that are no multiple of the noise loop's 4 draws or shorter than the three
observed slots, a binding slot cap, every mode combination, the preset clamps, env ids past 2^31, one env and more
envs than one launch wave of workgroups, env-range views, poisoned buffers and bitwise repeatability.

Every parity case goes through ``dcml_env_helper.run_parity(extended=True)``: the assertions of
``test_env_kernel_matches_torch`` plus ``share`` after every step and the carried state compared directly (integers
and the fp32 bid profile bit-equal, doubles at 1e-12).  The figures quoted per case (exempt env-steps, branch counts,
slot-cap hits) are those of the reference alone on the CPU; profiles/env_edges/README.md lists them."""
import numpy as np
import pytest
import torch

from dcml_env_helper import BRANCHES, make_actions, make_pair, run_parity
from mat_dcml_amd.envs.dcml.config import DCMLConfig
from mat_dcml_amd.envs.dcml.data import load_preset
from mat_dcml_amd.envs.dcml.vec_env import DeviceDCMLEnv

pytestmark = pytest.mark.gpu

ALL = frozenset(BRANCHES)


# ---------------------------------------------------------------------------------------------- preset set-ups
def _tables(env, rows):
    m, prs, dis = load_preset(env.cfg)
    return m[:rows].copy(), prs[:rows].copy(), dis[:rows].copy()


def setup_three_rows(env):
    """3-row table, first rows 0 / 1 / 2 across the envs: after two steps every env has run past the last row."""
    m, prs, dis = _tables(env, 3)
    env.set_preset_tables(m, prs, dis, np.arange(env.E) % 3)


def setup_disable_edges(env):
    """Disable counts below 0, 0, W - 1 and above W - 1, cycled over 12 rows so that each stays in play on every step:
    both clamps of ``dis`` and both ends of ``denom = W - dis``."""
    m, prs, dis = _tables(env, 12)
    dis[:] = np.tile(np.array([-3, 0, env.W - 1, env.W + 5]), 3)
    env.set_preset_tables(m, prs, dis, np.arange(env.E) % 4)


def setup_pr_zero(env):
    env.modify_preset(Pr=0.0)


def setup_ties(env):
    """Every worker the same loss probability, every task the same (largest) size: the workers' delays differ only
    through their retry draws and bid profiles, and tie exactly in 59 of the reference's 512 env-steps."""
    env.modify_preset(R=2 ** 20, C=2 ** 10, Pr=0.3)


# ---------------------------------------------------------------------------------------------- parity cases
# id -> (make_pair keywords, steps, branches the reference reaches and the case requires, slot cap reached)
CASES = {}


def _case(name, require=ALL, cap=False, steps=8, **kw):
    CASES[name] = (kw, steps, frozenset(require), cap)


for _W in (1, 2, 63, 64, 65, 129, 192, 193, 255, 256):     # 1-4 waves; last wave with one lane, 63 lanes, full
    _case(f"W{_W}", W=_W)
for _P in (1, 2, 3, 5, 7):                                 # (P + 3) / 4 noise draws, (arrive + k) % P with P < 3
    _case(f"W32-P{_P}", W=32, period=_P, **({"max_slot_iters": 48} if _P == 1 else {}), cap=_P == 1)
_case("W32-cap1", W=32, max_slot_iters=1, cap=True)
_case("W32-cap3", W=32, max_slot_iters=3, cap=True)
_case("W65-shannon-fixed", W=65, shannon=True, fixed=True, require=())
_case("W65-shannon-preset", W=65, shannon=True, preset=True)
_case("W65-preset-fixed", W=65, preset=True, fixed=True, require=())
_case("W32-preset-3rows", W=32, preset=True, setup=setup_three_rows, steps=5)
_case("W32-preset-disable", W=32, preset=True, setup=setup_disable_edges)
_case("W32-preset-pr0", W=32, preset=True, setup=setup_pr_zero)
_case("W32-preset-ties", W=32, preset=True, setup=setup_ties)
_case("W100-offset-2^31+5", W=100, env_id_offset=2 ** 31 + 5)
_case("W100-seed12345", W=100, seed=12345)
_case("W4-E1", W=4, E=1, require=())                       # one env: the recipe's forced ranges are empty
_case("W4-E4099", W=4, E=4099, steps=2)


@pytest.mark.parametrize("name", list(CASES))
def test_env_kernel_edge_matches_torch(gpu, name):
    kw, steps, require, cap = CASES[name]
    hip, ref = make_pair(gpu, **kw)
    assert hip._kern is not None and ref._kern is None
    st = run_parity(hip, ref, steps=steps, extended=True)
    print(f"[env-edge] {name}: {st}")
    for b in require:
        assert st["branch"][b] > 0, (b, st)
    if cap:   # the slot loop ran to max_slot_iters on both paths
        assert st["cap_hits"] > 0 and st["cap_hits_test"] > 0, st
    if name == "W32-preset-ties":
        assert st["tie_env_steps"] > 0, st
    if name == "W32-preset-3rows":   # 1 + 5 tasks started from rows 0..2 of 3: every env ran past the last row
        assert int(ref.preset_idx.min()) >= 6 and torch.equal(hip.preset_idx, ref.preset_idx)
        last = torch.as_tensor(load_preset(ref.cfg)[0][2], device=gpu)
        assert torch.equal(ref.R, last[0].expand(ref.E)) and torch.equal(hip.R, ref.R)
    if name == "W32-preset-disable":
        seen = set(ref.n_disable.tolist())
        assert seen <= {0, ref.W - 1} and torch.equal(hip.n_disable, ref.n_disable)


def test_preset_disable_clamps_reach_both_ends(gpu):
    """The four disable values of ``setup_disable_edges`` land on 0, 0, W - 1 and W - 1 after the reset alone, with all
    or exactly one worker available."""
    hip, ref = make_pair(gpu, W=32, preset=True, setup=setup_disable_edges)
    hip.reset(), ref.reset()
    want = torch.tensor([0, 0, 31, 31], device=gpu).repeat(16)
    for env in (hip, ref):
        assert torch.equal(env.n_disable, want)
        assert torch.equal(env.avail.sum(1), 32 - want)
    assert torch.allclose(hip.obs, ref.obs, atol=1e-6)


# ---------------------------------------------------------------------------------------------- views, poison, repeat
def _snapshot(env, outs):
    d = {k: getattr(env, k).clone() for k in DeviceDCMLEnv._PER_ENV}
    for i, o in enumerate(outs):
        d[f"out{i}"] = o.clone()
    return d


def _assert_same(a, b, where):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (where, k)


def test_group_views_match_whole_env(gpu):
    """An E = 64 HIP env stepped as four env-range views equals a second HIP env stepped whole: outputs and every
    per-env tensor bit-equal."""
    E, W = 64, 65
    whole, parent = make_pair(gpu, W=W, E=E, backends=("hip", "hip"))
    o_w, o_p = whole.reset(), parent.reset()
    _assert_same(_snapshot(whole, o_w), _snapshot(parent, o_p), "reset")
    views = parent.group_views(4)
    n = E // 4
    g = torch.Generator(device=gpu).manual_seed(3)
    for step in range(4):
        act = make_actions(g, E, W, gpu)
        ow = [o.clone() for o in whole.step(act)]
        ov = [[o.clone() for o in v.step(act[i * n:(i + 1) * n])] for i, v in enumerate(views)]
        for j in range(len(ow)):
            assert torch.equal(ow[j], torch.cat([o[j] for o in ov], 0)), (step, j)
        for k in DeviceDCMLEnv._PER_ENV:
            assert torch.equal(getattr(whole, k), getattr(parent, k)), (step, k)


@pytest.mark.parametrize("W,shannon", [(65, False), (65, True), (256, False), (256, True)])
def test_poisoned_buffers_are_overwritten(gpu, W, shannon):
    """NaN in every buffer a reset must define (obs, share, ava, lw, worker_pr, rate, up_rate) before ``reset()`` and in
    the step outputs before a ``step()``: nothing of it survives, and everything equals an unpoisoned twin."""
    E = 16
    clean, dirty = make_pair(gpu, W=W, E=E, shannon=shannon, backends=("hip", "hip"))
    for k in ("obs", "share", "ava", "lw", "worker_pr", "rate", "up_rate"):
        getattr(dirty, k).fill_(float("nan"))
    oc, od = clean.reset(), dirty.reset()
    sc, sd = _snapshot(clean, oc), _snapshot(dirty, od)
    _assert_same(sc, sd, "reset")
    g = torch.Generator(device=gpu).manual_seed(5)
    for step in range(2):
        act = make_actions(g, E, W, gpu)
        if step == 1:
            rew, done, delay, pay = dirty._out
            rew.fill_(float("nan")), delay.fill_(float("nan")), pay.fill_(float("nan")), done.fill_(True)
        sc, sd = _snapshot(clean, clean.step(act)), _snapshot(dirty, dirty.step(act))
        _assert_same(sc, sd, f"step {step}")
    for k, t in sd.items():
        if t.is_floating_point():
            assert torch.isfinite(t).all(), k


def test_bitwise_repeat_with_interleaved_work(gpu):
    """Two same-seed HIP envs, a large matmul between the steps of one of them: every output and state tensor equal."""
    E, W = 64, 129
    a, b = make_pair(gpu, W=W, E=E, shannon=True, backends=("hip", "hip"))
    _assert_same(_snapshot(a, a.reset()), _snapshot(b, b.reset()), "reset")
    big = torch.randn(4096, 4096, device=gpu)
    g = torch.Generator(device=gpu).manual_seed(9)
    for step in range(8):
        act = make_actions(g, E, W, gpu)
        sa = _snapshot(a, a.step(act))
        (big @ big).sum()
        sb = _snapshot(b, b.step(act))
        _assert_same(sa, sb, f"step {step}")


# ---------------------------------------------------------------------------------------------- the kernel's refusal
def test_auto_takes_torch_path_beyond_kernel_limit(gpu):
    env = DeviceDCMLEnv(2, DCMLConfig(n_workers=257), device=gpu, backend="auto")
    assert env._kern is None
    ok = DeviceDCMLEnv(2, DCMLConfig(n_workers=256), device=gpu, backend="auto")
    assert ok._kern is not None


def test_hip_backend_raises_beyond_kernel_limit(gpu):
    with pytest.raises(RuntimeError, match="256 workers"):
        DeviceDCMLEnv(2, DCMLConfig(n_workers=257), device=gpu, backend="hip")
