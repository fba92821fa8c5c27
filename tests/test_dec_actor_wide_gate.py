"""The second opt-in of MAT-Dec's fused gate: MAT_DCML_DEC_ACTOR_WIDE_OBS=fused, next to MAT_DCML_DEC_ACTOR_TRAIN=fused,
opens the shared actor to observations wider than the in-kernel embedding (obs_dim > 16: csrc/obs_embed.hip computes the
actor's pre-activation, the WIDE kernels of csrc/mat_actor_ct.hip the rest).  Alone, the first switch refuses them as
before and names the second.  CPU only: the gates are device independent."""
import pytest

from test_dec_actor_gate import ENV, _mat, _need_lib

WIDE = "MAT_DCML_DEC_ACTOR_WIDE_OBS"
HEADS = [("Semi_Discrete", 2), ("Discrete", 36), ("Continuous", 17)]


def _both(monkeypatch):
    monkeypatch.setenv(ENV, "fused")
    monkeypatch.setenv(WIDE, "fused")


@pytest.mark.parametrize("obs_dim", [17, 30, 1288])
@pytest.mark.parametrize("action_type,act_dim", HEADS)
def test_both_switches_open_wide_observations(monkeypatch, obs_dim, action_type, act_dim):
    _need_lib()
    from mat_dcml_amd.ops import mat_fused, mat_train
    from mat_dcml_amd.ops.paths import gate_reasons
    _both(monkeypatch)
    m = _mat(act_dim, action_type, obs_dim=obs_dim)
    assert gate_reasons(m) == {"encoder": [], "decode": [], "train": []}
    assert mat_train.supported(m) and mat_train.dec_actor_fused(m) and mat_fused.supports(m)


@pytest.mark.parametrize("value", [None, "hybrid"])
@pytest.mark.parametrize("obs_dim", [17, 1288])
def test_first_switch_alone_refuses_as_before_and_names_the_second(monkeypatch, obs_dim, value):
    _need_lib()
    from mat_dcml_amd.ops import mat_fused, mat_train
    from mat_dcml_amd.ops.paths import gate_reasons
    monkeypatch.setenv(ENV, "fused")
    if value is None:
        monkeypatch.delenv(WIDE, raising=False)
    else:
        monkeypatch.setenv(WIDE, value)
    m = _mat(obs_dim=obs_dim)
    g = gate_reasons(m)
    today = (f"dec_actor with obs_dim {obs_dim} > 16: the fused actor kernels embed at most 16 observation features")
    assert len(g["train"]) == 1 and g["train"][0].startswith(today) and WIDE + "=fused" in g["train"][0], g
    assert g["decode"] == ["dec_actor (mat_dec) has no autoregressive decode", g["train"][0]], g
    assert g["encoder"] == []
    assert not mat_train.supported(m) and not mat_train.dec_actor_fused(m) and not mat_fused.supports(m)


def test_second_switch_alone_changes_nothing(monkeypatch):
    """Without MAT_DCML_DEC_ACTOR_TRAIN=fused the second switch is not even read: the default reason, whatever it says."""
    _need_lib()
    from mat_dcml_amd.ops.paths import gate_reasons
    monkeypatch.delenv(ENV, raising=False)
    m = _mat(obs_dim=30)
    monkeypatch.delenv(WIDE, raising=False)
    default = gate_reasons(m)
    assert len(default["train"]) == 1 and ENV + "=fused" in default["train"][0] and WIDE not in default["train"][0]
    for value in ("fused", "yes"):
        monkeypatch.setenv(WIDE, value)
        assert gate_reasons(m) == default


def test_narrow_observations_read_as_before(monkeypatch):
    _need_lib()
    from mat_dcml_amd.ops.paths import gate_reasons
    for value in (None, "hybrid", "fused"):
        monkeypatch.setenv(ENV, "fused")
        if value is None:
            monkeypatch.delenv(WIDE, raising=False)
        else:
            monkeypatch.setenv(WIDE, value)
        assert gate_reasons(_mat(obs_dim=16)) == {"encoder": [], "decode": [], "train": []}


def test_switch_is_read_at_call_time(monkeypatch):
    _need_lib()
    from mat_dcml_amd.ops import mat_train
    m = _mat(obs_dim=30)
    monkeypatch.setenv(ENV, "fused")
    monkeypatch.delenv(WIDE, raising=False)
    assert mat_train.dec_actor_wide_obs_mode() == "hybrid" and mat_train.decoder_unsupported_reasons(m)
    monkeypatch.setenv(WIDE, "fused")
    assert mat_train.dec_actor_wide_obs_mode() == "fused" and mat_train.decoder_unsupported_reasons(m) == []
    monkeypatch.delenv(WIDE)
    assert mat_train.decoder_unsupported_reasons(m)


@pytest.mark.parametrize("obs_dim", [7, 30])
def test_bogus_value_raises(monkeypatch, obs_dim):
    _need_lib()
    from mat_dcml_amd.ops import mat_fused, mat_train
    monkeypatch.setenv(ENV, "fused")
    monkeypatch.setenv(WIDE, "yes")
    with pytest.raises(ValueError, match=WIDE):
        mat_train.dec_actor_wide_obs_mode()
    with pytest.raises(ValueError, match=WIDE):
        mat_train.decoder_unsupported_reasons(_mat(obs_dim=obs_dim))
    with pytest.raises(ValueError, match=WIDE):
        mat_fused.unsupported_reasons(_mat(obs_dim=obs_dim))


def test_per_agent_actors_stay_refused_with_exactly_their_reason(monkeypatch):
    _need_lib()
    from mat_dcml_amd.ops.paths import gate_reasons
    _both(monkeypatch)
    why = gate_reasons(_mat(share_actor=False, obs_dim=30))["train"]
    assert why == [f"dec_actor with per-agent actors (share_actor=False): {ENV}=fused takes the shared actor"], why
    monkeypatch.delenv(WIDE)   # and without the second switch: today's two reasons, in today's order
    why = gate_reasons(_mat(share_actor=False, obs_dim=17))["train"]
    assert len(why) == 2 and "share_actor=False" in why[0] and "obs_dim 17" in why[1] and "16" in why[1], why


def test_available_continuous_actors_stay_refused(monkeypatch):
    _need_lib()
    from mat_dcml_amd.ops.paths import gate_reasons
    _both(monkeypatch)
    why = gate_reasons(_mat(4, "Available_Continuous", obs_dim=30))["train"]
    assert why == ["dec_actor with action_type Available_Continuous: the fused actor kernels take Discrete, "
                   "Semi_Discrete and Continuous"], why


class _Policy:
    def __init__(self, m, device):
        import torch
        self.transformer, self.device, self.kernels = m, torch.device(device), "auto"

    def _is_mat(self):
        return True

    def _enc_fused(self):
        return True


class _Runner:
    def __init__(self, m, device, trainer=None):
        self.policy, self.trainer = _Policy(m, device), trainer


class _Trainer:
    fused, obs_embed_grad = True, "partials"


def test_kernel_report_names_the_obs_embedding_stage(monkeypatch):
    """A fused trainer over a wide-observation MAT-Dec model reports the hip: train and decode paths with the
    obs-embedding stage (the train string as the encoder's wide path already reads); narrow models read as before."""
    _need_lib()
    from mat_dcml_amd.ops.paths import kernel_report
    _both(monkeypatch)
    rep = kernel_report(_Runner(_mat(36, "Discrete", obs_dim=30), "cuda", _Trainer()))
    assert rep["train"] == "hip:mat_enc_fwd/bwd+mat_actor_fwd/bwd+ppo_loss+adam+obs_embed_fwd/bwd[grad=partials]", rep
    assert rep["decode"] == "hip:mat_actor_fwd+obs_embed_fwd", rep
    assert rep["encoder"] == "hip:mat_enc_fwd", rep
    narrow = kernel_report(_Runner(_mat(36, "Discrete", obs_dim=16), "cuda"))
    assert narrow["decode"] == "hip:mat_actor_fwd", narrow
    # the first switch alone: the torch decode and the hybrid reason, both naming the second switch
    monkeypatch.delenv(WIDE)
    rep = kernel_report(_Runner(_mat(36, "Discrete", obs_dim=30), "cuda"))
    assert rep["decode"].startswith("torch (") and WIDE + "=fused" in rep["decode"], rep
    assert "obs_embed" not in rep["decode"] and WIDE + "=fused" in rep["train"], rep
