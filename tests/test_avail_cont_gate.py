"""The fused-training gate of the Available_Continuous action type (ops/mat_train.decoder_unsupported_reasons): hybrid
by default, the fused decoder kernels with MAT_DCML_AVAIL_CONT_TRAIN=fused and 3 <= action_dim <= 16.  CPU only: the
gates are device independent (ops/paths.gate_reasons)."""
import os

import pytest

from mat_dcml_amd.ops import kernels

ENV = "MAT_DCML_AVAIL_CONT_TRAIN"


def _need_lib():
    if not os.path.exists(kernels.LIB_PATH):
        pytest.skip("HIP library not built")


def _mat(act_dim, action_type="Available_Continuous"):
    from mat_dcml_amd.models.mat import MultiAgentTransformer
    return MultiAgentTransformer(7, 7, act_dim, 9, 2, 64, 2, action_type=action_type)


@pytest.mark.parametrize("action_type", ["Available_Continuous", "Available_Continous"])
def test_fused_switch_opens_the_train_gate(monkeypatch, action_type):
    _need_lib()
    from mat_dcml_amd.ops import mat_train
    from mat_dcml_amd.ops.paths import gate_reasons
    monkeypatch.setenv(ENV, "fused")
    m = _mat(4, action_type)
    g = gate_reasons(m)
    assert g == {"encoder": [], "decode": [], "train": []}, g
    assert mat_train.decoder_supported(m) and mat_train.supported(m)


def test_default_stays_hybrid_and_names_the_switch(monkeypatch):
    _need_lib()
    from mat_dcml_amd.ops import mat_train
    from mat_dcml_amd.ops.paths import gate_reasons
    m = _mat(4)
    for value in (None, "hybrid"):
        if value is None:
            monkeypatch.delenv(ENV, raising=False)
        else:
            monkeypatch.setenv(ENV, value)
        g = gate_reasons(m)
        assert g["encoder"] == [] and g["decode"] == [], g
        assert len(g["train"]) == 1, g
        assert "Available_Continuous" in g["train"][0] and ENV + "=fused" in g["train"][0], g
        assert not mat_train.decoder_supported(m)


def test_switch_is_read_at_call_time(monkeypatch):
    _need_lib()
    from mat_dcml_amd.ops import mat_train
    m = _mat(4)
    monkeypatch.delenv(ENV, raising=False)
    assert mat_train.decoder_unsupported_reasons(m)
    monkeypatch.setenv(ENV, "fused")
    assert mat_train.decoder_unsupported_reasons(m) == []
    monkeypatch.delenv(ENV)
    assert mat_train.decoder_unsupported_reasons(m)


@pytest.mark.parametrize("act_dim", [2, 17])
def test_action_dim_outside_the_kernel_names_the_limit(monkeypatch, act_dim):
    _need_lib()
    from mat_dcml_amd.ops.paths import gate_reasons
    monkeypatch.setenv(ENV, "fused")
    why = gate_reasons(_mat(act_dim))["train"]
    assert any("Available_Continuous" in r and f"action_dim {act_dim}" in r and "3 <= action_dim <= 16" in r
               for r in why), why


@pytest.mark.parametrize("act_dim", [3, 16])
def test_action_dim_limits_are_inclusive(monkeypatch, act_dim):
    _need_lib()
    from mat_dcml_amd.ops.paths import gate_reasons
    monkeypatch.setenv(ENV, "fused")
    assert gate_reasons(_mat(act_dim))["train"] == []


def test_bogus_value_raises(monkeypatch):
    _need_lib()
    from mat_dcml_amd.ops import mat_train
    monkeypatch.setenv(ENV, "yes")
    with pytest.raises(ValueError, match=ENV):
        mat_train.decoder_unsupported_reasons(_mat(4))


def test_other_action_types_ignore_the_switch(monkeypatch):
    """The variable is read only for Available_Continuous models: a bogus value does not disturb the others."""
    _need_lib()
    from mat_dcml_amd.ops import mat_train
    monkeypatch.setenv(ENV, "yes")
    assert mat_train.decoder_unsupported_reasons(_mat(3, "Continuous")) == []
