"""The fused gate of MAT-Dec (``dec_actor``; ops/mat_train.decoder_unsupported_reasons, ops/mat_fused.unsupported_reasons):
hybrid by default, the fused actor kernels (csrc/mat_actor_ct.hip) with MAT_DCML_DEC_ACTOR_TRAIN=fused for a shared
actor on obs_dim <= 16 with a Discrete / Semi_Discrete (semi_index -1) / Continuous head of at most 64 actions; and the
layout of the kernels' argument struct against its ctypes mirror.  CPU only: the gates are device independent."""
import ctypes
import os
import subprocess

import pytest

from mat_dcml_amd.ops import kernels

ENV = "MAT_DCML_DEC_ACTOR_TRAIN"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _need_lib():
    if not os.path.exists(kernels.LIB_PATH):
        pytest.skip("HIP library not built")


def _mat(act_dim=2, action_type="Semi_Discrete", obs_dim=7, share_actor=True, semi_index=-1):
    from mat_dcml_amd.models.mat import MultiAgentTransformer
    return MultiAgentTransformer(obs_dim, obs_dim, act_dim, 9, 2, 64, 2, action_type=action_type, dec_actor=True,
                                 share_actor=share_actor, semi_index=semi_index)


def test_default_stays_hybrid_and_names_the_switch(monkeypatch):
    _need_lib()
    from mat_dcml_amd.ops import mat_train
    from mat_dcml_amd.ops.paths import gate_reasons
    m = _mat()
    for value in (None, "hybrid"):
        if value is None:
            monkeypatch.delenv(ENV, raising=False)
        else:
            monkeypatch.setenv(ENV, value)
        g = gate_reasons(m)
        assert g["encoder"] == [], g
        assert len(g["train"]) == 1 and "dec_actor" in g["train"][0] and ENV + "=fused" in g["train"][0], g
        assert any("dec_actor" in r for r in g["decode"]) and any(ENV + "=fused" in r for r in g["decode"]), g
        assert not mat_train.decoder_supported(m) and not mat_train.dec_actor_fused(m)


@pytest.mark.parametrize("action_type,act_dim", [("Semi_Discrete", 2), ("Discrete", 36), ("Discrete", 64),
                                                 ("Continuous", 17)])
def test_fused_switch_opens_every_gate(monkeypatch, action_type, act_dim):
    _need_lib()
    from mat_dcml_amd.ops import mat_fused, mat_train
    from mat_dcml_amd.ops.paths import gate_reasons
    monkeypatch.setenv(ENV, "fused")
    m = _mat(act_dim, action_type)
    assert gate_reasons(m) == {"encoder": [], "decode": [], "train": []}
    assert mat_train.supported(m) and mat_fused.supports(m) and mat_train.dec_actor_fused(m)


def test_switch_is_read_at_call_time(monkeypatch):
    _need_lib()
    from mat_dcml_amd.ops import mat_train
    m = _mat()
    monkeypatch.delenv(ENV, raising=False)
    assert mat_train.decoder_unsupported_reasons(m)
    monkeypatch.setenv(ENV, "fused")
    assert mat_train.decoder_unsupported_reasons(m) == []
    monkeypatch.delenv(ENV)
    assert mat_train.decoder_unsupported_reasons(m)


def test_bogus_value_raises(monkeypatch):
    _need_lib()
    from mat_dcml_amd.ops import mat_fused, mat_train
    monkeypatch.setenv(ENV, "yes")
    with pytest.raises(ValueError, match=ENV):
        mat_train.decoder_unsupported_reasons(_mat())
    with pytest.raises(ValueError, match=ENV):
        mat_fused.unsupported_reasons(_mat())


def test_other_models_ignore_the_switch(monkeypatch):
    """The variable is read only for dec_actor models: a bogus value does not disturb the others."""
    _need_lib()
    from mat_dcml_amd.models.mat import MultiAgentTransformer
    from mat_dcml_amd.ops import mat_train
    monkeypatch.setenv(ENV, "yes")
    assert mat_train.decoder_unsupported_reasons(MultiAgentTransformer(7, 7, 2, 9, 2, 64, 2,
                                                                       action_type="Semi_Discrete")) == []


@pytest.mark.parametrize("kw,needle", [
    (dict(share_actor=False), ("share_actor=False", ENV)),
    (dict(obs_dim=17), ("obs_dim 17", "16")),
    (dict(action_type="Available_Continuous", act_dim=4), ("Available_Continuous", "Discrete, Semi_Discrete and Continuous")),
    (dict(semi_index=-2), ("semi_index -2 != -1",)),
    (dict(action_type="Discrete", act_dim=65), ("action_dim 65 > 64",)),
])
def test_one_reason_per_failed_condition(monkeypatch, kw, needle):
    _need_lib()
    from mat_dcml_amd.ops.paths import gate_reasons
    monkeypatch.setenv(ENV, "fused")
    g = gate_reasons(_mat(**kw))
    assert len(g["train"]) == 1 and all(s in g["train"][0] for s in needle), g
    assert any(all(s in r for s in needle) for r in g["decode"]), g


def test_two_failed_conditions_give_two_reasons(monkeypatch):
    _need_lib()
    from mat_dcml_amd.ops.paths import gate_reasons
    monkeypatch.setenv(ENV, "fused")
    why = gate_reasons(_mat(share_actor=False, obs_dim=17))["train"]
    assert len(why) == 2 and "share_actor=False" in why[0] and "obs_dim 17" in why[1], why


def test_shared_actor_matrix_is_packed():
    """decoder_linears names the shared actor's Linear(64, 64) (the ModelPack / fragment map / fused update tables are
    built from it); per-agent actors pack nothing."""
    from mat_dcml_amd.ops import mat_train
    m = _mat()
    assert mat_train.decoder_linears(m) == [m.decoder.mlp[4]] and tuple(m.decoder.mlp[4].weight.shape) == (64, 64)
    assert mat_train.decoder_linears(_mat(share_actor=False)) == []


ARG_STRUCTS = ("EncP", "DecP", "ActP")
PART_STRUCTS = ("Mat", "LNp", "Blk", "Sv", "HSv")


@pytest.fixture(scope="module")
def c_struct_layout(tmp_path_factory):
    """{"sizeof X": bytes, "X.field": offset} of the kernel argument structs as the C compiler lays them out: one host
    program compiled from the library's own header (the method of tests/test_build_guard.py), shared by the cases."""
    from mat_dcml_amd.ops import mat_train
    csrc = os.path.join(ROOT, "mat_dcml_amd", "csrc")
    lines = [f'  printf("sizeof {n} %zu\\n", sizeof({n}));' for n in ARG_STRUCTS + PART_STRUCTS]
    for st in ARG_STRUCTS:
        lines += [f'  printf("{st}.{n} %zu\\n", offsetof({st}, {n}));' for n, _ in getattr(mat_train, st)._fields_]
    d = tmp_path_factory.mktemp("arg_structs")
    src = d / "sz.hip"
    src.write_text(f'#include <cstdio>\n#include <cstddef>\n#include "{csrc}/mat_train_common.h"\n'
                   'int main() {\n' + "\n".join(lines) + '\n}\n')
    exe = d / "sz"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O0", "--offload-arch=gfx950", str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout
    return {l.rsplit(" ", 1)[0]: int(l.rsplit(" ", 1)[1]) for l in out.strip().splitlines()}


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
@pytest.mark.parametrize("st", ARG_STRUCTS)
def test_actor_arg_struct_matches_ctypes(c_struct_layout, st):
    """EncP's, DecP's and ActP's ctypes mirrors against the C struct's size and EVERY field offset (array and nested
    members at the member's own offset), plus the sizes of the structs they are built from."""
    from mat_dcml_amd.ops import mat_train
    cls = getattr(mat_train, st)
    want = {f"sizeof {n}": ctypes.sizeof(getattr(mat_train, n)) for n in (st,) + PART_STRUCTS}
    want.update({f"{st}.{n}": getattr(cls, n).offset for n, _ in cls._fields_})
    got = {k: v for k, v in c_struct_layout.items() if k in want}
    assert len(want) == len(cls._fields_) + 1 + len(PART_STRUCTS)
    assert got == want, (got, want)
