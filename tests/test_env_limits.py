"""The DCML env's Python-side kernel limits: equal to the kernel's own (``MAXW`` / ``MAXP`` in csrc/dcml_env.hip, which
the host entry points refuse beyond), ``backend="auto"`` takes the torch path past them and ``backend="hip"`` raises at
construction.  CPU only: nothing is launched."""
import os
import re

import pytest

from mat_dcml_amd.envs.dcml import vec_env
from mat_dcml_amd.envs.dcml.config import DCMLConfig
from mat_dcml_amd.envs.dcml.vec_env import DeviceDCMLEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "mat_dcml_amd", "csrc", "dcml_env.hip")


def _define(text, name):
    m = re.findall(rf"^#define\s+{name}\s+(\d+)\s*$", text, flags=re.M)
    assert len(m) == 1, (name, m)
    return int(m[0])


def test_python_limits_equal_kernel_limits():
    with open(SRC) as f:
        text = f.read()
    assert vec_env.MAX_KERNEL_WORKERS == _define(text, "MAXW")
    assert vec_env.MAX_KERNEL_PERIOD == _define(text, "MAXP")
    # both host entry points refuse beyond them before any launch
    assert text.count("if (c->W > MAXW || c->P > MAXP) return -1;") == 2


def test_auto_backend_takes_torch_path_beyond_limit():
    for cfg in (DCMLConfig(n_workers=257), DCMLConfig(n_workers=4, period=65)):
        env = DeviceDCMLEnv(2, cfg, device="cpu", backend="auto")
        assert env._kern is None


def test_hip_backend_raises_at_construction_beyond_limit():
    with pytest.raises(RuntimeError, match="at most 256 workers"):
        DeviceDCMLEnv(2, DCMLConfig(n_workers=257), device="cpu", backend="hip")
    with pytest.raises(RuntimeError, match="period of 64"):
        DeviceDCMLEnv(2, DCMLConfig(n_workers=4, period=65), device="cpu", backend="hip")
    DeviceDCMLEnv(2, DCMLConfig(n_workers=256), device="cpu", backend="hip")   # at the limit: accepted
