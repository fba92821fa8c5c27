"""HIP DCML env kernels vs the torch implementation (same Philox draws)."""
import pytest
import torch

from dcml_env_helper import make_pair, run_parity
from mat_dcml_amd.envs.dcml.config import DCMLConfig
from mat_dcml_amd.envs.dcml.vec_env import DeviceDCMLEnv

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("W,fixed,preset,shannon", [(32, False, False, False), (100, False, False, False),
                                                    (100, True, False, False), (100, False, True, False),
                                                    (4, False, False, False), (128, False, False, False),
                                                    (32, False, False, True)])
def test_env_kernel_matches_torch(gpu, W, fixed, preset, shannon):
    """Same Philox draws on both paths, so every INTEGER quantity must match exactly — per worker the transmission
    count n (download + upload retries, DCML_Worker_TIMESLOT_MultiProcess.py:53-106) and the consumed timeslots,
    per env N, K and the standalone flag (DCML_BID_FIRST_MA_ENV_SingleProcess.py:64-105) — and the double-precision
    delays / payment / reward to 1e-6 relative.  The one legitimate exception: an env with a geometric draw whose
    log U / log Pr lies within 1e-6 of an integer (the floor may flip between libm and the device log); those envs
    are flagged from the same draws and excluded.  The standalone (N = 0) and both K-clamp branches are asserted
    on their own subsets.  The body lives in tests/dcml_env_helper.py, shared with tests/test_gpu_env_edges.py."""
    hip, ref = make_pair(gpu, W, E=64, seed=7, fixed=fixed, preset=preset, shannon=shannon)
    assert hip._kern is not None and ref._kern is None
    st = run_parity(hip, ref, steps=8)   # asserts the per-step comparisons and the 1 % cap on exempt env-steps
    if not fixed:
        assert min(st["branch"].values()) > 0, st["branch"]


def test_env_kernel_throughput(gpu):
    cfg = DCMLConfig(n_workers=32)
    env = DeviceDCMLEnv(2048, cfg, device=gpu, seed=1, backend="hip")
    env.reset()
    act = torch.ones(2048, 33, device=gpu)
    act[:, -1] = 0.7
    for _ in range(3):
        env.step(act)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(20):
        env.step(act)
    e.record()
    torch.cuda.synchronize()
    ms = s.elapsed_time(e) / 20
    print(f"dcml_env_step 2048 envs x 32 workers: {ms * 1e3:.1f} us")
    assert ms < 5.0
