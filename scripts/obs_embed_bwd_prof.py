"""The wide-observation embedding backward (csrc/obs_embed.hip) at SMAC's training minibatch (86,400 tokens x 1,288
bf16 features) in both gradient modes, 3 x 10 calls each, alternating — for a kernel trace:

    rocprofv3 --kernel-trace --stats -d OUT -o bwd --output-format csv -- python scripts/obs_embed_bwd_prof.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mat_dcml_amd.ops import mat_train   # noqa: E402
from test_gpu_train import make_discrete   # noqa: E402

gpu = torch.device("cuda:0")
N, od = 86400, 1288
oe = mat_train.ObsEmbed(make_discrete(3, 5, od, gpu, seed=4))
g = torch.Generator(device=gpu).manual_seed(6)
obs = (torch.rand(N, od, device=gpu, generator=g) * (torch.rand(N, od, device=gpu, generator=g) < 0.3)).to(torch.bfloat16)
dpre = torch.randn(N, 64, device=gpu, generator=g)
_, stat = oe.forward(obs)
for p in (oe.lin.weight, oe.lin.bias, oe.ln.weight, oe.ln.bias):
    p.grad = torch.zeros_like(p)
for _ in range(3):
    for mode in ("atomic", "partials"):
        oe.grad_mode = mode
        for _ in range(10):
            oe.backward(obs, stat, dpre)
        torch.cuda.synchronize()
print("done")
