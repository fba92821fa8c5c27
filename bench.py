#!/usr/bin/env python
"""Headline benchmark: MAT-AS PPO training throughput on 32-worker DCML (BASELINE.json).

One "step" = one full PPO iteration of the reference training loop (``dcml_runner.py:39-91``): a T=50-step
stochastic rollout over the rank's 256 vectorised envs (encoder + autoregressive MAT decode + env step per
step) followed by the complete MAT-PPO update (15 epochs x 4 minibatches, next-value + GAE recomputed each
epoch, clip / Huber / ValueNorm / grad clip / Adam, gradient all-reduce under DP).  Nothing is skipped inside
the timed region.  Weak scaling: every rank owns 256 envs, so the node runs 256·N envs.

    python bench.py --gpus 1 --steps 5 --warmup 2
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29500 \
        bench.py --gpus 8 --steps 5 --warmup 2

Rank 0 prints ONE JSON line; ``value`` = whole-node env-steps/s (max time over ranks).
Baseline = 43 env-steps/s: the reference itself on the 32-worker config (CPU, measured).

A plain run sets up, warms up, times ``--steps`` iterations and prints the line.  ``--full`` adds what takes runs of
its own after the timed loop: the per-phase breakdown (``--steps`` more instrumented iterations) and the eval block
(the reference benchmark sweep for a random-init policy, the trained checkpoints and the fixed heuristic).
``--dump-outputs DIR`` writes what the last timed iteration left with its caller as ``DIR/<name>.npy``.
"""
import argparse
import json
import os
import sys
import time

import torch

BASELINE_ENV_STEPS_PER_S = 43.0
METRIC = "env-steps/sec (whole node) MAT-AS 32-worker DCML at 1/2/4/8 GPU; eval task time"
# reference training FPS measured on its own code per worker count (41-43 at 32 workers, 8 at 100)
BASELINE_BY_WORKERS = {32: 43.0, 100: 8.0}


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1,
                   help="ranks = GPUs; without WORLD_SIZE in the env bench.py starts that many rank processes itself")
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--n_workers", type=int, default=32)
    p.add_argument("--envs", type=int, default=256, help="vectorised envs per GPU")
    p.add_argument("--episode_length", type=int, default=50)
    p.add_argument("--ppo_epoch", type=int, default=15)
    p.add_argument("--num_mini_batch", type=int, default=4)
    p.add_argument("--kernels", default="auto")
    p.add_argument("--dtype", default="bf16")
    p.add_argument("--full", action="store_true",
                   help="after the timed loop also run the phase breakdown and the eval block (each can still be "
                        "switched off with --no_phase_timers / --no_eval); a plain run measures the headline only")
    p.add_argument("--dump-outputs", dest="dump_outputs", default=None, metavar="DIR",
                   help="write what the last timed step computed (its training statistics, the updated parameters "
                        "and the rollout it stored) as DIR/<name>.npy, at most 64 MB in all")
    p.add_argument("--phases", action="store_true", help="also print the phase summary to stderr (with --full)")
    p.add_argument("--no_phase_timers", action="store_true",
                   help="with --full: skip the phase breakdown (extra instrumented steps after the timed loop; the "
                        "timed loop itself never records phase events)")
    p.add_argument("--allreduce", default="rccl", choices=["rccl", "oneshot", "auto", "ordered"],
                   help="data-parallel gradient all-reduce: RCCL (default), the one-shot peer-memory kernel, auto "
                        "(one-shot only if it matches RCCL and is faster at start-up), or ordered (all-gather + "
                        "rank-order sum: bitwise independent of how the buffer is split)")
    p.add_argument("--grad_overlap", action="store_true",
                   help="data parallelism: all-reduce the decoder's gradient slice under the encoder backward")
    p.add_argument("--config", default="dcml", choices=["dcml", "smac"],
                   help="dcml: the headline 32-worker DCML config; smac: MAT on the SMAC-shaped 27m_vs_30m stress env")
    p.add_argument("--rollout_groups", type=int, default=1,
                   help="env groups of the pipelined rollout (each on its own stream; identical rollout)")
    p.add_argument("--no_eval", action="store_true",
                   help="with --full: skip the post-timing eval sweep (ct / payment / latency)")
    p.add_argument("--model_dir", default=None,
                   help="trained checkpoint for the eval block (default: the committed 32-worker run, if it matches)")
    a = p.parse_args()
    if a.phases and not (a.full and not a.no_phase_timers):
        p.error("--phases prints the phase breakdown, which runs only with --full (and without --no_phase_timers)")
    return a


def launch_ranks(n):
    """``--gpus N`` without a torchrun launcher: start N rank processes (children, never exec) with the torchrun
    env contract, before this process touches the GPU; exit with the first failing rank's code."""
    import signal
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    try:
        while procs:
            for p in list(procs):
                code = p.poll()
                if code is None:
                    continue
                procs.remove(p)
                if code != 0 and rc == 0:
                    rc = code
                    for q in procs:   # a dead rank leaves the others blocked in a collective
                        q.send_signal(signal.SIGTERM)
            time.sleep(0.2)
    finally:
        for p in procs:
            p.kill()
    return rc if rc >= 0 else 128 - rc


def measure_the_built_library():
    """Where this user cannot write the library's directory, the benchmark cannot rebuild the library anyway: hide
    the compiler from the loader (``csrc/build.py`` reads ``HIPCC``), so that a stale library is reported as stale
    instead of as a failed write, and nothing is compiled inside a run whose time is being measured.  This file is
    also the yardstick for A/B runs against other revisions of the package (``scripts/build_ab.sh``); revisions whose
    loader opens its rebuild lock before it checks the library could not load in such a tree at all without this.
    Only set in that case, for this process and the rank processes it starts."""
    lib_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mat_dcml_amd", "_lib")
    if os.path.exists(os.path.join(lib_dir, "libmatdcml.so")) and not os.access(lib_dir, os.W_OK):
        os.environ["HIPCC"] = os.path.join(lib_dir, "no-compiler-for-a-read-only-tree")


def main():
    a = parse()
    measure_the_built_library()
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        sys.exit(launch_ranks(a.gpus))
    if a.config == "smac":
        return bench_smac(a)

    from mat_dcml_amd.config import get_config, parse_args
    from mat_dcml_amd.ops.paths import kernel_report
    from mat_dcml_amd.parallel.comm import init_from_env
    from mat_dcml_amd.runner.dcml_runner import DCMLRunner

    os.environ["MAT_DCML_ALLREDUCE"] = a.allreduce
    comm = init_from_env(prefer_gpu=True)
    if comm.world_size != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={comm.world_size}: the launch does not match")
    topo = comm.describe()
    if comm.device.type == "cuda" and topo["shared_devices"] and os.environ.get("MAT_DCML_SHARE_DEVICES") != "1":
        raise SystemExit(f"bench.py: ranks share GPUs {topo['devices']}")
    argv = ["--env_name", "DCML", "--scenario", "AS", "--algorithm_name", "mat", "--n_rollout_threads", str(a.envs),
            "--episode_length", str(a.episode_length), "--lr", "5e-5", "--ppo_epoch", str(a.ppo_epoch),
            "--num_mini_batch", str(a.num_mini_batch), "--gamma", "0.99", "--use_valuenorm", "--use_popart",
            "--entropy_coef", "0.01", "--n_workers", str(a.n_workers), "--kernels", a.kernels, "--dtype", a.dtype,
            "--seed", "1", "--rollout_groups", str(a.rollout_groups)]
    if a.phases:
        argv.append("--profile_phases")
    if a.grad_overlap:
        argv.append("--grad_overlap")
    args = parse_args(argv, get_config(), warn=False)
    runner = DCMLRunner({"all_args": args, "device": comm.device, "run_dir": None, "comm": comm})
    runner.warmup()
    dev = comm.device

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)

    for _ in range(a.warmup):
        runner.train_iteration()
    paths = kernel_report(runner)   # after the warm-up: the decode entry names the kernel its calls ran on
    runner.timers.enabled = False    # the headline loop runs uninstrumented
    sync()
    comm.barrier()
    sync()
    comm.enable_timing(True)   # hipEvents around the critical-path collectives (grad average, epoch statistics)
    t0 = time.perf_counter()
    infos = None
    for _ in range(a.steps):
        infos = runner.train_iteration()
    sync()
    t_rank = time.perf_counter() - t0      # this rank's own time, before waiting for the others
    comm.barrier()
    sync()
    dt = time.perf_counter() - t0
    t = torch.tensor([dt], dtype=torch.float64, device=dev)
    comm.all_reduce_max_(t)
    dt = float(t)
    n = comm.world_size
    comm_ms = comm.timing_ms()
    comm.enable_timing(False)
    per_rank = comm.all_gather_object((round(t_rank / a.steps * 1e3, 3), comm_ms))
    diag = {"rank_ms_per_step": [r[0] for r in per_rank],
            "comm_ms_per_step": {k: round(max(r[1].get(k, 0.0) for r in per_rank) / a.steps, 4)
                                 for k in ("grad_allreduce", "stats_allreduce")},
            "collectives_per_step": {k: max(r[1].get(k + "_calls", 0) for r in per_rank) // max(a.steps, 1)
                                     for k in ("grad_allreduce", "stats_allreduce")}}
    if a.dump_outputs and comm.is_main:   # before anything below runs the trainer again
        dump_outputs(a.dump_outputs, runner, infos)
    phases = phase_breakdown(a, runner, comm, sync) if a.full and not a.no_phase_timers else None
    env_steps = a.steps * a.episode_length * a.envs * n
    value = env_steps / dt
    eval_info = None
    if a.full and not a.no_eval and comm.is_main and dev.type == "cuda":
        eval_info = eval_block(a, args, runner, dev)
    if comm.is_main:
        if a.phases and phases:
            print(phases, file=sys.stderr)
        print(json.dumps({
            "metric": METRIC if a.n_workers == 32 else f"env-steps/sec (whole node) MAT-AS {a.n_workers}-worker DCML",
            "value": round(value, 2), "unit": "env-steps/s", "n_gpus": topo["distinct_devices"], "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": (round(value / BASELINE_BY_WORKERS[a.n_workers], 2)
                                           if a.n_workers in BASELINE_BY_WORKERS else None),
            "dtype": a.dtype if dev.type == "cuda" else "fp32",
            "data": "synthetic (on-device DCML env simulation, Philox streams; random-init MAT weights)",
            "config": {"model": f"MAT (2+2 blocks, d=64, 2 heads) on DCML {a.n_workers}-worker bid-first env "
                                f"({a.n_workers + 1} agents)",
                       "global_batch": a.envs * n, "seq_len": a.n_workers + 1,
                       "parallelism": f"dp{n}", "envs_per_gpu": a.envs, "episode_length": a.episode_length,
                       "ppo_epoch": a.ppo_epoch, "num_mini_batch": a.num_mini_batch,
                       "rollout_groups": runner._groups(),
                       "device": torch.cuda.get_device_name(dev) if dev.type == "cuda" else "cpu"},
            "ranks": n, "backend": topo["backend"], "rank_devices": topo["devices"], "hosts": topo["hosts"],
            "kernels": paths, "native_build": _native_build(), "grad_allreduce": getattr(runner.trainer, "grad_allreduce", topo["backend"]) if n > 1 else None,
            "grad_allreduce_probe": comm.oneshot_probe,
            # which gradient path ran: the workspace mode, bit-reproducibility, the update
            # launch, and under data parallelism the single blocking all-reduce vs the overlapped two-slice schedule
            "grad_path": _grad_path(runner.trainer, n),
            "deterministic": bool(getattr(runner.trainer, "deterministic", False)),
            # scaling diagnostics: each rank's own ms per step (max = ms_per_step up to the closing barrier) and the
            # critical-path collective time per step (hipEvents on the compute stream, max over ranks)
            **diag,
            # per-phase GPU time per step (decode / env / insert / update; train_fwd / train_bwd = the four fused
            # training kernels inside the update) and the training kernels per minibatch
            **(phases or {}),
            "eval": eval_info,
        }), flush=True)
    comm.destroy()


def phase_breakdown(a, runner, comm, sync):
    """Where a step's time goes: ``a.steps`` MORE iterations after the timed loop with a hipEvent pair around EVERY
    phase occurrence (pack / decode / env / insert per rollout step, update; train_fwd / train_bwd per minibatch).
    Nothing is sampled or scaled, so the phases partition the instrumented step up to the GPU idle between them;
    the headline loop above runs without any events (each pair costs a few us of stream bubble)."""
    runner.timers.enabled = True
    runner.timers.every.clear()
    runner.timers.summary(reset=True)
    sync()
    comm.barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        runner.train_iteration()
    sync()
    dt = time.perf_counter() - t0
    tot = runner.timers.totals_ms()
    runner.timers.summary(reset=True)
    runner.timers.enabled = False
    n_mb = a.steps * a.ppo_epoch * a.num_mini_batch
    ph = {k: round(v / a.steps, 3) for k, v in tot.items()}
    top = sum(ph.get(k, 0.0) for k in ("pack", "decode", "env", "insert", "update"))
    return {"phase_ms_per_step": ph,
            "phase_run": {"ms_per_step": round(dt / a.steps * 1e3, 3), "phases_sum_ms": round(top, 3),
                          "note": "phases = pack + decode + env + insert + update of separate instrumented steps "
                                  "(every occurrence timed); train_fwd / train_bwd lie inside update"},
            "train_kernels_ms_per_minibatch": {k[6:]: round(tot[k] / n_mb, 4) for k in ("train_fwd", "train_bwd")
                                               if k in tot}}


DUMP_BUDGET_BYTES = 64 << 20
DUMP_ROLLOUT = ("actions", "action_log_probs", "value_preds", "rewards", "returns", "advantages")


def dump_outputs(out_dir, runner, infos):
    """``--dump-outputs DIR``: what a caller of the timed path holds after the last timed ``train_iteration()``, one
    float32 / float64 ``DIR/<name>.npy`` each: the training statistics it returned (``info_<key>``), the parameters
    its update left (``params``, flat, in ``parameters()`` order) and the rollout it stored (``rollout_<field>``).
    The env, the sampling noise and the initial weights are all seeded by the arguments, so two builds run with the
    same arguments see identical inputs.  An array above its share of the 64 MB budget is written as a fixed seeded
    sample of its elements (same indices for the same shape)."""
    import numpy as np
    arrays = {f"info_{k}": torch.as_tensor(v).detach().double().reshape(-1) for k, v in (infos or {}).items()}
    arrays["params"] = torch.cat([p.detach().reshape(-1).float() for p in runner.policy.transformer.parameters()])
    for name in DUMP_ROLLOUT:
        arrays[f"rollout_{name}"] = getattr(runner.buffer, name).detach().float()
    cap = DUMP_BUDGET_BYTES // len(arrays)
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), sample_within(t.cpu().numpy(), cap))


def sample_within(x, cap_bytes):
    """``x`` itself when it fits in ``cap_bytes``; otherwise ``cap_bytes`` worth of its elements at distinct, sorted
    flat indices drawn with a fixed seed (the same indices for the same size and cap)."""
    import numpy as np
    if x.nbytes <= cap_bytes:
        return x
    idx = np.sort(np.random.default_rng(0).choice(x.size, cap_bytes // x.itemsize, replace=False))
    return x.reshape(-1)[idx]


def _grad_path(tr, n):
    m = tr.policy.transformer
    return {"workspace": getattr(m, "_mdl_gws_mode", None), "fused_update": bool(getattr(tr, "_upd_fused", False)),
            "minibatch_inputs": ("in-kernel index" if os.environ.get("MAT_DCML_MB_INDEX", "gather") == "kernel" else
                                 "gather" + (" (next minibatch's on a side stream)" if getattr(tr, "gather_ahead", False)
                                             else " (next minibatch's inside the update launch)"
                                             if getattr(tr, "fused_gather", False) and getattr(tr, "_upd_fused", False)
                                             else "")),
            "allreduce": None if n == 1 else ("overlap(decoder slice under enc_bwd)" if tr.grad_overlap else
                                              f"single blocking ({getattr(tr, 'grad_allreduce', 'rccl')})")}


def _native_build():
    """Source hash of the loaded HIP library (ops/kernels.lib() checked it against the tree), or None."""
    from mat_dcml_amd.ops import kernels
    return kernels.BUILD_ID


# Trained checkpoints of the eval block, per worker count: (JSON key, path).  "trained" is always the reference reward
# -(99 ct + payment) (reward_beta 1); 32 workers also report the round-5 payment-weight-3 run next to it.  Each was
# selected on the held-out preset sets Sample_2..10 (profiles/r6_train*/README.md, profiles/r5_train32/README.md).
DEFAULT_CKPT = {32: [("trained", "profiles/r6_train32/selected_beta1.pt"),
                     ("trained_beta3", "profiles/r5_train32/transformer_500_beta3.pt")],
                100: [("trained", "profiles/r6_train100/selected_beta1.pt")]}


def eval_block(a, args, runner, dev):
    """"Eval task time": the reference benchmark protocol (``DCML_MAT_ALT_Benchmark.py:114-146``: preset replay,
    11-point available-worker sweep, 1000 deterministic decisions per point, batch decision stride 10) for
    (1) a fresh random-init MAT (``torch.manual_seed(1)``, BASELINE.md's random-init row), (2) the trained
    checkpoints (``--model_dir``, default ``DEFAULT_CKPT[n_workers]``) and (3) the fixed heuristic.  Independent of
    ``--steps``: the benchmarked runner's weights are never used here."""
    from mat_dcml_amd.algos.policy import TransformerPolicy
    from mat_dcml_amd.envs.dcml.spaces import dcml_action_spaces
    from mat_dcml_amd.runner.benchmark import eval_report, frontier_counts, run_sweep

    def fresh_policy():
        torch.manual_seed(1)
        envs = runner.envs
        return TransformerPolicy(args, envs.observation_space[0], envs.share_observation_space[0],
                                 dcml_action_spaces(runner.dcml.n_workers)[0], runner.num_agents, device=dev)

    def summary(res):
        out = {"ct": [round(x, 4) for x in res["ct"]], "payment": [round(x, 3) for x in res["payment"]],
               "ct_mean": round(sum(res["ct"]) / len(res["ct"]), 4),
               "payment_mean": round(sum(res["payment"]) / len(res["payment"]), 3)}
        if "decision_ms_b1" in res:
            out["decision_ms_b1_stride10"] = round(res["decision_ms_b1"], 4)
            out["decision_ms_batched"] = round(res["decision_ms_batched"], 4)
        return out

    kw = dict(sweep="AW", n_points=11, steps=1000, shards=50, stride=10, verbose=False)
    info = {"protocol": "DCML_MAT_ALT_Benchmark.py AW sweep: 11 points x 1000 preset decisions, stride 10, "
                        f"{a.n_workers} workers (available-worker steps scaled to the pool)"}
    info["random_init"] = summary(run_sweep(fresh_policy(), runner.dcml, dev, latency_b1=20, **kw))
    ckpts = [("trained", a.model_dir)] if a.model_dir else DEFAULT_CKPT.get(a.n_workers, [])
    for key, ckpt in ckpts:
        if not (ckpt and os.path.exists(ckpt)):
            continue
        pol = fresh_policy()
        pol.restore(ckpt)
        ent = info[key] = summary(run_sweep(pol, runner.dcml, dev, latency_b1=20 if key == "trained" else 0, **kw))
        ent["checkpoint"] = ckpt
        # held-out preset sets (Sample_2..10, which the reference benchmark never reads) and, on Sample_1, where each
        # point lies against the heuristic's own ct-payment trade-off (K = floor(rho N), rho = 0.3 .. 1.0)
        rep = eval_report(pol, runner.dcml, dev, **{k: v for k, v in kw.items() if k != "verbose"})
        ent["wins_vs_fixed_sample1"] = {k: rep["per_sample"][1][k] for k in ("ct_wins", "payment_wins", "both_wins")}
        ent["heldout"] = rep.get("heldout")
        fr = rep.get("frontier") or []
        ent["frontier"] = {"ratios": rep.get("frontier_ratios"),
                           "beyond_per_point": [f["beyond"] for f in fr],
                           "dominated_by_per_point": [f["dominated_by"] for f in fr],
                           "payment_margin_per_point": [f["margin"] for f in fr],
                           "outside_per_point": [f["outside"] for f in fr],
                           "dominates_per_point": [f["dominates"] for f in fr],
                           # only numeric positive margins count; points faster than every heuristic
                           # setting are counted apart, with no verdict
                           **{k + "_count": v for k, v in frontier_counts(fr).items()}}
    info["fixed_heuristic"] = summary(run_sweep(None, runner.dcml, dev, fixed=True, latency_b1=0, **kw))
    return info


def bench_smac(a):
    """BASELINE config #5 (cross-env stress): MAT on the SMAC-shaped 27m_vs_30m env, 32 envs per GPU,
    episode_length 100, ppo_epoch 15, 1 minibatch, clip 0.05 (train_smac.sh)."""
    from mat_dcml_amd.config import _SMAC_FLAGS, get_config, parse_args
    from mat_dcml_amd.parallel.comm import init_from_env
    from mat_dcml_amd.runner.smac_runner import SMACRunner
    os.environ["MAT_DCML_ALLREDUCE"] = a.allreduce
    comm = init_from_env(prefer_gpu=True)
    if comm.world_size != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={comm.world_size}: the launch does not match")
    envs = a.envs if a.envs != 256 else 32
    T = a.episode_length if a.episode_length != 50 else 100
    argv = ["--env_name", "StarCraft2", "--algorithm_name", "mat", "--map_name", "27m_vs_30m", "--n_rollout_threads",
            str(envs), "--episode_length", str(T), "--lr", "5e-4", "--ppo_epoch", "15", "--num_mini_batch", "1",
            "--clip_param", "0.05", "--use_value_active_masks", "--kernels", a.kernels, "--dtype", a.dtype]
    args = parse_args(argv, get_config(), extra=_SMAC_FLAGS, warn=False)
    runner = SMACRunner({"all_args": args, "device": comm.device, "run_dir": None, "comm": comm})
    runner.warmup()
    dev = comm.device
    for _ in range(a.warmup):
        runner.train_iteration()
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    comm.barrier()
    t0 = time.perf_counter()
    infos = None
    for _ in range(a.steps):
        infos = runner.train_iteration()
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    comm.barrier()
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
    comm.all_reduce_max_(t)
    dt, n = float(t), comm.world_size
    if a.dump_outputs and comm.is_main:
        dump_outputs(a.dump_outputs, runner, infos)
    value = a.steps * T * envs * n / dt
    if comm.is_main:
        print(json.dumps({"metric": "env-steps/sec (whole node) MAT on SMAC 27m_vs_30m (synthetic SMAC-shaped env)",
                          "value": round(value, 2), "unit": "env-steps/s", "n_gpus": n, "steps": a.steps,
                          "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 3), "higher_is_better": True,
                          "scaling": "weak", "vs_baseline": None, "dtype": a.dtype,
                          "data": "synthetic (SMAC-shaped on-device env: 27 agents x 1288 obs, 36 actions)",
                          "config": {"model": "MAT (2+2 blocks, d=64, 2 heads) on SMAC 27m_vs_30m", "global_batch":
                                     envs * n, "seq_len": 27, "parallelism": f"dp{n}", "episode_length": T}}),
              flush=True)
    comm.destroy()


if __name__ == "__main__":
    main()
