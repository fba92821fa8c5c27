"""Every decision of ``ops/mat_fused.decode`` against an fp64 replay of the kernel's own actions, on every launch
variant of the three decode kernels (csrc/mat_decode.hip, csrc/mat_decode_wave.hip): per token the log-prob, per
decision the CDF interval that holds its draw (or the argmax gap), availability, the Normal rows' implied means and
log-prob identity, and the path string of the launch.  The bound of a case is 2.5 x the statistic of the bf16-autocast
eager decoder on the same actions (test_train_edges_helper.token_bound); nothing is measured on the kernels.  The cases,
the dispatch enumeration they come from and the measurements: tests/test_decode_edges_helper.py,
profiles/decode_edges/README.md."""
import contextlib
import time

import pytest
import torch

from mat_dcml_amd.models import act
from mat_dcml_amd.ops import mat_fused
from test_decode_edges_helper import (AVAIL, CONT, MODES, check_decode, double_model, launch_cases, make_inputs,
                                      make_model, replay_logits)

pytestmark = pytest.mark.gpu
B_ENVS = 8
LAUNCH = launch_cases()


@contextlib.contextmanager
def switches(mode, layout=0):
    from mat_dcml_amd.ops.kernels import lib
    saved = mat_fused.WAVE_DECODE, mat_fused.SPEC_DECODE
    mat_fused.WAVE_DECODE, mat_fused.SPEC_DECODE = MODES[mode]
    lib().mdl_decode_spec_layout(layout)
    try:
        yield
    finally:
        lib().mdl_decode_spec_layout(0)
        mat_fused.WAVE_DECODE, mat_fused.SPEC_DECODE = saved


@torch.no_grad()
def yard_logits(m, rep, obs, actions, det, stride):
    """The bf16-autocast eager decoder on the same actions: the teacher-forced pass, or the stride replay."""
    with torch.autocast("cuda", dtype=torch.bfloat16):
        if det and stride > 1 and m.action_type not in AVAIL:
            return replay_logits(m, rep, obs, actions, det, stride).float()
        return m.decoder(act.shifted_from_actions(m, actions).to(rep.dtype), rep, obs).float()


def run_case(dev, cid, kind, A, L, nb, mode, det, path=None, stride=1, B=B_ENVS, ava_mode="mixed", layout=0, gen=False):
    """One decode call per weight set, checked against the fp64 replay.  Returns [(actions, log-probs)] per set."""
    outs, fails = [], []
    for sharp in (False, True):
        t0 = time.perf_counter()
        m = make_model(kind, A, L, nb, dev, sharp=sharp)
        assert mat_fused.supports(m), mat_fused.unsupported_reasons(m)
        obs, rep, ava, rand = make_inputs(m, B, L, A, dev, ava_mode="none" if kind in CONT else ava_mode,
                                          n_cat=2 if kind in AVAIL else None)
        with switches(mode, layout):
            if gen:
                mat_fused.set_sampling_key(m, 11, env0=37)
                k0, k1, ctr = m._mdl_draw_key
                a_k, lp_k = mat_fused.decode(m, rep, ava, det, stride, None)
                rand = act.philox_rand(B, L, A, k0, k1, ctr, 37, dev, normal=kind != "Discrete")
            else:
                a_k, lp_k = mat_fused.decode(m, rep, ava, det, stride, rand)
            got = m._mdl_decode_path
        torch.cuda.synchronize()
        assert path is None or got == path, (cid, got, path)
        lg64 = replay_logits(double_model(m), rep.double(), obs.double(), a_k, det, stride)
        assert lg64.dtype == torch.float64
        yard = yard_logits(m, rep, obs, a_k, det, stride)
        std = None if kind == "Discrete" else m.action_std()
        st, f = check_decode(kind, A, L, lg64, yard, a_k, lp_k, ava, rand, std, det)
        fmt = lambda k: " ".join(f"{v:.3e}" for v in st[k]) if k in st else "-"   # noqa: E731
        print(f"[decode-edges] {cid} | {'det' if det else 'sampled'}{f' stride {stride}' if stride > 1 else ''} | "
              f"{'sharp' if sharp else 'init'} | {got} | lp {fmt('lp')} | mean {fmt('mean')} | "
              f"ident {st.get('normal_lp_identity', float('nan')):.2e} | {time.perf_counter() - t0:.2f} s | "
              f"{'ok' if not f else 'FAIL'}")
        fails += [f"{'sharp' if sharp else 'init'}: {x}" for x in f]
        outs.append((a_k, lp_k))
    assert not fails, f"{cid}: " + "\n".join(fails)
    return outs


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("cid", sorted(LAUNCH))
def test_launch_variant(gpu, cid, det):
    c = LAUNCH[cid]
    run_case(gpu, cid, c["kind"], c["A"], c["L"], c["nb"], c["mode"], det, c["path"], layout=c["layout"])


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("mode", ["spec", "4wave"])
@pytest.mark.parametrize("L,A,kind", [(1, 3, "Discrete"), (1, 2, "Semi_Discrete"), (2, 2, "Semi_Discrete"), (2, 1, "Discrete")])
def test_degenerate_shapes(gpu, L, A, kind, mode, det):
    """One or two agents; Semi_Discrete at L = 1 has no discrete agent, only the Normal row; one action."""
    run_case(gpu, f"degenerate-{kind}-L{L}-A{A}-{mode}", kind, A, L, 2, mode, det, None if mode == "spec" else "4wave")


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("mode", ["spec", "wave", "4wave"])
@pytest.mark.parametrize("B,ava_mode", [(1, "mixed"), (3, "mixed"), (B_ENVS, "none")])
def test_small_batches_and_no_availability(gpu, B, ava_mode, mode, det):
    for kind, A in (("Semi_Discrete", 2), ("Discrete", 6)):
        run_case(gpu, f"batch-B{B}-ava_{ava_mode}-{kind}-{mode}", kind, A, 9, 2, mode, det,
                 "4wave" if mode == "4wave" else None, B=B, ava_mode=ava_mode)


@pytest.mark.parametrize("kind,A", [("Semi_Discrete", 2), ("Discrete", 6)])
@pytest.mark.parametrize("L", [20, 37])
@pytest.mark.parametrize("nb", [1, 2, 3])
def test_stride_mode(gpu, nb, L, kind, A):
    """Batch decisions (deterministic, 4-wave kernel): strides that do not divide n_disc, RMAX = 16 rows and one more,
    n_disc and beyond it, against the stride replay.  Sampled calls ignore the stride bit for bit."""
    n_disc = L if kind == "Discrete" else L - 1
    for stride in (3, 16, 17, n_disc, n_disc + 5):
        run_case(gpu, f"stride-nb{nb}-{kind}-L{L}", kind, A, L, nb, "spec", True, "4wave", stride=stride)
    one = run_case(gpu, f"stride-nb{nb}-{kind}-L{L}-sampled", kind, A, L, nb, "spec", False, stride=1)
    for stride in (3, 17):
        other = run_case(gpu, f"stride-nb{nb}-{kind}-L{L}-sampled", kind, A, L, nb, "spec", False, stride=stride)
        for (a1, lp1), (a2, lp2) in zip(one, other):
            assert torch.equal(a1, a2) and torch.equal(lp1, lp2)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("kind,A", [("Continuous", 1), ("Continuous", 2), ("Continuous", 16), ("Continuous", 17),
                                    ("Continuous", 64), ("Available_Continuous", 3), ("Available_Continuous", 16)])
def test_continuous_types(gpu, kind, A, nb, det):
    for L in (1, 2, 17):
        run_case(gpu, f"{kind}-A{A}-nb{nb}-L{L}", kind, A, L, nb, "spec", det, "4wave")


@pytest.mark.parametrize("kind,A,mode", [("Semi_Discrete", 2, "spec"), ("Semi_Discrete", 2, "wave"),
                                         ("Semi_Discrete", 2, "4wave"), ("Discrete", 6, "spec"), ("Discrete", 6, "wave"),
                                         ("Discrete", 6, "4wave"), ("Continuous", 5, "4wave")])
def test_inkernel_draws_decision_by_decision(gpu, kind, A, mode):
    """rand=None: the kernel's own Philox draws at env0 = 37, rebuilt on the host by models/act.philox_rand, explain
    every decision and every Normal sample."""
    want = {"spec": "spec(nreg=0)" if A <= 4 else "spec(nreg=6)", "wave": "wave(nreg=2)", "4wave": "4wave"}[mode]
    run_case(gpu, f"inkernel-{kind}-{mode}", kind, A, 17, 2, mode, False, want, gen=True)
