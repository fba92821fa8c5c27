"""Comparison helpers of tests/test_gpu_train_edges.py and their CPU self-tests: the per-token output statistic with
its bound, the per-row gradient statistic, and a Python mirror of the training kernels' persistent tiling
(csrc/mat_train_common.h FOR_TILES / chunk_plan / stagger_chunk) that names the workgroup and chunk of a sequence."""
import torch

YARD_FACTOR = 2.5        # the project's factor over the bf16-autocast error (tests/test_gpu_train.py)
TOKEN_BOUND_FLOOR = 2.5e-3   # = YARD_FACTOR x 1e-3: a yardstick below 1e-3 does not tighten the bound further
ROW_FLOOR = 1e-3         # a row's norm-ratio denominator is at least this fraction of the whole tensor's norm

FWD_NW, BWD_NW = 4, 8    # waves per workgroup of the forward / backward translation units (MDL_NW, MDL_CT_BWD_NW)
CHUNK_A4 = 8             # MDL_CHUNK_A4


def rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-300)).item()


def token_errors(k, ref):
    """|k - ref| / (1 + |ref|) per element, in fp64."""
    k, ref = k.detach().double().cpu(), ref.detach().double().cpu()
    assert k.shape == ref.shape, (k.shape, ref.shape)
    return (k - ref).abs() / (1.0 + ref.abs())


def token_stat(k, ref):
    """max_t |k - ref| / (1 + |ref|): one wrong token is the statistic, however many right ones surround it."""
    e = token_errors(k, ref)
    return float("nan") if bool(torch.isnan(e).any()) else e.max().item()


def token_bound(yard):
    """2.5 x the yardstick's own statistic, floored where the yardstick is below 1e-3."""
    return max(TOKEN_BOUND_FLOOR, YARD_FACTOR * yard)


def token_check(k, ref, yard_out):
    """(statistic of k, statistic of the yardstick, bound, ok)."""
    s, y = token_stat(k, ref), token_stat(yard_out, ref)
    b = token_bound(y)
    return s, y, b, bool(s <= b)


def row_stats(g, ref, dim):
    """Norm ratio of every slice of ``g`` along ``dim`` against the same slice of ``ref``, the denominator floored at
    ROW_FLOOR x the whole tensor's norm."""
    g, ref = g.detach().double().cpu(), ref.detach().double().cpu()
    other = tuple(d for d in range(ref.dim()) if d != dim)
    den = ref.norm(dim=other).clamp_min(ROW_FLOOR * ref.norm().item())
    return (g - ref).norm(dim=other) / den


# ------------------------------------------------------------------------------------------------ persistent tiling
def chunk_rounds(s, L, nw):
    return (((s * L + 15) >> 4) + nw - 1) // nw


def chunk_plan(n, SQ, L, nw):
    """> 0: that many near-equal chunks; < 0: -(number of chunks) of SQ sequences each but the last."""
    if n <= 0:
        return 0
    n0 = (n + SQ - 1) // SQ

    def bal(k):
        q, r = divmod(n, k)
        return 4 * (r * chunk_rounds(q + 1, L, nw) + (k - r) * chunk_rounds(q, L, nw)) + CHUNK_A4 * k

    best, cost = n0, bal(n0)
    cg = 4 * ((n0 - 1) * chunk_rounds(SQ, L, nw) + chunk_rounds(n - (n0 - 1) * SQ, L, nw)) + CHUNK_A4 * n0
    if cg < cost:
        best, cost = -n0, cg
    if n0 + 1 <= n and bal(n0 + 1) < cost:
        best = n0 + 1
    return best


def workgroup_walk(B, SQ, L, grid, w, backward):
    """[(first sequence, sequences)] of workgroup ``w``'s chunks in the order it walks them: workgroup w owns
    [B w / G, B (w + 1) / G); the backward's odd groups of 8 workgroups walk in reverse."""
    lo, hi = B * w // grid, B * (w + 1) // grid
    n = hi - lo
    plan = chunk_plan(n, SQ, L, BWD_NW if backward else FWD_NW)
    nch = abs(plan)
    out = []
    for it in range(nch):
        ch = nch - 1 - it if (backward and nch >= 2 and ((w >> 3) & 1)) else it
        if plan < 0:
            s0, ns = lo + ch * SQ, min(SQ, n - ch * SQ)
        else:
            s0 = lo + n * ch // nch
            ns = lo + n * (ch + 1) // nch - s0
        out.append((s0, ns))
    return out


def launch_grid(B, SQ, n_cu, backward):
    tiles = -(-B // SQ)
    return min(tiles, n_cu if backward else 2 * n_cu)


def chunk_map(B, SQ, L, grid, backward):
    """Per sequence: (workgroup, step of its walk, chunks in the walk, sequences in the chunk)."""
    out = [None] * B
    for w in range(grid):
        walk = workgroup_walk(B, SQ, L, grid, w, backward)
        for it, (s0, ns) in enumerate(walk):
            for s in range(s0, s0 + ns):
                assert out[s] is None, s
                out[s] = (w, it, len(walk), ns)
    assert all(o is not None for o in out)
    return out


def describe_sequences(seqs, B, SQ, L, n_cu):
    """Where the given sequences run: 'seq 17: fwd wg 3 chunk 2/2 (3 seq), bwd wg 1 chunk 3/3 (5 seq)'."""
    fwd = chunk_map(B, SQ, L, launch_grid(B, SQ, n_cu, False), False)
    bwd = chunk_map(B, SQ, L, launch_grid(B, SQ, n_cu, True), True)
    part = lambda m: f"wg {m[0]} chunk {m[1] + 1}/{m[2]} ({m[3]} seq)"  # noqa: E731
    return "; ".join(f"seq {s}: fwd {part(fwd[s])}, bwd {part(bwd[s])}" for s in seqs)


# ------------------------------------------------------------------------------------------------ CPU self-tests
def test_per_token_statistic_sees_one_wrong_token_that_the_norm_ratio_accepts():
    """An fp64 'reference' logp of the largest case's shape, a 'yardstick' and a 'kernel' copy that differ from it by
    Gaussian noise of one scale (bf16's 2^-9 half-ulp on values of order 1), and ONE kernel token moved by 20 x the
    bound: the per-token check rejects it, the whole-tensor norm ratio of tests/test_gpu_train.py (< 3e-2) accepts."""
    g = torch.Generator().manual_seed(0)
    ref = -(torch.randn(1287, 33, 1, generator=g, dtype=torch.float64).abs() + 0.05)
    sigma = 2.0 ** -9
    yard = ref + sigma * torch.randn(ref.shape, generator=g, dtype=torch.float64)
    kern = ref + sigma * torch.randn(ref.shape, generator=g, dtype=torch.float64)
    s, y, b, ok = token_check(kern, ref, yard)
    assert ok and 0 < s <= b and b == YARD_FACTOR * y > TOKEN_BOUND_FLOOR, (s, y, b)
    bad = kern.clone()
    seq, tok = 1000, 32
    bad[seq, tok, 0] += 20 * b * (1 + ref[seq, tok, 0].abs())
    s2, _, b2, ok2 = token_check(bad, ref, yard)
    assert b2 == b and not ok2 and s2 > 19 * b, (s2, b)
    assert rel(bad, ref) < 3e-2, rel(bad, ref)            # the old check cannot see it
    per_seq = token_errors(bad, ref).amax(dim=(1, 2))
    assert (per_seq > b).nonzero().flatten().tolist() == [seq]
    assert not token_check(torch.full_like(ref, float("nan")), ref, yard)[3]   # NaN never passes


def test_token_bound_floor():
    assert token_bound(0.0) == TOKEN_BOUND_FLOOR == token_bound(9.9e-4)
    assert abs(token_bound(1e-3) - TOKEN_BOUND_FLOOR) < 1e-15 and abs(token_bound(4e-3) - 1e-2) < 1e-15


def test_row_statistic_sees_one_wrong_row():
    g = torch.Generator().manual_seed(1)
    ref = torch.randn(64, 6, generator=g, dtype=torch.float64)
    ref[:, 5] *= 1e-6                                     # a nearly unused token id: its denominator is the floor
    k = ref + 1e-3 * torch.randn(ref.shape, generator=g, dtype=torch.float64)
    k[:, 2] = ref[:, 2] * 1.5
    r = row_stats(k, ref, 1)
    assert r.shape == (6,) and r[2] > 0.4 and bool((r[[0, 1, 3, 4]] < 6e-2).all()), r
    assert abs(r[5].item() - (k[:, 5] - ref[:, 5]).norm().item() / (ROW_FLOOR * ref.norm().item())) < 1e-12
    assert rel(k, ref) < 0.25 < r[2]


def test_tiling_mirror_gives_the_bench_chunks():
    """13 sequences of 33 agents per backward workgroup (SQ = 5): chunks (5, 5, 3), walked (3, 5, 5) in odd groups of
    8 workgroups; 6-7 per forward workgroup: two chunks (csrc/mat_train_common.h's own example)."""
    n_cu, L, SQ = 256, 33, 5
    B = 13 * n_cu
    assert chunk_plan(13, SQ, L, BWD_NW) == -3
    gb, gf = launch_grid(B, SQ, n_cu, True), launch_grid(B, SQ, n_cu, False)
    assert (gb, gf) == (n_cu, 2 * n_cu)
    assert [ns for _, ns in workgroup_walk(B, SQ, L, gb, 0, True)] == [5, 5, 3]
    assert [ns for _, ns in workgroup_walk(B, SQ, L, gb, 8, True)] == [3, 5, 5]
    assert workgroup_walk(B, SQ, L, gb, 8, True)[0] == (8 * 13 + 10, 3)
    for w in (0, 1, 8, 511):
        walk = workgroup_walk(B, SQ, L, gf, w, False)
        assert len(walk) == 2 and sum(ns for _, ns in walk) in (6, 7) and walk[0][0] == B * w // gf
    m = chunk_map(B, SQ, L, gb, True)
    assert m[0] == (0, 0, 3, 5) and m[12] == (0, 2, 3, 3) and m[8 * 13] == (8, 2, 3, 5) and m[B - 1][0] == n_cu - 1
    # 5 n_CU + 7 sequences: most workgroups one full chunk, seven of them six sequences in two chunks
    B = 5 * n_cu + 7
    walks = [workgroup_walk(B, SQ, L, launch_grid(B, SQ, n_cu, True), w, True) for w in range(n_cu)]
    assert sum(len(x) == 2 for x in walks) == 7 and sum(len(x) == 1 for x in walks) == n_cu - 7
    assert "seq 12: fwd wg 1 chunk 2/2" in describe_sequences([12], 13 * n_cu, SQ, L, n_cu)
