"""GPU: several query tokens per call over frozen and shared segments -- mustafar_decode_shared_segment_multi, mustafar_decode_multi_segment,
SharedSegment.decode_multi, decode_segment_multi and MustafarAttention.decode_multi_split.

Comparators are the suite's own: the float64 models of tests/exact_data.py and tests/partial_util.py with their derived bounds (ratio <= 1),
the split bound of tests/shared_util.py, needles that are exact, and the existing entry points bit for bit.  kv heads <= 2, T <= 1024."""
import numpy as np
import pytest
import torch

from tests import exact_data as xd
from tests import multi_split_util as mu
from tests import partial_util as pu
from tests import shared_util as su
from tests.hd64_util import DEV, NEG, S, oracle_prune
from tests.multi_split_util import bits
from tests.test_gpu_multi_query import _attn, _grow, needle_data, needle_want
from tests.test_gpu_shared_segment import SPLIT_KINDS, _shared_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    from mustafar_amd import _lib, compression
    return _lib.load(), compression


def _hook(Dd, Hq, Hkv, **kw):
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    return MustafarAttention(MustafarConfig(num_attention_heads=Hq, num_key_value_heads=Hkv, head_dim=Dd, k_sparsity=S, v_sparsity=S,
                                            api="fused", **kw))


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV).half()


# ---- 1. the shared form, C level -----------------------------------------------------------------------------------------------------------
#   (n_seqs, groups, n_q): R = 8; G' = 12, beyond the old limit of 8; groups 1; R = 64 exactly; R = 80, a last chunk of 16 rows; R = 84, a
#   sequence's rows straddle the chunk boundary; R = 128, two full chunks; R = 1024
SHARED = [(1, 4, 2), (2, 4, 3), (3, 1, 5), (2, 8, 4), (5, 4, 4), (7, 4, 3), (2, 8, 8), (32, 8, 4)]
T_RUNS = 704   # 11 blocks: at every R of the list but 8 a run holds several blocks and the last run is shorter


@pytest.mark.parametrize("n,groups,n_q", SHARED)
@pytest.mark.parametrize("T", [128, T_RUNS])
@pytest.mark.parametrize("Dd", [64, 128])
def test_shared_form_against_the_models_and_on_needles(pkg, Dd, T, n, groups, n_q):
    Hkv, R = 2, n * groups * n_q
    K, V = _randn((1, Hkv, T, Dd), T + Dd + R), _randn((1, Hkv, T, Dd), T + Dd + R + 1)
    q = _randn((n, Hkv * groups, n_q, Dd), R)
    Kp, Vp = oracle_prune(K, S), oracle_prune(V, S)
    c = mu.SharedMultiCall(pkg, Kp, Vp, groups, n, n_q)
    slabs, bpw, last = c.run_shape()
    rule = -(-8 * min(R, 64) * (Dd + 2) // (88 * Dd))     # blocks per run: the rule of DESIGN.md 4.10 at min(R, 64) rows
    assert slabs == -(-(T // 64) // rule)
    if T == T_RUNS:
        assert slabs >= 2 and (R == 8 or (rule >= 2 and (T // 64) % rule))
    out, lse = c.call(q)
    mu.assert_segment_models(out, lse, q, Kp, Vp, groups, f"shared D={Dd} T={T} R={R} ({slabs} runs of {bpw}, last {last})")
    if R > 64:
        return
    # needles, wherever tests/shared_util.py has a slot for every row: G' = groups * n_q q heads per kv head, one token each
    Gq = groups * n_q
    rng = np.random.default_rng(Dd + T + R)
    for i, pos in enumerate(su.assign_rows(su.edge_positions(T), n, Hkv * Gq, rng, T)[:2]):
        K, V, q1, w = su.needle_data(Dd, n, Gq, Hkv, T, pos, seed=Dd + T + i)
        K, V, q1 = K.to(DEV), V.to(DEV), q1.to(DEV)
        c = mu.SharedMultiCall(pkg, oracle_prune(K, S), oracle_prune(V, S), groups, n, n_q)
        out, lse = c.call(q1.view(n, Hkv * groups, n_q, Dd))
        miss = xd.needle_misses(mu.as_one_token(out), su.needle_expect(V, pos, Gq))
        assert not miss.any(), f"call {i}: rows {miss.nonzero().tolist()} differ from their needle's V row"
        assert torch.equal(lse, torch.full_like(lse, su.needle_x(Dd, w))), f"call {i}: an LSE is not the needle's x"


@pytest.mark.parametrize("Dd", [64, 128])
def test_shared_form_bit_equality(pkg, Dd):
    Hkv, T = 2, T_RUNS
    Kp, Vp = oracle_prune(_randn((1, Hkv, T, Dd), Dd), S), oracle_prune(_randn((1, Hkv, T, Dd), Dd + 1), S)
    # n_q = 1 is mustafar_decode_shared_segment; (n, 2, 4) is that call with groups = 8 on the same memory
    for n, groups, n_q in [(5, 4, 1), (16, 4, 1), (3, 2, 4), (8, 2, 4)]:
        q = _randn((n, Hkv * groups, n_q, Dd), n + n_q)
        out, lse = mu.SharedMultiCall(pkg, Kp, Vp, groups, n, n_q).call(q)
        old, old_lse = su.SharedCall(pkg, Kp, Vp, groups * n_q, n).call(q)
        assert torch.equal(bits(out).reshape(-1), bits(old).reshape(-1)) and torch.equal(bits(lse).reshape(-1), bits(old_lse).reshape(-1)), \
            f"({n}, {groups}, {n_q}) differs from mustafar_decode_shared_segment"
    # R = 128 in one call against two 64-row calls of the same entry point on its halves
    n, groups, n_q = 2, 8, 8
    q = _randn((n, Hkv * groups, n_q, Dd), 128)
    whole, whole_lse = mu.SharedMultiCall(pkg, Kp, Vp, groups, n, n_q).call(q)
    half = mu.SharedMultiCall(pkg, Kp, Vp, groups, n, n_q)
    half.ws = torch.empty((pkg[0].mustafar_shared_segment_multi_workspace_bytes(T, Hkv, groups, 1, n_q, Dd),), dtype=torch.uint8, device=DEV)
    half.call(q, rows=(0, 1))
    half.call(q, rows=(1, 2))
    assert torch.equal(bits(whole), bits(half.out)) and torch.equal(bits(whole_lse), bits(half.lse))


# ---- 2. the per-sequence form, C level -------------------------------------------------------------------------------------------------------
def _masks(B, n_q, T, seed):
    """{name: mask [B, 1, 1 or n_q, T]}, each an odd-offset column slice of a wider tensor: finite values that are fp16 numbers, the left
    padding of sequence 1 at finfo.min, and (rows: n_q) query token 1 of sequence 0 masked entirely."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = {}
    for rows in sorted({1, n_q}):
        wide = torch.randint(-8, 1, (B, 1, rows, T + 8), generator=g, device=DEV).half() * 0.25
        m = wide[..., 5:5 + T]
        m[1, :, :, :37] = NEG
        if rows > 1:
            m[0, :, 1, :] = NEG
        assert m.data_ptr() % 4 == 2 and m.stride(3) == 1
        out["one row" if rows == 1 else "a row per token"] = m
    return out


SEG_ROWS = [2, 12, 16, 20, 64]   # n_q at GQA-4: R = 8, 48, 64, 80 (a last chunk of 16 rows), 256


@pytest.mark.parametrize("n_q", SEG_ROWS)
@pytest.mark.parametrize("Dd", [64, 128])
def test_per_sequence_form_over_one_view(pkg, Dd, n_q):
    """T = 192, B' = 2 x 2 heads: without a mask, with one mask row, with a row per token; needles on the cut and on the block edges."""
    B, Hkv, groups, T = 2, 2, 4, 192
    K, V = _randn((B, Hkv, T, Dd), Dd + n_q), _randn((B, Hkv, T, Dd), Dd + n_q + 1)
    q = _randn((B, Hkv * groups, n_q, Dd), n_q)
    Kp, Vp = oracle_prune(K, S), oracle_prune(V, S)
    c = mu.SegmentMultiCall(pkg, B, Hkv, T, Dd, groups, n_q, Kp, Vp)
    out, lse = c.call(q)
    mu.assert_segment_models(out, lse, q, Kp, Vp, groups, f"segment D={Dd} R={n_q * groups} runs {c.run_shape()}")
    for name, m in _masks(B, n_q, T, n_q).items():
        c.out.fill_(mu.NAN)
        c.lse.fill_(mu.NAN)
        out, lse = c.call(q, m)
        mu.assert_segment_models(out, lse, q, Kp, Vp, groups, f"segment D={Dd} R={n_q * groups} mask: {name}", mask=m)
    if n_q * groups > 64:
        return
    # needles: the B' heads as the kv heads of one sequence at G' = groups * n_q (tests/shared_util.py), every row its own token
    Gq, heads = groups * n_q, B * Hkv
    pos = su.assign_rows(su.edge_positions(T), 1, heads * Gq, np.random.default_rng(Dd + n_q), T)[0]
    K, V, q1, w = su.needle_data(Dd, 1, Gq, heads, T, pos, seed=Dd + n_q)
    K, V, q1 = K.to(DEV), V.to(DEV), q1.to(DEV)
    c = mu.SegmentMultiCall(pkg, B, Hkv, T, Dd, groups, n_q, oracle_prune(K, S).view(B, Hkv, T, Dd), oracle_prune(V, S).view(B, Hkv, T, Dd))
    out, lse = c.call(q1.view(B, Hkv * groups, n_q, Dd))
    miss = xd.needle_misses(out.view(1, heads * Gq, 1, Dd), su.needle_expect(V, pos, Gq))
    assert not miss.any(), f"rows {miss.nonzero().tolist()} differ from their needle's V row"
    assert torch.equal(lse, torch.full_like(lse, su.needle_x(Dd, w))), "an LSE is not the needle's x"


@pytest.mark.parametrize("n_q", [2, 16, 20])
@pytest.mark.parametrize("extents", [1, 2])
@pytest.mark.parametrize("kind", ["arena", "ext64"])
def test_per_sequence_form_over_extents(pkg, kind, extents, n_q):
    """A base of 256 tokens plus one and two 256-token extents read through the device tables (an arena at D = 128, an ExtentCache64 at
    D = 64), B' = 1 x 2 heads: R = 8 runs block by block; R = 64 and 80 run six blocks at a time, so run 0 crosses base -> extent (and run
    1 extent -> extent).  Random data against the models with and without a mask; needles on the seams."""
    B, Hkv, groups = 1, 2, 4
    attn = _attn(kind)
    Dd, T = attn.head_dim, 256 * (extents + 1)
    total = T + 32
    K, V = _randn((B, Hkv, total, Dd), extents + Dd), _randn((B, Hkv, total, Dd), extents + Dd + 1)
    q = _randn((B, Hkv * groups, n_q, Dd), n_q)
    past, _ = _grow(attn, K, V, q[:, :, :1].contiguous(), extents)
    assert past[4] == T and len(past[0].extents) == extents and past[0].tokens == 256
    views, keep = past[0].view_args(past[2], tables=True)
    c = mu.SegmentMultiCall(pkg, B, Hkv, T, Dd, groups, n_q, views=views)
    rule = -(-8 * min(n_q * groups, 64) * (Dd + 2) // (88 * Dd))
    assert rule == (1 if n_q == 2 else 6) and c.run_shape()[0] == -(-(T // 64) // rule)   # 6 blocks: run 0 holds blocks 3 and 4, either
    #                                                                                       side of the base's end; run 1 blocks 7 and 8
    Kp, Vp = oracle_prune(K[:, :, :T], S), oracle_prune(V[:, :, :T], S)
    out, lse = c.call(q)
    mu.assert_segment_models(out, lse, q, Kp, Vp, groups, f"{kind} {extents} extents R={n_q * groups}")
    m = _masks(B + 1, n_q, T, n_q)["a row per token"][1:]   # (the left-padded sequence)
    c.out.fill_(mu.NAN)
    out, lse = c.call(q, m)
    mu.assert_segment_models(out, lse, q, Kp, Vp, groups, f"{kind} {extents} extents R={n_q * groups}, masked", mask=m)
    # through the hook: the same bits
    out2, lse2 = attn.decode_segment_multi(q, past[0], past[2], T, m)
    assert torch.equal(bits(out2), bits(out)) and torch.equal(bits(lse2), bits(lse))
    if n_q * groups > 64:
        return
    edges = [t for e in range(extents + 1) for t in (256 * e, 256 * e + 255)]
    pos = np.zeros((B, Hkv * groups, n_q), np.int64)
    for i, idx in enumerate(np.ndindex(B, Hkv * groups, n_q)):
        pos[idx] = edges[i % len(edges)]
    K, V, q, w = needle_data(Dd, B, Hkv, groups, n_q, total, pos, T, seed=7 + extents)
    past, _ = _grow(attn, K, V, q[:, :, :1].contiguous(), extents)
    out, lse = attn.decode_segment_multi(q, past[0], past[2], T)
    miss = (out.float() != needle_want(V, pos, T, groups).float()).any(-1)
    assert not miss.any(), f"rows {miss.nonzero().tolist()} differ from their needle's V row"
    assert torch.equal(lse, torch.full_like(lse, su.needle_x(Dd, w))), "an LSE is not the needle's x"
    del keep


# ---- 3. decode_multi_split ------------------------------------------------------------------------------------------------------------------
F_SHARED, LIVE_C, LIVE_W = 512, 256, 40


def _split_setup(attn, kind, K, V, F=F_SHARED, live=LIVE_C + LIVE_W):
    """K / V [B, Hkv, F + live + n_q, D] whose first F rows are the same for every sequence -> (the shared segment over them, the live past
    over rows [F, F + live), the rows as the caches hold them: the first F + compressed-length rows pruned)."""
    C_all = F + max(0, (live - attn.cfg.residual_length) // 256 * 256)
    Kp, Vp = pu.pruned_rows(K, V, C_all)
    seg = _shared_of(kind, Kp[:1, :, :F], Vp[:1, :, :F])
    past = attn.to_fused(attn.build_cache(K[:, :, F:F + live].contiguous(), V[:, :, F:F + live].contiguous()))
    assert past[4] == C_all - F
    return seg, past, Kp, Vp


def _split_ratio(out, q, Kp, Vp, groups, cuts, first, mask=None, shift=0):
    """max over the query tokens of |split - model of the whole| / split bound (tests/shared_util.py): token j sees rows [0, first + j + 1)
    of Kp / Vp, the parts being the row ranges between `cuts` (the last one open: it ends where the token's sight ends).  mask
    [B, 1, 1 or n_q, >= first + n_q]: additive, the row of token j.  shift: token j is given the columns of token j + shift (the
    negative control)."""
    worst = 0.0
    for j in range(q.shape[2]):
        Lj = min(first + j + 1 + shift, Kp.shape[2])
        qj = q[:, :, j:j + 1]
        mj = None if mask is None else (mask if mask.shape[2] == 1 else mask[:, :, j:j + 1])[..., :Lj]
        want, bound = xd.hook_model(qj, Kp[:, :, :Lj], Vp[:, :, :Lj], groups, mask=mj)
        lse_all, _ = pu.lse_model(qj, Kp[:, :, :Lj], groups, mask=mj)
        parts, lse_bounds = [], []
        for a, b in zip(cuts, list(cuts[1:]) + [Lj]):
            mp = None if mj is None else mj[..., a:b]
            o_i, _ = xd.hook_model(qj, Kp[:, :, a:b], Vp[:, :, a:b], groups, mask=mp)
            l_i, bl_i = pu.lse_model(qj, Kp[:, :, a:b], groups, mask=mp)
            parts.append((o_i, torch.exp(l_i - lse_all)))
            lse_bounds.append(bl_i)
        r = (out[:, :, j:j + 1].double() - want).abs() / su.split_bound(parts, lse_bounds, want, bound)
        worst = max(worst, float(r.max()) if torch.isfinite(r).all() else float("inf"))
    return worst


def _shared_prefix(K, V, F):
    K[1:, :, :F], V[1:, :, :F] = K[:1, :, :F], V[:1, :, :F]


@pytest.mark.parametrize("Dd,kind,live_kw", SPLIT_KINDS)
def test_decode_multi_split_on_needles_and_random_data(pkg, Dd, kind, live_kw):
    """A shared prefix of 512 tokens + live caches of 256 compressed and 40 window rows, batch 2, three new tokens."""
    B, Hkv, groups, n_q = 2, 2, 4, 3
    Hq, F = Hkv * groups, F_SHARED
    L0 = F + LIVE_C + LIVE_W
    attn = _hook(Dd, Hq, Hkv, **live_kw)
    # needles: per row in the shared part (the same token for both sequences: there is one copy), in the live compressed part, in the
    # window and among the new rows -- on the cut and on the seams; token j's latest is its own row
    spots = [0, F - 1, 64, 319, F, F + 255, F + 256, L0 - 1, L0, L0 + 1, L0 + 2]
    pos = np.zeros((B, Hq, n_q), np.int64)
    for i, (b, h, j) in enumerate(np.ndindex(B, Hq, n_q)):
        p = spots[(h * n_q + j + (3 * b if h >= 4 else 0)) % len(spots)]
        pos[b, h, j] = p if p <= L0 + j else L0 + j
    assert (pos[0, :4] == pos[1, :4]).all() and (pos[:, :4] < F).any() and (pos >= L0).any() and ((pos >= F) & (pos < F + 256)).any()
    pos[1][pos[0] < F] = pos[0][pos[0] < F]          # a needle in the shared part sits where sequence 0's does
    pos[0][pos[1] < F] = pos[1][pos[1] < F]
    K, V, q, w = needle_data(Dd, B, Hkv, groups, n_q, L0 + n_q, pos, F + LIVE_C, seed=5)
    _shared_prefix(K, V, F)
    seg, past, _, _ = _split_setup(attn, kind, K, V)
    out, lse, _ = attn.decode_multi_split(q, K[:, :, L0:], V[:, :, L0:], past, [seg], return_lse=True)
    miss = (out.float() != needle_want(V, pos, F + LIVE_C, groups).float()).any(-1)
    assert not miss.any(), f"rows {miss.nonzero().tolist()} differ from the whole"
    assert torch.equal(lse, torch.full_like(lse, su.needle_x(Dd, w))), "a merged LSE is not the needle's x"

    # random data: per token against the model of the whole, with the split bound of DESIGN.md 4.9
    K, V = _randn((B, Hkv, L0 + n_q, Dd), Dd), _randn((B, Hkv, L0 + n_q, Dd), Dd + 1)
    q = _randn((B, Hq, n_q, Dd), Dd + 2)
    _shared_prefix(K, V, F)
    seg, past, Kp, Vp = _split_setup(attn, kind, K, V)
    out, new = attn.decode_multi_split(q, K[:, :, L0:], V[:, :, L0:], past, [seg])
    r = _split_ratio(out, q, Kp, Vp, groups, (0, F), L0)
    print(f"multi split D={Dd} {kind}: |split - whole model| / bound = {r:.3f}")
    assert r <= 1.0
    # the comparator can fail: without the frozen entry, and with token j given the columns of token j + 1
    _, past2, _, _ = _split_setup(attn, kind, K, V)
    alone, _ = attn.decode_multi(q, K[:, :, L0:], V[:, :, L0:], past2)
    r_alone = _split_ratio(alone, q, Kp, Vp, groups, (0, F), L0)
    r_shift = _split_ratio(out, q, Kp, Vp, groups, (0, F), L0, shift=1)
    print(f"  negative controls: frozen entry dropped {r_alone:.1f}, columns of the next token {r_shift:.1f}")
    assert r_alone > 1.0 and r_shift > 1.0

    # the returned past is what decode_multi returns for the live cache alone, window bits included
    twin = attn.to_fused(attn.build_cache(K[:, :, F:L0].contiguous(), V[:, :, F:L0].contiguous()))
    _, ref = attn.decode_multi(q, K[:, :, L0:], V[:, :, L0:], twin)
    assert len(new) == 6 and new[4:] == ref[4:] == (LIVE_C, L0 - F + n_q) and type(new[0]) is type(ref[0]) and type(new[2]) is type(ref[2])
    for i in (1, 3):
        assert new[i].len == ref[i].len == LIVE_W + n_q and new[i].cap == ref[i].cap
        assert torch.equal(bits(new[i].view()), bits(ref[i].view()))
    # accept(rejected=1), then a further call over what stayed
    new = attn.accept(new, rejected=1)
    assert new[5] == L0 - F + n_q - 1 and new[1].len == LIVE_W + n_q - 1
    L1 = L0 + n_q - 1
    K2 = torch.cat([K[:, :, :L1], _randn((B, Hkv, 2, Dd), 40)], dim=2)
    V2 = torch.cat([V[:, :, :L1], _randn((B, Hkv, 2, Dd), 41)], dim=2)
    q2 = _randn((B, Hq, 2, Dd), 42)
    out2, new = attn.decode_multi_split(q2, K2[:, :, L1:], V2[:, :, L1:], new, [seg])
    Kp2, Vp2 = pu.pruned_rows(K2, V2, F + LIVE_C)
    r = _split_ratio(out2, q2, Kp2, Vp2, groups, (0, F), L1)
    print(f"  after accept(rejected=1): {r:.3f}")
    assert r <= 1.0 and new[5] == L1 - F + 2


@pytest.mark.parametrize("Dd", [64, 128])
def test_mixed_frozen_entries_with_a_mask_that_pads_the_per_sequence_one(pkg, Dd):
    """frozen = [a shared entry of 128 tokens, a per-sequence entry of 192], live 256 + 40, three new tokens.  The mask pads the first 70
    columns of sequence 1's per-sequence entry; the columns of the shared entry hold finfo.min and are never read."""
    B, Hkv, groups, n_q = 2, 2, 4, 3
    Hq, F, P = Hkv * groups, 128, 192
    L0 = F + P + LIVE_C + LIVE_W
    attn = _hook(Dd, Hq, Hkv)
    K, V = _randn((B, Hkv, L0 + n_q, Dd), Dd + 3), _randn((B, Hkv, L0 + n_q, Dd), Dd + 4)
    q = _randn((B, Hq, n_q, Dd), Dd + 5)
    _shared_prefix(K, V, F)
    _, _, Kp, Vp = _split_setup(attn, "tuple", K, V, F=F + P)   # (the live past over the rows behind BOTH frozen entries)
    from mustafar_amd.hook import _compress
    seg = _shared_of("tuple", Kp[:1, :, :F], Vp[:1, :, :F])
    kc = _compress(Kp[:, :, F:F + P].reshape(B * Hkv, P, Dd).contiguous(), "key")
    vc = _compress(Vp[:, :, F:F + P].reshape(B * Hkv, P, Dd).contiguous(), "value")
    for rows in (1, n_q):
        mask = torch.zeros((B, 1, rows, L0 + n_q), dtype=torch.float16, device=DEV)
        mask[1, :, :, F:F + 70] = NEG
        model_mask = mask.clone()
        mask[:, :, :, :F] = NEG                       # the shared entry's columns: whatever they hold, nobody reads them
        _, p, _, _ = _split_setup(attn, "tuple", K, V, F=F + P)
        out, _ = attn.decode_multi_split(q, K[:, :, L0:], V[:, :, L0:], p, [seg, (kc, vc, P)], attention_mask=mask)
        r = _split_ratio(out, q, Kp, Vp, groups, (0, F, F + P), L0, mask=model_mask)
        print(f"mixed frozen D={Dd}, {rows} mask rows: |split - whole model| / bound = {r:.3f}")
        assert r <= 1.0


@pytest.mark.parametrize("Dd,kind,live_kw", SPLIT_KINDS)
def test_a_call_whose_last_row_is_the_trigger_point(pkg, Dd, kind, live_kw):
    """Live cache: 256 compressed + 285 window rows; three new tokens bring the window to 288 = 32 + 256: accept() runs the trigger."""
    B, Hkv, groups, n_q, F = 1, 2, 4, 3, 256
    live = 256 + 285
    attn = _hook(Dd, Hkv * groups, Hkv, **live_kw)
    L0 = F + live
    K, V = _randn((B, Hkv, L0 + n_q, Dd), Dd + 6), _randn((B, Hkv, L0 + n_q, Dd), Dd + 7)
    q = _randn((B, Hkv * groups, n_q, Dd), Dd + 8)
    seg, past, Kp, Vp = _split_setup(attn, kind, K, V, F=F, live=live)
    with pytest.raises(ValueError, match="at most 3 fit"):
        attn.decode_multi_split(_randn((B, Hkv * groups, 4, Dd), 1), _randn((B, Hkv, 4, Dd), 2), _randn((B, Hkv, 4, Dd), 3), past, [seg])
    out, new = attn.decode_multi_split(q, K[:, :, L0:], V[:, :, L0:], past, [seg])
    assert _split_ratio(out, q, Kp, Vp, groups, (0, F), L0) <= 1.0
    assert new[4] == 256 and new[1].len == 288 and attn.trigger_due(new)
    new = attn.accept(new)
    assert new[4] == 512 and new[1].len == new[3].len == 32 and new[5] == live + n_q
    # the next call reads the 512 compressed tokens
    L1 = L0 + n_q
    K2, V2 = torch.cat([K, _randn((B, Hkv, 2, Dd), 9)], dim=2), torch.cat([V, _randn((B, Hkv, 2, Dd), 10)], dim=2)
    q2 = _randn((B, Hkv * groups, 2, Dd), 11)
    out2, _ = attn.decode_multi_split(q2, K2[:, :, L1:], V2[:, :, L1:], new, [seg])
    Kp2, Vp2 = pu.pruned_rows(K2, V2, F + 512)
    r = _split_ratio(out2, q2, Kp2, Vp2, groups, (0, F), L1)
    print(f"after the trigger D={Dd} {kind}: {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("Dd", [64, 128])
def test_a_draft_tree_next_to_a_shared_prefix(pkg, Dd):
    """Four drafted tokens: 0 the root, 1 and 2 its children, 3 the child of 2.  Each sees the shared prefix, the live cache, its ancestors
    and itself; accept(keep=) keeps the path 0 -> 2 -> 3."""
    B, Hkv, groups, n_q, F = 2, 2, 4, 4, 256
    Hq = Hkv * groups
    L0 = F + LIVE_C + LIVE_W
    attn = _hook(Dd, Hq, Hkv)
    K, V = _randn((B, Hkv, L0 + n_q, Dd), Dd + 12), _randn((B, Hkv, L0 + n_q, Dd), Dd + 13)
    q = _randn((B, Hq, n_q, Dd), Dd + 14)
    _shared_prefix(K, V, F)
    seg, past, Kp, Vp = _split_setup(attn, "tuple", K, V, F=F)
    sees = {0: [0], 1: [0, 1], 2: [0, 2], 3: [0, 2, 3]}
    mask = torch.zeros((B, 1, n_q, L0 + n_q), dtype=torch.float16, device=DEV)
    mask[:, :, :, L0:] = NEG
    for j, anc in sees.items():
        mask[:, :, j, [L0 + a for a in anc]] = 0.0
    out, new = attn.decode_multi_split(q, K[:, :, L0:], V[:, :, L0:], past, [seg], attention_mask=mask)
    # the model: every new row is in sight of every token, the mask takes away what the tree (and the causal limit) hides
    r = _split_ratio(out, q, Kp, Vp, groups, (0, F), L0, mask=mask, shift=n_q)
    print(f"draft tree D={Dd}: |split - whole model| / bound = {r:.3f}")
    assert r <= 1.0
    assert _split_ratio(out, q, Kp, Vp, groups, (0, F), L0) > 1.0      # the plain causal model does not fit: the tree was applied
    path = torch.tensor([[0, 2, 3]] * B, device=DEV)
    new = attn.accept(new, keep=path, n_q=n_q)
    assert new[1].len == LIVE_W + 3 and new[5] == L0 - F + 3
    for win, X in ((new[1], K), (new[3], V)):
        assert torch.equal(bits(win.view()[:, :, LIVE_W:]), bits(X[:, :, [L0, L0 + 2, L0 + 3]]))


# ---- 4. SharedSegment.decode_multi ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dd", [64, 128])
def test_shared_segment_decode_multi(pkg, Dd):
    """bsz 20 at GQA-4 with four tokens: 320 rows per kv head, five chunks, ONE call; n_q = 1 is SharedSegment.decode bit for bit."""
    from mustafar_amd import partial
    bsz, Hkv, groups, n_q, T = 20, 2, 4, 4, 320
    attn = _hook(Dd, Hkv * groups, Hkv)
    K, V = _randn((1, Hkv, T, Dd), Dd + 15), _randn((1, Hkv, T, Dd), Dd + 16)
    q = _randn((bsz, Hkv * groups, n_q, Dd), Dd + 17)
    seg = partial.SharedSegment.from_dense(attn, K, V)
    out, lse = seg.decode_multi(attn, q)
    assert out.shape == (bsz, Hkv * groups, n_q, Dd) and lse.shape == (bsz, Hkv * groups, n_q)
    Kp, Vp = oracle_prune(K, S), oracle_prune(V, S)
    mu.assert_segment_models(out, lse, q, Kp, Vp, groups, f"SharedSegment.decode_multi D={Dd} bsz 20")
    out2, lse2 = partial.decode_segment_multi(attn, q.transpose(0, 1).contiguous().transpose(0, 1), seg)   # a query that is not contiguous
    assert torch.equal(bits(out2), bits(out)) and torch.equal(bits(lse2), bits(lse))
    # more than 1024 rows per kv head: consecutive calls over whole sequences (70 x 16 rows: 64 + 6 sequences)
    big = _randn((70, Hkv * groups, n_q, Dd), Dd + 18)
    ob, lb = seg.decode_multi(attn, big)
    mu.assert_segment_models(ob, lb, big, Kp, Vp, groups, f"SharedSegment.decode_multi D={Dd} bsz 70")
    for n in (5, 16):
        q1 = q[:n, :, :1].contiguous()
        a, al = seg.decode_multi(attn, q1)
        b, bl = seg.decode(attn, q1)
        assert a.shape == b.shape and al.shape == (n, Hkv * groups, 1)
        assert torch.equal(bits(a), bits(b)) and torch.equal(bits(al).reshape(-1), bits(bl).reshape(-1))


# ---- 5. graph -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dd", [64, 128])
def test_one_graph_of_a_decode_multi_split_replays_bit_for_bit(pkg, Dd):
    """Shared prefix + live cache at fixed lengths: the captured call appends the same rows at the same place on every replay."""
    B, Hkv, groups, n_q, F = 2, 2, 4, 3, 256
    Hq = Hkv * groups
    L0 = F + LIVE_C + LIVE_W
    attn = _hook(Dd, Hq, Hkv)
    K, V = _randn((B, Hkv, L0 + n_q, Dd), Dd + 19), _randn((B, Hkv, L0 + n_q, Dd), Dd + 20)
    _shared_prefix(K, V, F)
    qs = _randn((3, B, Hq, n_q, Dd), Dd + 21)
    kn, vn = K[:, :, L0:].contiguous(), V[:, :, L0:].contiguous()
    seg, past, _, _ = _split_setup(attn, "tuple", K, V, F=F)
    eager = []
    for i in range(3):
        past[1].len = past[3].len = LIVE_W           # (the host lengths of the first call: every call appends at the same rows)
        o, l, _ = attn.decode_multi_split(qs[i], kn, vn, past._replace(kv_seq_len=L0 - F), [seg], return_lse=True)
        eager.append((o.clone(), l.clone()))
    past[1].len = past[3].len = LIVE_W
    q_in = qs[0].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse, _ = attn.decode_multi_split(q_in, kn, vn, past._replace(kv_seq_len=L0 - F), [seg], return_lse=True)
    for i in (1, 2, 0):
        q_in.copy_(qs[i])
        out.fill_(mu.NAN)
        lse.fill_(mu.NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(eager[i][0])) and torch.equal(bits(lse), bits(eager[i][1])), f"replay of query {i}"
