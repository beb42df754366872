"""GPU: one compressed copy of a shared segment decoded for a whole batch (ABI 111: mustafar_decode_shared_segment, partial.SharedSegment,
decode_split with shared entries).

Exact on needles whose slots are narrow enough for every row of a kv head (tests/shared_util.py), against the float64 models of
tests/exact_data.py and tests/partial_util.py with their derived bounds on random data.  kv heads <= 2 everywhere."""
import numpy as np
import pytest
import torch

from tests import exact_data as xd
from tests import partial_util as pu
from tests import shared_util as su
from tests.hd64_util import DEV, S, needle_data_64, needle_expect_64, oracle_prune

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    from mustafar_amd import _lib, compression
    return _lib.load(), compression


def _hook(Dd, Hq, Hkv, ks=S, vs=S, **kw):
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    return MustafarAttention(MustafarConfig(num_attention_heads=Hq, num_key_value_heads=Hkv, head_dim=Dd, k_sparsity=ks, v_sparsity=vs,
                                            api="fused", **kw))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _rand(n, Hkv, T, groups, Dd, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    K = torch.randn((1, Hkv, T, Dd), generator=g, device=DEV).half()
    V = torch.randn((1, Hkv, T, Dd), generator=g, device=DEV).half()
    q = torch.randn((n, Hkv * groups, 1, Dd), generator=g, device=DEV).half()
    return K, V, q


def _assert_models(out, lse, q, Kp, Vp, groups, what):
    """|out - hook_model| / bound <= 1 and |lse - lse_model| / bound <= 1, the one copy expanded over the sequences (a view)."""
    n = q.shape[0]
    Ke, Ve = Kp.expand(n, -1, -1, -1), Vp.expand(n, -1, -1, -1)
    want, bound = xd.hook_model(q, Ke, Ve, groups)
    r_out = float(((out.double() - want).abs() / bound).max())
    want_l, bound_l = pu.lse_model(q, Ke, groups)
    r_lse = pu.lse_ratio(lse, want_l, bound_l)
    print(f"{what}: |out - model| / bound = {r_out:.3f}, |lse - model| / bound = {r_lse:.3f}")
    assert r_out <= 1.0 and r_lse <= 1.0, f"{what}: out {r_out:.3f}, lse {r_lse:.3f}"


# ---- 1. exact, on needles ---------------------------------------------------------------------------------------------------------------
# R = 35, 48 and 33: three row tiles (wave 3 idles in the softmax step) -- padded rows, a tile exactly full, one row into the tile
RT3 = [(5, 7), (12, 4), (11, 3)]


@pytest.mark.parametrize("n,groups", [(1, 4), (3, 3), (4, 4), (8, 4), (16, 4), (8, 8)] + RT3)
@pytest.mark.parametrize("T", [64, 576])
@pytest.mark.parametrize("Dd", [64, 128])
def test_exact_on_needles(pkg, Dd, T, n, groups):
    """Needles on token 0, the first and last token of every block and T - 1, spread over the rows: every row's output is its needle's
    pruned V row as values, every row's LSE its needle's x exactly."""
    Hkv = 2
    H = Hkv * groups
    rng = np.random.default_rng(Dd + T + n * groups)
    for i, pos in enumerate(su.assign_rows(su.edge_positions(T), n, H, rng, T)):
        K, V, q, w = su.needle_data(Dd, n, groups, Hkv, T, pos, seed=Dd + T + i)
        K, V, q = K.to(DEV), V.to(DEV), q.to(DEV)
        out, lse = su.SharedCall(pkg, oracle_prune(K, S), oracle_prune(V, S), groups, n).call(q)
        miss = xd.needle_misses(out, su.needle_expect(V, pos, groups))
        assert not miss.any(), f"call {i}: rows {miss.nonzero().tolist()} differ from their needle's V row"
        assert torch.equal(lse, torch.full_like(lse, su.needle_x(Dd, w))), f"call {i}: an LSE is not the needle's x"


@pytest.mark.parametrize("Dd", [64, 128])
def test_needles_beyond_the_64th_slab(pkg, Dd):
    """R = 8 is one block per run: 4608 tokens are 72 slabs, more than the 64 lanes of the merge's max loop.  On random data (shape c) the
    fold is the same sum under any maximum that does not overflow; here every row's needle, of twice the level, sits in slabs 64 .. 71
    and its x stands more than 88 above everything in the first 64: a maximum taken over those alone makes exp() overflow."""
    n, groups, Hkv, T = 2, 4, 2, 4608
    assert su.run_shape(pkg[0], T, Hkv, groups, n, Dd) == (72, 1, 1)
    late = [t for b in range(64, 72) for t in (64 * b, 64 * b + 63)]
    pos = np.asarray([late[i % len(late)] for i in range(n * Hkv * groups)], np.int64).reshape(n, Hkv * groups)
    K, V, q, w = su.needle_data(Dd, n, groups, Hkv, T, pos, seed=Dd + 9, boost=2)
    assert su.needle_x(Dd, w, 2) - su.other_x_max(Dd, w) > 88.8   # (exp(88.73) is the first fp32 infinity)
    K, V, q = K.to(DEV), V.to(DEV), q.to(DEV)
    out, lse = su.SharedCall(pkg, oracle_prune(K, S), oracle_prune(V, S), groups, n).call(q)
    miss = xd.needle_misses(out, su.needle_expect(V, pos, groups))
    assert not miss.any(), f"rows {miss.nonzero().tolist()} differ from their needle's V row"
    assert torch.equal(lse, torch.full_like(lse, su.needle_x(Dd, w, 2))), "an LSE is not the needle's x"


# ---- 2. random data against the models ----------------------------------------------------------------------------------------------------
def _t_for(L_, shape, Hkv, groups, n, Dd):
    """T of a run shape, with the (slabs, blocks per run, blocks of the last run) it must give.  The rule gives one block per run up to
    R = 10, so at R = 4 shapes b and c are more one-block runs."""
    R = n * groups
    want = -(-8 * R * (Dd + 2) // (88 * Dd))
    if shape == "a":      # one block per workgroup
        T = 192 if want == 1 else 64
        return T, (T // 64, 1, 1)
    if shape == "b":      # at least two blocks per workgroup, a shorter last run
        if want == 1:
            return 320, (5, 1, 1)
        return 64 * (2 * want - 1), (2, want, want - 1)
    ntb = 32512 // 64     # c: the largest run length the rule produces, many runs
    slabs = -(-ntb // want)
    return 32512, (slabs, want, ntb - (slabs - 1) * want)


@pytest.mark.parametrize("ks,vs", [(0.5, 0.7), (0.7, 0.9)])
@pytest.mark.parametrize("n,groups,shape", [(n, groups, shape) for n, groups in [(1, 4), (5, 4), (8, 4), (8, 8)] for shape in "abc"] +
                         [(n, groups, shape) for n, groups in RT3 for shape in "ab"])   # (c is 32512 tokens: not again per row tile)
@pytest.mark.parametrize("Dd", [64, 128])
def test_random_data_against_the_models(pkg, Dd, n, groups, shape, ks, vs):
    Hkv = 1 if shape == "c" else 2
    T, want_shape = _t_for(pkg[0], shape, Hkv, groups, n, Dd)
    assert su.run_shape(pkg[0], T, Hkv, groups, n, Dd) == want_shape
    if shape != "a":
        assert want_shape[1] >= 2 or n * groups <= 10
    K, V, q = _rand(n, Hkv, T, groups, Dd, seed=T + Dd + n * groups)
    Kp, Vp = oracle_prune(K, ks), oracle_prune(V, vs)
    out, lse = su.SharedCall(pkg, Kp, Vp, groups, n).call(q)
    _assert_models(out, lse, q, Kp, Vp, groups, f"D={Dd} R={n * groups} T={T} K{ks}/V{vs}")


# ---- 3. chunking ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dd", [64, 128])
def test_more_than_64_rows_take_one_launch_per_chunk(pkg, Dd):
    """bsz 20 at G = 4: 80 rows per kv head, two launches (16 + 4 sequences) through partial.decode_segment; every row against the model."""
    from mustafar_amd import partial
    bsz, Hkv, groups, T = 20, 2, 4, 128
    attn = _hook(Dd, Hkv * groups, Hkv)
    K, V, q = _rand(bsz, Hkv, T, groups, Dd, seed=Dd)
    seg = partial.SharedSegment.from_dense(attn, K, V)
    out, lse = partial.decode_segment(attn, q, seg)
    assert out.shape == (bsz, Hkv * groups, 1, Dd) and lse.shape == (bsz, Hkv * groups)
    _assert_models(out, lse, q, oracle_prune(K, S), oracle_prune(V, S), groups, f"D={Dd} bsz 20")
    # a query that is not contiguous, and the old signature next to the new one
    out2, lse2 = partial.decode_segment(attn, q.transpose(0, 1).contiguous().transpose(0, 1), seg)
    assert torch.equal(_bits(out2), _bits(out)) and torch.equal(_bits(lse2), _bits(lse))
    from mustafar_amd.hook import _compress
    kc = _compress(oracle_prune(K, S).reshape(Hkv, T, Dd).contiguous(), "key")
    vc = _compress(oracle_prune(V, S).reshape(Hkv, T, Dd).contiguous(), "value")
    out1, lse1 = partial.decode_segment(attn, q[:1], kc, vc, T)
    _assert_models(out1, lse1, q[:1], oracle_prune(K, S), oracle_prune(V, S), groups, f"D={Dd} per-sequence call")


# ---- 4. decode_split ------------------------------------------------------------------------------------------------------------------
def _shared_of(kind, Kp, Vp):
    """The pruned rows [1, Hkv, t, D] of the shared prefix as a SharedSegment over the cache kind asked for."""
    from mustafar_amd import partial
    from mustafar_amd.cache import CompressedArena
    from mustafar_amd.cache64 import ExtentCache64
    from mustafar_amd.hook import _compress
    _, Hkv, t, Dd = Kp.shape
    kc = _compress(Kp.reshape(Hkv, t, Dd).contiguous(), "key")
    vc = _compress(Vp.reshape(Hkv, t, Dd).contiguous(), "value")
    if kind == "arena":
        kc, vc = CompressedArena.from_reference(kc, "key", t), CompressedArena.from_reference(vc, "value", t)
    elif kind == "ext64":
        kc, vc = ExtentCache64(kc, "key", Hkv, t), ExtentCache64(vc, "value", Hkv, t)
    return partial.SharedSegment(kc, vc, t, Hkv)


SPLIT_KINDS = [(64, "tuple", {}), (64, "ext64", {"hd64_extents": True}), (128, "arena", {"arena": True})]


@pytest.mark.parametrize("Dd,kind,live_kw", SPLIT_KINDS)
def test_split_with_a_shared_prefix(pkg, Dd, kind, live_kw):
    """A shared prefix of 512 tokens + per-sequence live caches of 256 compressed rows + 40 window rows, bsz 2."""
    B, Hkv, groups = 2, 2, 4
    Hq = Hkv * groups
    F, n = 512, 512 + 256 + 40 + 1
    C_all = F + 256
    attn = _hook(Dd, Hq, Hkv, **live_kw)

    def run(K, V, q):
        Kp, Vp = pu.pruned_rows(K, V, C_all)
        seg = _shared_of(kind, Kp[:1, :, :F], Vp[:1, :, :F])
        past = attn.to_fused(attn.build_cache(K[:, :, F:n - 1].contiguous(), V[:, :, F:n - 1].contiguous()))
        assert past[4] == 256
        out, new = attn.decode_split(q, K[:, :, n - 1:], V[:, :, n - 1:], past, [seg])
        # the returned past is what decode() returns for the same live cache without the frozen entry, window contents included
        twin = attn.to_fused(attn.build_cache(K[:, :, F:n - 1].contiguous(), V[:, :, F:n - 1].contiguous()))
        _, ref = attn.decode(q, K[:, :, n - 1:], V[:, :, n - 1:], twin)
        assert len(new) == 6 and new[4:] == ref[4:] == (256, n - F) and type(new[0]) is type(ref[0]) and type(new[2]) is type(ref[2])
        for i in (1, 3):
            assert new[i].len == ref[i].len == 41 and new[i].cap == ref[i].cap
            assert torch.equal(_bits(new[i].buf[:, :, :41]), _bits(ref[i].buf[:, :, :41]))
        return out, Kp, Vp

    # needles: heads 0-3 in the shared part (the same token for both sequences: there is one copy), heads 4-7 in the live part, which
    # differs per sequence; on the cut and on the seams
    pos = np.array([[0, F - 1, 64, 319, F, F + 255, F + 256, n - 1], [0, F - 1, 64, 319, F + 1, F + 254, n - 2, F + 256]])
    if Dd == 64:
        K, V, q = needle_data_64(B, Hq, Hkv, n, pos, seed=5)
    else:
        K, V, q, _ = xd.needle_data(B, Hq, Hkv, n, pos, k_sparsity=S, seed=5, device=DEV)
    K[1, :, :F], V[1, :, :F] = K[0, :, :F], V[0, :, :F]      # one prefix: sequence 1's needles there sit where sequence 0's do
    out, _, _ = run(K, V, q)
    want = needle_expect_64(V, pos, C_all, groups) if Dd == 64 else xd.needle_expect(V, pos, C_all, S, Hq)
    miss = xd.needle_misses(out, want)
    assert not miss.any(), f"rows {miss.nonzero().tolist()} differ from the whole"

    # random data: the split bound of DESIGN.md 4.9 against the model of the whole
    g = torch.Generator(device=DEV).manual_seed(Dd)
    K = torch.randn((B, Hkv, n, Dd), generator=g, device=DEV).half()
    V = torch.randn((B, Hkv, n, Dd), generator=g, device=DEV).half()
    q = torch.randn((B, Hq, 1, Dd), generator=g, device=DEV).half()
    K[1, :, :F], V[1, :, :F] = K[0, :, :F], V[0, :, :F]
    out, Kp, Vp = run(K, V, q)
    want, bound = xd.hook_model(q, Kp, Vp, groups)
    lse_all, _ = pu.lse_model(q, Kp, groups)
    parts, lse_bounds = [], []
    for a, b in ((0, F), (F, n)):
        o_i, _ = xd.hook_model(q, Kp[:, :, a:b], Vp[:, :, a:b], groups)
        l_i, bl_i = pu.lse_model(q, Kp[:, :, a:b], groups)
        parts.append((o_i, torch.exp(l_i - lse_all)))
        lse_bounds.append(bl_i)
    r = float(((out.double() - want).abs() / su.split_bound(parts, lse_bounds, want, bound)).max())
    print(f"shared split D={Dd} {kind}: |split - whole model| / bound = {r:.3f}")
    assert r <= 1.0


def test_a_cache_that_has_grown_by_extents_is_refused(pkg):
    from mustafar_amd import partial
    Hkv, groups = 2, 4
    attn = _hook(128, Hkv * groups, Hkv, arena=True)
    g = torch.Generator(device=DEV).manual_seed(1)
    K = torch.randn((1, Hkv, 288 + 255, 128), generator=g, device=DEV).half()
    past = attn.to_fused(attn.build_cache(K, K.clone()))
    q = torch.randn((1, Hkv * groups, 1, 128), generator=g, device=DEV).half()
    _, past = attn.decode_fused(q, K[:, :, :1].contiguous(), K[:, :, :1].contiguous(), past)
    assert past[0].extents, "the cache did not grow by an extent"
    with pytest.raises(ValueError, match="consolidate"):
        partial.SharedSegment(past[0], past[2], past[0].total_tokens)
    seg = partial.SharedSegment(past[0].consolidate(), past[2].consolidate(), past[0].total_tokens)
    assert seg.kv_heads == Hkv and seg.tokens == 512


# ---- 5. graph -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dd", [64, 128])
def test_one_graph_of_call_and_merge_replays_bit_for_bit(pkg, Dd):
    n, Hkv, groups, T = 8, 2, 4, 576
    K, V, _ = _rand(n, Hkv, T, groups, Dd, seed=3)
    sc = su.SharedCall(pkg, oracle_prune(K, S), oracle_prune(V, S), groups, n)
    g = torch.Generator(device=DEV).manual_seed(4)
    qs = torch.randn((3, n, Hkv * groups, 1, Dd), generator=g, device=DEV).half()
    eager = []
    for i in range(3):
        out, lse = sc.call(qs[i])
        eager.append((out.clone(), lse.clone()))
    q_in = torch.empty_like(qs[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sc.call(q_in.copy_(qs[0]))
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = sc.call(q_in)
    for i in (1, 2, 0):
        q_in.copy_(qs[i])
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(eager[i][0])) and torch.equal(_bits(lse), _bits(eager[i][1])), f"replay of query {i}"


# ---- 6. memory ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dd", [64, 128])
def test_one_copy_holds_the_bytes_of_one_sequence(pkg, Dd):
    from mustafar_amd import partial
    from mustafar_amd.hook import _compress
    bsz, Hkv, groups, T = 3, 2, 4, 256
    attn = _hook(Dd, Hkv * groups, Hkv)
    K, V, _ = _rand(1, Hkv, T, groups, Dd, seed=6)
    seg = partial.SharedSegment.from_dense(attn, K, V)

    def held(x, prune, which):
        c = _compress(prune(x).reshape(-1, T, Dd).contiguous(), which)
        return c[0].numel() * 8 + c[1].numel() * 4 + c[3].numel() * 4 + c[2].flat.numel() * 2

    one = held(K, attn.dh_prune_key, "key") + held(V, attn.dh_prune_value, "value")
    rep = held(K.expand(bsz, -1, -1, -1).contiguous(), attn.dh_prune_key, "key") + \
        held(V.expand(bsz, -1, -1, -1).contiguous(), attn.dh_prune_value, "value")
    assert seg.bytes_in_use() == one and rep == bsz * one
