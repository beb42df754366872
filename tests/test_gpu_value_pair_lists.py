"""GPU: sorted channel lists over pairs of blocks for a value base (include/mustafar_hip.h: MUSTAFAR_VIEW_VALUE_PAIR_LISTS).

`MustafarAttention.to_fused()` prefers this form for the value BASE of an arena where the launch of the call shape reads it (the GQA-4
one-pass super-block kernel on the two vector engines) and key rows are wanted too; `value_pair_lists=False` falls back to the lists per
block, `value_lists=False` to tiles.  All at G = 4, D = 128, one or two kv heads, batch 1-2, at four blocks per workgroup
(mustafar_tune(1, 2), as tests/test_gpu_value_lists.py):
  1. the device retile, both directions, against tests/value_pair_lists_ref.py and bit for bit back to the base arrays;
  2. decode parity: pair lists, lists per block and tiles, with and without key rows, against the native two-call sequence and against
     each other, both engines; unequal sparsities; the special pairs; workgroups with one, two and three blocks; a negative control;
  3. growth: an extent in tiles behind a base in pair lists across a trigger, graphs with a step counter and a device-side T;
  4. stickiness of require_tiles(), the knobs, the form the launch reports."""
import os

import numpy as np
import pytest
import torch

import value_pair_lists_ref as ref
from tests import exact_data as xd
from tests.test_value_pair_lists_host import special_pair_rows
from tests.util import NATIVE_ULPS, excess

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 32
FORM_SB = 3
FORMS = ("pairs", "lists", "tiles")


def _lib():
    from mustafar_amd import _lib as lib
    return lib


@pytest.fixture
def tbw():
    """The super-block kernel at small shapes, four blocks per workgroup (mustafar_tune(1, 2); the small form stays out)."""
    L = _lib().load()
    assert L.mustafar_tune(1, 2) == 0
    yield 2
    L.mustafar_tune(1, 0)


def _attn(hq, hkv, form="pairs", api="fused", arena=True, ks=0.7, vs=0.7, **kw):
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    return MustafarAttention(MustafarConfig(num_attention_heads=hq, num_key_value_heads=hkv, k_sparsity=ks, v_sparsity=vs, api=api,
                                            arena=arena, value_lists=form != "tiles", value_pair_lists=form == "pairs", **kw))


def _inputs(seed, bsz, hq, hkv, T, w=40, steps=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g).half().to(DEV)
    K0, V0 = rnd(bsz, hkv, T + R + w, 128), rnd(bsz, hkv, T + R + w, 128)
    return K0, V0, [(rnd(bsz, hq, 1, 128), rnd(bsz, hkv, 1, 128), rnd(bsz, hkv, 1, 128)) for _ in range(steps)]


def _is(arena, form):
    return {"pairs": arena.value_pair_lists and arena.value_lists, "lists": arena.value_lists and not arena.value_pair_lists,
            "tiles": not arena.value_lists and not arena.value_pair_lists}[form]


def _settle(past, form):
    """The value base of `past` in `form`.  With key rows turned off to_fused() takes the lists per block: pair lists are asked for."""
    v = past[2]
    if form == "pairs" and not v.value_pair_lists:
        v.require_tiles(sticky=False)
        assert v.to_value_pair_lists()
    assert _is(v, form), form
    return past


def _fused(attn, K0, V0, form="pairs"):
    return _settle(attn.to_fused(attn.build_cache(K0.clone(), V0.clone())), form)


def _form():
    return (_lib().load().mustafar_last_decode_choice() >> 8) & 15


# ---- 1. retile round trip ----------------------------------------------------------------------------------------------------------
def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "compress_reference.npz"))["rand_B2_t256_s0.7__x"].view(np.float16)


def _special(T):
    x = special_pair_rows(seed=T, T=max(T, 448))
    return np.ascontiguousarray(x[:, :T]) if T < 448 else x   # (256 tokens: the pairs of depth 128 and of nothing)


@pytest.mark.parametrize("data", ["special_256", "special_1280", "special_4160", "golden"])   # 4160: 65 blocks -- 33 pairs, the last a half
def test_retile_round_trip_is_bit_exact_and_pair_lists_equal_the_reference(data, golden_dir):   # pair, 67 table entries: a second trip of the scan
    from mustafar_amd.cache import CompressedArena
    x = _golden(golden_dir) if data == "golden" else _special(int(data.split("_")[1]))
    H, T = x.shape[0], x.shape[1]
    a = CompressedArena.from_pruned(torch.from_numpy(x).to(DEV), "value")
    if data != "golden":   # kept +0 at token 0 and kept -0 at token 9 of head 1: entries whose value is zero (the bitmap bit stays set)
        for t, bits in ((0, 0), (9, -32768)):
            a.nz.view(torch.int16)[1, 2 * int(a.idx[1, t])] = bits
    base = a.to_reference()
    bmp0, idx0, nz0 = base[0].clone(), base[1].clone(), [s.clone() for s in base[2]]
    table, blocks = ref.tiles_to_pair_lists(bmp0.cpu().numpy().view(np.uint64), idx0.cpu().numpy().view(np.uint32),
                                            [s.cpu().numpy().view(np.uint16) for s in nz0], T)
    if data != "golden":
        hdr = lambda p: blocks[0][4 * int(table[0, 2 * p]):4 * int(table[0, 2 * p]) + 256]
        assert hdr(0)[128 + 63] == 1 and hdr(0)[63] == 6 and hdr(0)[192 + 63] == 1   # depth 128 beside cnt 0
        assert not hdr(1)[128:256].any()                                            # an all-zero pair
        if T >= 448:
            assert list(hdr(2)[128:192]) == [64] * 5 + [0] * 59                     # all lists equal, depth 10 = 2 mod 4
    assert a.to_value_pair_lists() and a.value_pair_lists and a.value_lists and not a.key_rows
    assert not a.to_value_lists() and a.value_pair_lists, "one form at a time"
    assert np.array_equal(a.lists_table.cpu().numpy().view(np.uint32), table)
    got = a.lists_blocks.cpu().numpy().view(np.uint8)
    for h in range(H):
        assert np.array_equal(got[h, :blocks[h].size], blocks[h]), f"pairs of head {h}"
    assert a.bytes_in_use() == H * (2 * ((T // 64 + 1) // 2) + 1) * 4 + sum(b.size for b in blocks)
    assert a.bytes_reserved() > 0 and len(a.signature()) == 5
    assert a.value_pair_lists, "sizes, signature and the lists themselves are read without a retile"
    a.require_tiles()
    assert not a.value_lists and not a.value_pair_lists
    back = a.to_reference()
    assert torch.equal(back[0], bmp0) and torch.equal(back[1], idx0)
    for h in range(H):
        assert torch.equal(back[2][h].view(torch.int16), nz0[h].view(torch.int16)), f"stream of head {h}"
    # to_value_lists() still gives the lists per block, and reading a tile array settles either form in tiles
    a.keep_tiles = False
    assert a.to_value_lists() and a.value_lists and not a.value_pair_lists
    a.require_tiles(sticky=False)
    assert a.to_value_pair_lists()
    assert torch.equal(a.idx[:, :2 * T + 1], idx0.view(H, -1)) and not a.value_lists and a.keep_tiles
    k = CompressedArena.from_pruned(torch.from_numpy(x).to(DEV), "key")
    assert not k.to_value_pair_lists() and not k.value_lists, "a key arena does not take the form"


# ---- 2. decode parity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["valu", "dot2"])
@pytest.mark.parametrize("bsz,hkv,T", [(1, 2, 256), (2, 1, 512), (2, 2, 1280)])
def test_decode_with_pair_lists_equals_lists_tiles_and_the_native_sequence(tbw, engine, bsz, hkv, T):
    hq = 4 * hkv
    K0, V0, [(q, k, v)] = _inputs(T + 2, bsz, hq, hkv, T)
    native = _attn(hq, hkv, api="native", arena=False)
    want, _ = native.decode(q, k, v, native.build_cache(K0.clone(), V0.clone()))
    outs = {}
    for rows in (True, False):
        for form in FORMS:
            attn = _attn(hq, hkv, form, engine=engine, key_rows=rows)
            past = _fused(attn, K0, V0, form)
            assert past[0].key_rows == rows
            o, _ = attn.decode_fused(q, k, v, past)
            assert _form() == FORM_SB and past[0].key_rows == rows and _is(past[2], form)
            outs[rows, form] = o
            print(f"excess over the native sequence, rows {rows}, {form}: {excess(o, want, NATIVE_ULPS):.3f}")
            assert excess(o, want, NATIVE_ULPS) <= 1.0, (rows, form, excess(o, want, NATIVE_ULPS))
    for rows in (True, False):
        for other in ("lists", "tiles"):
            assert excess(outs[rows, "pairs"], outs[rows, other], NATIVE_ULPS) <= 1.0, (rows, other)


@pytest.mark.parametrize("engine", ["valu", "dot2"])
def test_unequal_sparsities(tbw, engine):
    bsz, hkv, hq, T = 2, 2, 8, 512
    K0, V0, [(q, k, v)] = _inputs(7, bsz, hq, hkv, T)
    native = _attn(hq, hkv, api="native", arena=False, ks=0.5, vs=0.8)
    want, _ = native.decode(q, k, v, native.build_cache(K0.clone(), V0.clone()))
    outs = {}
    for form in FORMS:
        attn = _attn(hq, hkv, form, engine=engine, ks=0.5, vs=0.8)
        outs[form] = attn.decode_fused(q, k, v, _fused(attn, K0, V0, form))[0]
        assert _form() == FORM_SB and excess(outs[form], want, NATIVE_ULPS) <= 1.0
    assert excess(outs["pairs"], outs["lists"], NATIVE_ULPS) <= 1.0 and excess(outs["pairs"], outs["tiles"], NATIVE_ULPS) <= 1.0


def _pruned_past(attn, K0, V0, T, vp=None):
    """A cache of T tokens (any multiple of 64) from pruned rows, the rest of K0 / V0 as the window."""
    from mustafar_amd.cache import CompressedArena
    from mustafar_amd.hook import Past
    B = K0.shape[0] * K0.shape[1]
    kp = attn.dh_prune_key(K0[:, :, :T]).reshape(B, T, 128)
    if vp is None:
        vp = attn.dh_prune_value(V0[:, :, :T]).reshape(B, T, 128)
    return attn.to_fused(Past(CompressedArena.from_pruned(kp, "key"), K0[:, :, T:].clone(), CompressedArena.from_pruned(vp.clone(), "value"),
                              V0[:, :, T:].clone(), T, K0.shape[2]))


def test_special_pairs_decode_like_tiles(tbw):
    """The special pairs of the retile test as the value cache of a decode: depth 128 beside cnt 0, an all-zero pair, equal lists with a
    half word, a trailing half pair (448 tokens: seven blocks)."""
    bsz, hkv, hq, T = 1, 2, 8, 448
    K0, V0, [(q, k, v)] = _inputs(8, bsz, hq, hkv, T)
    vp = torch.from_numpy(special_pair_rows(seed=5, T=T)).to(DEV)
    outs = {}
    for form in FORMS:
        attn = _attn(hq, hkv, form, engine="valu")
        past = _settle(_pruned_past(attn, K0, V0, T, vp), form)
        outs[form] = attn.decode_fused(q, k, v, past, defer_trigger=True)[0]
        assert _form() == FORM_SB
    assert excess(outs["pairs"], outs["tiles"], NATIVE_ULPS) <= 1.0 and excess(outs["pairs"], outs["lists"], NATIVE_ULPS) <= 1.0


@pytest.mark.parametrize("engine", ["valu", "dot2"])
@pytest.mark.parametrize("T", [320, 384, 448])
def test_workgroups_with_one_two_and_three_blocks(tbw, engine, T):
    """5, 6 and 7 blocks at four per workgroup.  The last workgroup holds one block (a trailing half pair), two (each pair of waves one
    block of the SAME pair of blocks: the other block's half of the e table weighs zero, and the second pair of waves starts at an odd
    block) or three (a pair and a half pair)."""
    bsz, hkv, hq = 1, 2, 8
    K0, V0, [(q, k, v)] = _inputs(T, bsz, hq, hkv, T)
    outs = {}
    for form in ("pairs", "tiles"):
        attn = _attn(hq, hkv, form, engine=engine)
        outs[form], _ = attn.decode_fused(q, k, v, _settle(_pruned_past(attn, K0, V0, T), form), defer_trigger=True)
        assert _form() == FORM_SB
    assert excess(outs["pairs"], outs["tiles"], NATIVE_ULPS) <= 1.0


def test_exact_sums_give_bit_equal_outputs_on_the_exact_engine(tbw):
    """V of small dyadic integers and a q of zeros (every e the same power of two): every product and every partial sum of the value
    phase is exact in fp32, so the order of the sum does not matter."""
    bsz, hkv, hq, T = 2, 2, 8, 512
    rng = np.random.default_rng(3)
    V0 = torch.from_numpy(xd.dyadic(rng, (bsz, hkv, T + R + 8, 128), 3, 2)).to(DEV)
    K0, _, [(q, k, _)] = _inputs(4, bsz, hq, hkv, T, w=8)
    q = torch.zeros_like(q)
    v = V0[:, :, -1:].clone()
    outs = {}
    for form in FORMS:
        attn = _attn(hq, hkv, form, engine="valu")
        outs[form] = attn.decode_fused(q, k, v, _fused(attn, K0, V0, form))[0]
        assert _form() == FORM_SB
    assert torch.equal(outs["pairs"], outs["tiles"]) and torch.equal(outs["pairs"], outs["lists"])


def test_one_altered_token_byte_fails_the_parity(tbw):
    """The negative control.  q points at key token 7, so that token carries nearly all the weight; one list entry of token 7 is sent to
    token 100 instead: its channel loses a whole value."""
    bsz, hkv, hq, T = 1, 2, 8, 256
    K0, V0, [(q, k, v)] = _inputs(51, bsz, hq, hkv, T)
    q = (3 * K0[:, :, 7:8]).repeat_interleave(4, dim=1).contiguous()
    attn, tiles = _attn(hq, hkv, engine="valu"), _attn(hq, hkv, "tiles", engine="valu")
    want, _ = tiles.decode_fused(q, k, v, _fused(tiles, K0, V0, "tiles"))
    past = _fused(attn, K0, V0)
    window = lambda p: (p[0], p[1].clone(), p[2], p[3].clone(), p[4], p[5])
    good, _ = attn.decode_fused(q, k, v, window(past))
    assert excess(good, want, NATIVE_ULPS) <= 1.0
    arena = past[2]
    raw = arena.lists_blocks.view(torch.uint8)
    start = 4 * (int(arena.lists_table[0, 0]) + 64)                      # head 0, pair 0, half 0: its first token row
    row = raw[0, start:start + 4 * int(raw[0, 4 * int(arena.lists_table[0, 0]) + 128])].cpu().numpy()
    at = int(np.flatnonzero(row == 7)[0])
    raw[0, start + at] = 100
    bad, _ = attn.decode_fused(q, k, v, window(past))
    assert arena.value_pair_lists and _form() == FORM_SB
    assert excess(bad, want, NATIVE_ULPS) > 1.0, "the parity check does not see a wrong token"


# ---- 3. growth ---------------------------------------------------------------------------------------------------------------------
def test_an_extent_in_tiles_behind_a_base_in_pair_lists_across_a_trigger(tbw):
    bsz, hkv, hq, T = 1, 2, 8, 512
    K0, V0, steps = _inputs(21, bsz, hq, hkv, T, w=250, steps=6 + 3)
    res = {}
    for form in ("pairs", "tiles"):
        attn = _attn(hq, hkv, form, engine="dot2")
        past = _fused(attn, K0, V0, form)
        outs = []
        for q, k, v in steps:
            o, past = attn.decode_fused(q, k, v, past, defer_trigger=True)
            if attn.trigger_due(past):
                past = attn.run_triggers([past])[0]
            outs.append(o)
        assert len(past[2].extents) == 1 and _is(past[2], form) and not any(e.value_lists for e in past[2].extents)
        assert _form() == FORM_SB
        res[form] = (outs, past)
    for i, (a, b) in enumerate(zip(res["pairs"][0], res["tiles"][0])):
        assert excess(a, b, NATIVE_ULPS) <= 1.0, f"step {i}"
    assert res["pairs"][1][2].bytes_in_use() > 0
    a, b = res["pairs"][1][2].to_reference(), res["tiles"][1][2].to_reference()   # (retiles the base back: the whole cache in the reference layout)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(torch.cat(list(a[2])), torch.cat(list(b[2])))
    c = res["pairs"][1][2].consolidate()
    assert not c.value_lists and c.total_tokens == T + 256


def test_a_graph_with_a_step_counter_over_a_base_in_pair_lists(tbw):
    bsz, hkv, hq, T = 1, 2, 8, 512
    K0, V0, steps = _inputs(23, bsz, hq, hkv, T, w=40, steps=3)
    attn, tiles = _attn(hq, hkv, engine="dot2"), _attn(hq, hkv, "tiles", engine="dot2")
    past, past_t = _fused(attn, K0, V0), _fused(tiles, K0, V0, "tiles")
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    gq, gk, gv = (x.clone() for x in steps[0])
    attn.decode_fused(gq, gk, gv, (past[0], past[1].clone(), past[2], past[3].clone(), past[4], past[5]))   # scratch outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g_out, _ = attn.decode_fused(gq, gk, gv, past, step_counter=counter)
    assert past[2].value_pair_lists, "a capture leaves the lists alone"
    for i, (q, k, v) in enumerate(steps):
        counter.fill_(i)   # (the steps since the capture: the caller's to advance)
        gq.copy_(q); gk.copy_(k); gv.copy_(v)
        g.replay()
        past = attn.advance(past, 1)
        o_t, past_t = tiles.decode_fused(q, k, v, past_t, defer_trigger=True)
        torch.cuda.synchronize()
        assert excess(g_out, o_t, NATIVE_ULPS) <= 1.0


def test_the_refusal_under_capture(tbw):
    """A captured call whose launch reads tiles cannot retile an arena in pair lists back: it raises, and the lists stay."""
    bsz, hkv, hq, T = 1, 2, 8, 512
    K0, V0, [(q, k, v)] = _inputs(33, bsz, hq, hkv, T)
    attn = _attn(hq, hkv, engine="dot2")
    p = _fused(attn, K0, V0)
    attn.decode_fused(q, k, v, (p[0], p[1].clone(), p[2], p[3].clone(), p[4], p[5]))   # scratch outside the capture
    attn.cfg.engine = "mfma"
    mf = _attn(hq, hkv, "tiles", engine="mfma")
    mf.decode_fused(q, k, v, _fused(mf, K0, V0, "tiles"))                               # (the matrix pipe's scratch too)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="require_tiles"):
        with torch.cuda.graph(g):
            attn.decode_fused(q, k, v, p, step_counter=counter)
    assert p[2].value_pair_lists


def test_one_graph_with_a_device_side_t_across_a_trigger(tbw):
    bsz, hkv, hq, T = 1, 2, 8, 512
    K0, V0, steps = _inputs(22, bsz, hq, hkv, T, w=253, steps=3)
    attn, tiles = _attn(hq, hkv, engine="dot2"), _attn(hq, hkv, "tiles", engine="dot2")
    past, past_t = _fused(attn, K0, V0), _fused(tiles, K0, V0, "tiles")
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    t_dev = torch.full((1,), T, dtype=torch.int32, device=DEV)
    gq, gk, gv = (x.clone() for x in steps[0])
    attn.decode_fused(gq, gk, gv, (past[0], past[1].clone(), past[2], past[3].clone(), past[4], past[5]))   # scratch outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g_out, _ = attn.decode_fused(gq, gk, gv, past, step_counter=counter, t_device=t_dev, t_capacity=T + 256)
    assert past[2].value_pair_lists
    o_t = None
    for q, k, v in steps:
        counter.fill_(past[1].len - (R + 253))
        gq.copy_(q); gk.copy_(k); gv.copy_(v)
        g.replay()
        past = attn.advance(past, 1)
        o_t, past_t = tiles.decode_fused(q, k, v, past_t, defer_trigger=True)
        torch.cuda.synchronize()
        assert excess(g_out, o_t, NATIVE_ULPS) <= 1.0
    assert attn.trigger_due(past) and tiles.trigger_due(past_t)
    past = attn.run_triggers([past])[0]
    past_t = tiles.run_triggers([past_t])[0]
    assert len(past[2].extents) == 1 and past[2].value_pair_lists
    t_dev.fill_(T + 256)
    counter.fill_(past[1].len - (R + 253))
    q, k, v = steps[0]
    gq.copy_(q); gk.copy_(k); gv.copy_(v)
    g.replay()
    o_t, _ = tiles.decode_fused(q, k, v, past_t, defer_trigger=True)
    torch.cuda.synchronize()
    assert excess(g_out, o_t, NATIVE_ULPS) <= 1.0


@pytest.mark.parametrize("engine", ["valu", "dot2"])
def test_a_device_side_t_below_the_base_leaves_blocks_of_a_pair_unused(tbw, engine):
    """A base of eight blocks read with 5, 6, 7 and 8 blocks in use (`t_device`; the launch is sized for T + 256).  With 5 and 7 the last
    pair of blocks in use has its second block in storage but NOT in use: its half of the e table has to weigh zero.  Against the same
    graph over tiles, and against an eager call over a cache that holds the tokens in use and nothing else."""
    bsz, hkv, hq, T = 1, 2, 8, 512
    K0, V0, [(q, k, v)] = _inputs(61, bsz, hq, hkv, T)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    graphs = {}
    for form in ("pairs", "tiles"):
        attn = _attn(hq, hkv, form, engine=engine)
        past = _fused(attn, K0, V0, form)
        t_dev = torch.full((1,), T, dtype=torch.int32, device=DEV)
        attn.decode_fused(q, k, v, (past[0], past[1].clone(), past[2], past[3].clone(), past[4], past[5]))   # scratch outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out, _ = attn.decode_fused(q, k, v, past, step_counter=counter, t_device=t_dev, t_capacity=T + 256)
        assert _is(past[2], form)
        graphs[form] = (g, out, t_dev, past)
    eager = _attn(hq, hkv, "tiles", engine=engine)
    seen = {}
    for t in (320, 384, 448, 512):
        got = {}
        for form, (g, out, t_dev, _) in graphs.items():
            t_dev.fill_(t)
            g.replay()
            torch.cuda.synchronize()
            got[form] = out.clone()
        assert excess(got["pairs"], got["tiles"], NATIVE_ULPS) <= 1.0, t
        # the cache of the first t tokens (pruning is per token: a prefix of the base) with the same window
        from mustafar_amd.cache import CompressedArena
        from mustafar_amd.hook import Past
        kp = eager.dh_prune_key(K0[:, :, :t]).reshape(bsz * hkv, t, 128)
        vp = eager.dh_prune_value(V0[:, :, :t]).reshape(bsz * hkv, t, 128)
        short = eager.to_fused(Past(CompressedArena.from_pruned(kp, "key"), K0[:, :, T:].clone(), CompressedArena.from_pruned(vp, "value"),
                                    V0[:, :, T:].clone(), t, t + K0.shape[2] - T))
        want, _ = eager.decode_fused(q, k, v, short, defer_trigger=True)
        print(f"{t} tokens in use: excess over the cache of {t} tokens {excess(got['pairs'], want, NATIVE_ULPS):.3f}")
        assert excess(got["pairs"], want, NATIVE_ULPS) <= 1.0, t
        seen[t] = got["pairs"]
    assert excess(seen[320], seen[512], NATIVE_ULPS) > 1.0, "the tokens in use did not change the result"
    assert graphs["pairs"][3][2].value_pair_lists


# ---- 4. stickiness, knobs, the reported form ---------------------------------------------------------------------------------------
def test_require_tiles_is_sticky_and_whatever_needs_tiles_gets_the_tile_arenas_results(tbw):
    bsz, hkv, hq, T = 1, 2, 8, 512
    K0, V0, [(q, k, v)] = _inputs(31, bsz, hq, hkv, T)
    attn, tiles = _attn(hq, hkv, engine="dot2"), _attn(hq, hkv, "tiles", engine="dot2", key_rows=False)
    p, pt = _fused(attn, K0, V0), _fused(tiles, K0, V0, "tiles")
    a, b = p[2].to_reference(), pt[2].to_reference()
    assert not p[2].value_lists and p[2].keep_tiles
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(torch.cat(list(a[2])), torch.cat(list(b[2])))
    assert not attn.to_fused(p)[2].value_lists, "once retiled back, the arena stays in tiles"
    # consolidate() returns a tile arena and clears the stickiness: the next to_fused() takes pair lists again
    p = _fused(attn, K0, V0)
    c = p[2].consolidate()
    assert c is p[2] and not c.value_lists
    assert attn.to_fused(p)[2].value_pair_lists
    # decode_multi reads tiles
    p, pt = _fused(attn, K0, V0), _fused(tiles, K0, V0, "tiles")
    g = torch.Generator(device="cpu").manual_seed(5)
    q2 = torch.randn(bsz, hq, 2, 128, generator=g).half().to(DEV)
    k2, v2 = torch.randn(bsz, hkv, 2, 128, generator=g).half().to(DEV), torch.randn(bsz, hkv, 2, 128, generator=g).half().to(DEV)
    om, _ = attn.decode_multi(q2, k2, v2, p)
    ot, _ = tiles.decode_multi(q2, k2, v2, pt)
    assert not p[2].value_lists and p[2].keep_tiles and torch.equal(om, ot)
    # an engine switch to the matrix pipe on an arena in pair lists: retiled back, the tile arena's bits
    p, pt = _fused(attn, K0, V0), _fused(tiles, K0, V0, "tiles")
    attn.cfg.engine = tiles.cfg.engine = "mfma"
    o1, _ = attn.decode_fused(q, k, v, p)
    o2, _ = tiles.decode_fused(q, k, v, pt)
    assert not p[2].value_lists and torch.equal(o1, o2)


def test_the_fallback_knobs_and_the_reported_form(tbw, monkeypatch):
    bsz, hkv, hq, T = 1, 2, 8, 512
    K0, V0, [(q, k, v)] = _inputs(41, bsz, hq, hkv, T)
    lib = _lib()
    outs = {}
    for form in FORMS:
        attn = _attn(hq, hkv, form, engine="dot2")
        p = attn.to_fused(attn.build_cache(K0.clone(), V0.clone()))
        assert _is(p[2], form) and p[0].key_rows, form
        assert p[2].view.flags == {"pairs": lib.VIEW_VALUE_PAIR_LISTS, "lists": lib.VIEW_VALUE_LISTS, "tiles": 0}[form]
        outs[form], _ = attn.decode_fused(q, k, v, p)
        assert _form() == FORM_SB and _is(p[2], form)
    assert excess(outs["pairs"], outs["lists"], NATIVE_ULPS) <= 1.0 and excess(outs["pairs"], outs["tiles"], NATIVE_ULPS) <= 1.0
    monkeypatch.setenv("MUSTAFAR_VALUE_PAIR_LISTS", "0")
    env = _attn(hq, hkv, engine="dot2")
    p = env.to_fused(env.build_cache(K0.clone(), V0.clone()))
    o_env, _ = env.decode_fused(q, k, v, p)
    assert _is(p[2], "lists") and _form() == FORM_SB and torch.equal(o_env, outs["lists"])
    monkeypatch.delenv("MUSTAFAR_VALUE_PAIR_LISTS")
    monkeypatch.setenv("MUSTAFAR_VALUE_LISTS", "0")
    p = env.to_fused(env.build_cache(K0.clone(), V0.clone()))
    assert _is(p[2], "tiles")
    monkeypatch.delenv("MUSTAFAR_VALUE_LISTS")
    assert _is(env.to_fused(env.build_cache(K0.clone(), V0.clone()))[2], "pairs")
    # where key rows are turned off to_fused() keeps the lists per block; a key arena that merely stays in tiles (sticky) changes nothing
    assert _is(_attn(hq, hkv, engine="dot2", key_rows=False).to_fused(env.build_cache(K0.clone(), V0.clone()))[2], "lists")
    p = env.to_fused(env.build_cache(K0.clone(), V0.clone()))
    p[0].require_tiles()
    p[2].require_tiles(sticky=False)
    p = env.to_fused(p)
    assert not p[0].key_rows and _is(p[2], "pairs")
    # where the launch form does not read lists nothing is retiled either: MHA, the matrix pipe, two blocks per workgroup, the default rule
    assert _is(_attn(8, 8).to_fused(_attn(8, 8).build_cache(K0.repeat(1, 4, 1, 1), V0.repeat(1, 4, 1, 1)))[2], "tiles")
    assert _is(_attn(hq, hkv, engine="mfma").to_fused(env.build_cache(K0.clone(), V0.clone()))[2], "tiles")
    lib.load().mustafar_tune(1, 1)
    assert _is(env.to_fused(env.build_cache(K0.clone(), V0.clone()))[2], "tiles")
    lib.load().mustafar_tune(1, 0)
    assert _is(env.to_fused(env.build_cache(K0.clone(), V0.clone()))[2], "tiles")
