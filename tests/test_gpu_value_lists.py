"""GPU: sorted channel lists of a value base (include/mustafar_hip.h: MUSTAFAR_VIEW_VALUE_LISTS).

`MustafarAttention.to_fused()` retiles the value BASE of an arena into channel lists where the launch of the call shape reads them (the
GQA-4 one-pass super-block kernel on the two vector engines); everything else gets tiles back through `CompressedArena.require_tiles()`.
All at G = 4, D = 128, one or two kv heads, batch 1-2, at four blocks per workgroup (mustafar_tune(1, 2), as tests/test_gpu_key_rows.py):
  1. the device retile, both directions, against tests/value_lists_ref.py and bit for bit back to the base arrays;
  2. decode parity: lists on against lists off and against the native two-call sequence, both engines, the three on / off combinations
     with key rows, unequal sparsities, mask, LSE; bit-equal outputs on data whose sums are exact;
  3. growth: extents in tiles behind a base in lists, a graph with a device-side T across a trigger, 34 alternating replays;
  4. fallbacks and refusals;  5. off by config and by environment."""
import ctypes
import os

import numpy as np
import pytest
import torch

import value_lists_ref as ref
from tests import exact_data as xd
from tests.test_value_lists_host import special_rows
from tests.util import NATIVE_ULPS, excess

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 32
FORM_SB = 3


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


def _attn(hq, hkv, api="fused", arena=True, ks=0.7, vs=0.7, **kw):
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    return MustafarAttention(MustafarConfig(num_attention_heads=hq, num_key_value_heads=hkv, k_sparsity=ks, v_sparsity=vs, api=api,
                                            arena=arena, **kw))


def _inputs(seed, bsz, hq, hkv, T, w=40, steps=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g).half().to(DEV)
    K0, V0 = rnd(bsz, hkv, T + R + w, 128), rnd(bsz, hkv, T + R + w, 128)
    return K0, V0, [(rnd(bsz, hq, 1, 128), rnd(bsz, hkv, 1, 128), rnd(bsz, hkv, 1, 128)) for _ in range(steps)]


def _fused(attn, K0, V0):
    return attn.to_fused(attn.build_cache(K0.clone(), V0.clone()))


def _form():
    return (_lib().load().mustafar_last_decode_choice() >> 8) & 15


# ---- 1. retile round trip ----------------------------------------------------------------------------------------------------------
def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "compress_reference.npz"))["rand_B2_t256_s0.7__x"].view(np.float16)


def _special(T):
    x = special_rows(seed=T, T=max(T, 320))
    if T < 320:   # the four special blocks of head 0 fit 256 tokens
        return np.ascontiguousarray(x[:, :T])
    return x


@pytest.mark.parametrize("data", ["special_256", "special_1280", "special_4160", "golden"])   # 4160: 65 blocks, a second trip of the table scan
def test_retile_round_trip_is_bit_exact_and_lists_equal_the_reference(data, golden_dir):
    from mustafar_amd.cache import CompressedArena
    x = _golden(golden_dir) if data == "golden" else _special(int(data.split("_")[1]))
    H, T = x.shape[0], x.shape[1]
    a = CompressedArena.from_pruned(torch.from_numpy(x).to(DEV), "value")
    if data != "golden":   # kept +0 at token 0 and kept -0 at token 9 of head 1: entries whose value is zero (the bitmap bit stays set)
        for t, bits in ((0, 0), (9, -32768)):
            a.nz.view(torch.int16)[1, 2 * int(a.idx[1, t])] = bits
    base = a.to_reference()
    bmp0, idx0, nz0 = base[0].clone(), base[1].clone(), [s.clone() for s in base[2]]
    table, blocks = ref.tiles_to_lists(bmp0.cpu().numpy().view(np.uint64), idx0.cpu().numpy().view(np.uint32),
                                       [s.cpu().numpy().view(np.uint16) for s in nz0], T)
    if data != "golden":
        hdr = lambda b: blocks[0][4 * int(table[0, b]):4 * int(table[0, b]) + 256]
        assert hdr(0)[128 + 31] == 1 and hdr(0)[63] == 6            # depth 64 beside cnt 0
        assert not hdr(1)[128:192].any()                           # an all-zero block
        assert list(hdr(2)[128:160]) == [64] * 5 + [0] * 27        # all lists equal, depth 10 = 2 mod 4
    assert a.to_value_lists() and a.value_lists and not a.key_rows
    assert np.array_equal(a.lists_table.cpu().numpy().view(np.uint32), table)
    got = a.lists_blocks.cpu().numpy().view(np.uint8)
    for h in range(H):
        assert np.array_equal(got[h, :blocks[h].size], blocks[h]), f"blocks of head {h}"
    assert a.bytes_in_use() == H * (T // 64 + 1) * 4 + sum(b.size for b in blocks)
    assert a.bytes_reserved() > 0 and len(a.signature()) == 5
    assert a.value_lists, "sizes, signature and the lists themselves are read without a retile"
    a.require_tiles()
    assert not a.value_lists
    back = a.to_reference()
    assert torch.equal(back[0], bmp0) and torch.equal(back[1], idx0)
    for h in range(H):
        assert torch.equal(back[2][h].view(torch.int16), nz0[h].view(torch.int16)), f"stream of head {h}"
    a.require_tiles()   # (nothing to do)
    # reading a tile array of an arena in lists settles it in tiles, like every other use of tiles
    a.keep_tiles = False
    assert a.to_value_lists() and a.value_lists
    assert torch.equal(a.idx[:, :2 * T + 1], idx0.view(H, -1)) and not a.value_lists and a.keep_tiles
    k = CompressedArena.from_pruned(torch.from_numpy(x).to(DEV), "key")
    assert not k.to_value_lists() and not k.value_lists, "a key arena does not take the form"


# ---- 2. decode parity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["valu", "dot2"])
@pytest.mark.parametrize("bsz,hkv,T", [(1, 2, 256), (2, 1, 512), (2, 2, 1280)])
def test_decode_with_value_lists_equals_tiles_and_the_native_sequence(tbw, engine, bsz, hkv, T):
    hq = 4 * hkv
    K0, V0, [(q, k, v)] = _inputs(T + 2, bsz, hq, hkv, T)
    native = _attn(hq, hkv, api="native", arena=False)
    want, _ = native.decode(q, k, v, native.build_cache(K0.clone(), V0.clone()))
    outs = {}
    for rows, lists in ((True, True), (False, True), (True, False), (False, False)):
        attn = _attn(hq, hkv, engine=engine, key_rows=rows, value_lists=lists)
        past = _fused(attn, K0, V0)
        assert past[0].key_rows == rows and past[2].value_lists == lists
        o, _ = attn.decode_fused(q, k, v, past)
        assert _form() == FORM_SB and past[0].key_rows == rows and past[2].value_lists == lists
        outs[rows, lists] = o
        assert excess(o, want, NATIVE_ULPS) <= 1.0, (rows, lists, excess(o, want, NATIVE_ULPS))
    for rows in (True, False):
        assert excess(outs[rows, True], outs[rows, False], NATIVE_ULPS) <= 1.0


@pytest.mark.parametrize("engine", ["valu", "dot2"])
def test_unequal_sparsities(tbw, engine):
    bsz, hkv, hq, T = 2, 2, 8, 512
    K0, V0, [(q, k, v)] = _inputs(7, bsz, hq, hkv, T)
    native = _attn(hq, hkv, api="native", arena=False, ks=0.5, vs=0.8)
    want, _ = native.decode(q, k, v, native.build_cache(K0.clone(), V0.clone()))
    outs = []
    for lists in (True, False):
        attn = _attn(hq, hkv, engine=engine, ks=0.5, vs=0.8, value_lists=lists)
        past = _fused(attn, K0, V0)
        assert past[2].value_lists == lists
        outs.append(attn.decode_fused(q, k, v, past)[0])
        assert _form() == FORM_SB and excess(outs[-1], want, NATIVE_ULPS) <= 1.0
    assert excess(outs[0], outs[1], NATIVE_ULPS) <= 1.0


def test_special_blocks_decode_like_tiles(tbw):
    """The special blocks of the retile test as the value cache of a decode: depth 64 beside cnt 0, an all-zero block, equal lists with a
    half word, a tie row."""
    from mustafar_amd.cache import CompressedArena
    from mustafar_amd.hook import Past
    bsz, hkv, hq, T = 1, 2, 8, 512
    K0, V0, [(q, k, v)] = _inputs(8, bsz, hq, hkv, T)
    vp = torch.from_numpy(special_rows(seed=5, T=T)).to(DEV)
    outs = []
    for lists in (True, False):
        attn = _attn(hq, hkv, engine="valu", value_lists=lists)
        kp = attn.dh_prune_key(K0[:, :, :T]).reshape(bsz * hkv, T, 128)
        past = attn.to_fused(Past(CompressedArena.from_pruned(kp, "key"), K0[:, :, T:].clone(), CompressedArena.from_pruned(vp.clone(), "value"),
                                  V0[:, :, T:].clone(), T, K0.shape[2]))
        assert past[2].value_lists == lists
        outs.append(attn.decode_fused(q, k, v, past, defer_trigger=True)[0])
        assert _form() == FORM_SB
    assert excess(outs[0], outs[1], NATIVE_ULPS) <= 1.0


@pytest.mark.parametrize("engine", ["valu", "dot2"])
def test_mask_and_lse_with_value_lists(tbw, engine):
    from tests.test_gpu_mask import _left_padding_mask
    bsz, hkv, hq, T = 2, 2, 8, 512
    K0, V0, [(q, k, v)] = _inputs(11, bsz, hq, hkv, T)
    mask = _left_padding_mask(bsz, T + R + 40 + 1, [0, 37])
    res = {}
    for lists in (True, False):
        attn = _attn(hq, hkv, engine=engine, value_lists=lists)
        past = _fused(attn, K0, V0)
        assert past[2].value_lists == lists
        o_m, _ = attn.decode_fused(q, k, v, _fused(attn, K0, V0), attention_mask=mask)
        o, lse, _ = attn.decode_fused(q, k, v, past, return_lse=True)
        assert _form() == FORM_SB
        res[lists] = (o_m, o, lse)
    assert excess(res[True][0], res[False][0], NATIVE_ULPS) <= 1.0 and excess(res[True][1], res[False][1], NATIVE_ULPS) <= 1.0
    assert torch.equal(res[True][2], res[False][2]), "the LSE comes from the key phase and the softmax step: the same bits"


def test_exact_sums_give_bit_equal_outputs_on_the_exact_engine(tbw):
    """V of small dyadic integers and a q of zeros (every e the same power of two): every product and every partial sum of the value
    phase is exact in fp32, so neither the order of the sum nor the split into blocks A and B matters."""
    bsz, hkv, hq, T = 2, 2, 8, 512
    rng = np.random.default_rng(3)
    V0 = torch.from_numpy(xd.dyadic(rng, (bsz, hkv, T + R + 8, 128), 3, 2)).to(DEV)
    K0, _, [(q, k, _)] = _inputs(4, bsz, hq, hkv, T, w=8)
    q = torch.zeros_like(q)
    v = V0[:, :, -1:].clone()
    outs = []
    for lists in (True, False):
        attn = _attn(hq, hkv, engine="valu", value_lists=lists)
        past = _fused(attn, K0, V0)
        assert past[2].value_lists == lists
        outs.append(attn.decode_fused(q, k, v, past)[0])
        assert _form() == FORM_SB
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("engine", ["valu", "dot2"])
@pytest.mark.parametrize("T", [320, 448])
def test_workgroups_with_an_odd_number_of_blocks(tbw, engine, T):
    """5 and 7 blocks at four per workgroup: the last workgroup holds one block (one pair idle, the other with a lone block A) or three."""
    from mustafar_amd.cache import CompressedArena
    from mustafar_amd.hook import Past
    bsz, hkv, hq = 1, 2, 8
    K0, V0, [(q, k, v)] = _inputs(T, bsz, hq, hkv, T)
    outs = {}
    for lists in (True, False):
        attn = _attn(hq, hkv, engine=engine, value_lists=lists)
        kp = attn.dh_prune_key(K0[:, :, :T]).reshape(bsz * hkv, T, 128)
        vp = attn.dh_prune_value(V0[:, :, :T]).reshape(bsz * hkv, T, 128)
        past = attn.to_fused(Past(CompressedArena.from_pruned(kp, "key"), K0[:, :, T:].clone(), CompressedArena.from_pruned(vp, "value"),
                                  V0[:, :, T:].clone(), T, K0.shape[2]))
        assert past[2].value_lists == lists
        outs[lists], _ = attn.decode_fused(q, k, v, past, defer_trigger=True)
        assert _form() == FORM_SB
    assert excess(outs[True], outs[False], NATIVE_ULPS) <= 1.0


# ---- 3. growth ---------------------------------------------------------------------------------------------------------------------
def test_extents_in_tiles_behind_a_base_in_lists(tbw):
    bsz, hkv, hq, T = 1, 2, 8, 512
    K0, V0, steps = _inputs(21, bsz, hq, hkv, T, w=250, steps=6 + 3)
    res = {}
    for lists in (True, False):
        attn = _attn(hq, hkv, engine="dot2", value_lists=lists)
        past = _fused(attn, K0, V0)
        outs = []
        for q, k, v in steps:
            o, past = attn.decode_fused(q, k, v, past, defer_trigger=True)
            if attn.trigger_due(past):
                past = attn.run_triggers([past])[0]
            outs.append(o)
        assert len(past[2].extents) == 1 and past[2].value_lists == lists and not any(e.value_lists for e in past[2].extents)
        assert _form() == FORM_SB
        res[lists] = (outs, past)
    for i, (a, b) in enumerate(zip(res[True][0], res[False][0])):
        assert excess(a, b, NATIVE_ULPS) <= 1.0, f"step {i}"
    assert res[True][1][2].bytes_in_use() > 0
    a, b = res[True][1][2].to_reference(), res[False][1][2].to_reference()   # (retiles the base back: the whole cache in the reference layout)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(torch.cat(list(a[2])), torch.cat(list(b[2])))
    res[True][1][2].drop_extents()
    assert res[True][1][2].total_tokens == T


def test_graphs_over_a_base_in_lists_device_t_capture_ahead_and_alternating_replays(tbw):
    bsz, hkv, hq, T = 1, 2, 8, 512
    K0, V0, steps = _inputs(22, bsz, hq, hkv, T, w=253, steps=3)
    attn, tiles = _attn(hq, hkv, engine="dot2"), _attn(hq, hkv, engine="dot2", value_lists=False)
    past, past_t = _fused(attn, K0, V0), _fused(tiles, K0, V0)
    assert past[2].value_lists and not past_t[2].value_lists
    # ONE graph with a device-side T, recorded ahead of the trigger over the current base (EXT instantiation, capacity T + 256)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    t_dev = torch.full((1,), T, dtype=torch.int32, device=DEV)
    gq, gk, gv = (x.clone() for x in steps[0])
    attn.decode_fused(gq, gk, gv, (past[0], past[1].clone(), past[2], past[3].clone(), past[4], past[5]))   # scratch outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g_out, _ = attn.decode_fused(gq, gk, gv, past, step_counter=counter, t_device=t_dev, t_capacity=T + 256)
    assert past[2].value_lists, "a capture leaves the lists alone"
    # 34 replays with two alternating queries on one scratch (no stale e), against eager calls over the tile arena
    qa, qb = steps[1][0], steps[2][0]
    want = {}
    for name, qq in (("a", qa), ("b", qb)):
        want[name] = tiles.decode_fused(qq, gk, gv, (past_t[0], past_t[1].clone(), past_t[2], past_t[3].clone(), past_t[4], past_t[5]))[0]
    for i in range(34):
        name, qq = ("a", qa) if i % 2 == 0 else ("b", qb)
        gq.copy_(qq)
        counter.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert excess(g_out, want[name], NATIVE_ULPS) <= 1.0, f"replay {i}"
    # the trigger fires: the same graph reads the extent (tiles) behind the base (lists)
    past = attn.advance(past, 1)
    o_t, past_t2 = tiles.decode_fused(gq, gk, gv, past_t, defer_trigger=True)
    for q, k, v in steps[1:]:
        counter.fill_(past[1].len - (R + 253))
        gq.copy_(q); gk.copy_(k); gv.copy_(v)
        g.replay()
        past = attn.advance(past, 1)
        o_t, past_t2 = tiles.decode_fused(q, k, v, past_t2, defer_trigger=True)
        torch.cuda.synchronize()
        assert excess(g_out, o_t, NATIVE_ULPS) <= 1.0
    assert attn.trigger_due(past) and tiles.trigger_due(past_t2)
    past = attn.run_triggers([past])[0]
    past_t2 = tiles.run_triggers([past_t2])[0]
    assert len(past[2].extents) == 1 and past[2].value_lists
    t_dev.fill_(T + 256)
    counter.fill_(past[1].len - (R + 253))
    q, k, v = steps[0]
    gq.copy_(q); gk.copy_(k); gv.copy_(v)
    g.replay()
    o_t, _ = tiles.decode_fused(q, k, v, past_t2, defer_trigger=True)
    torch.cuda.synchronize()
    assert excess(g_out, o_t, NATIVE_ULPS) <= 1.0


# ---- 4. fallbacks ------------------------------------------------------------------------------------------------------------------
def test_whatever_needs_tiles_retiles_back_once_and_gives_the_tile_arenas_results(tbw):
    from mustafar_amd import partial
    bsz, hkv, hq, T = 1, 2, 8, 512
    K0, V0, [(q, k, v)] = _inputs(31, bsz, hq, hkv, T)
    attn, tiles = _attn(hq, hkv, engine="dot2"), _attn(hq, hkv, engine="dot2", key_rows=False, value_lists=False)
    # to_reference()
    p, pt = _fused(attn, K0, V0), _fused(tiles, K0, V0)
    assert p[2].value_lists and not pt[2].value_lists
    a, b = p[2].to_reference(), pt[2].to_reference()
    assert not p[2].value_lists and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(torch.cat(list(a[2])), torch.cat(list(b[2])))
    # consolidate() returns a tile arena; the next to_fused() may retile it again
    p = _fused(attn, K0, V0)
    c = p[2].consolidate()
    assert c is p[2] and not c.value_lists
    assert attn.to_fused(p)[2].value_lists
    # decode_multi (the multi-query entry point reads tiles)
    p, pt = _fused(attn, K0, V0), _fused(tiles, K0, V0)
    g = torch.Generator(device="cpu").manual_seed(5)
    q2 = torch.randn(bsz, hq, 2, 128, generator=g).half().to(DEV)
    k2, v2 = torch.randn(bsz, hkv, 2, 128, generator=g).half().to(DEV), torch.randn(bsz, hkv, 2, 128, generator=g).half().to(DEV)
    om, _ = attn.decode_multi(q2, k2, v2, p)
    ot, _ = tiles.decode_multi(q2, k2, v2, pt)
    assert not p[2].value_lists and p[2].keep_tiles and torch.equal(om, ot)
    assert not attn.to_fused(p)[2].value_lists, "once retiled back, the arena stays in tiles"
    # the shared-segment entry point reads tiles
    p, pt = _fused(attn, K0, V0), _fused(tiles, K0, V0)
    q3 = torch.randn(3, hq, 1, 128, generator=torch.Generator(device="cpu").manual_seed(6)).half().to(DEV)
    s1 = partial.SharedSegment(p[0], p[2], T, hkv).decode(attn, q3)
    s2 = partial.SharedSegment(pt[0], pt[2], T, hkv).decode(tiles, q3)
    assert not p[2].value_lists
    for a, b in zip(s1, s2):
        assert torch.equal(a, b)
    # a per-sequence segment runs the same launch: it reads the lists
    p, pt = _fused(attn, K0, V0), _fused(tiles, K0, V0)
    o1 = attn.decode_segment(q, p[0], p[2], T)
    o2 = tiles.decode_segment(q, pt[0], pt[2], T)
    assert p[2].value_lists and _form() == FORM_SB and excess(o1[0], o2[0], NATIVE_ULPS) <= 1.0
    # an engine switch to the matrix pipe on a lists arena: retiled back, the tile arena's bits
    attn.cfg.engine = tiles.cfg.engine = "mfma"
    o1, _ = attn.decode_fused(q, k, v, p)
    o2, _ = tiles.decode_fused(q, k, v, pt)
    assert not p[2].value_lists and torch.equal(o1, o2)


def test_refusals_under_capture_and_at_the_c_boundary(tbw):
    bsz, hkv, hq, T = 1, 2, 8, 512
    K0, V0, [(q, k, v)] = _inputs(33, bsz, hq, hkv, T)
    attn = _attn(hq, hkv, engine="dot2", key_rows=False)
    p = _fused(attn, K0, V0)
    assert p[2].value_lists and not p[0].key_rows
    attn.decode_fused(q, k, v, (p[0], p[1].clone(), p[2], p[3].clone(), p[4], p[5]))   # scratch outside the capture
    attn.cfg.engine = "mfma"
    attn.decode_fused(q, k, v, _fused(_attn(hq, hkv, engine="mfma"), K0, V0))            # (the matrix pipe's scratch too)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="require_tiles"):
        with torch.cuda.graph(g):
            attn.decode_fused(q, k, v, p, step_counter=counter)
    assert p[2].value_lists
    # direct C calls of entry points that do not read lists
    L, lib = _lib().load(), _lib()
    other = _fused(_attn(hq, hkv, engine="dot2", key_rows=False, value_lists=False), K0, V0)
    assert L.mustafar_cache_rehouse(None, p[2].view_ptr(), other[2].view_ptr(), p[2].heads, T, 0) == 1
    lse = torch.empty(hq, dtype=torch.float32, device=DEV)
    ws = torch.empty(L.mustafar_shared_segment_workspace_bytes(T, hkv, 4, 1, 128), dtype=torch.uint8, device=DEV)
    out = torch.empty_like(q)
    assert L.mustafar_decode_shared_segment(None, other[0].view_ptr(), p[2].view_ptr(), T, hkv, 4, 1, q.data_ptr(), out.data_ptr(),
                                            lse.data_ptr(), ws.data_ptr(), 128 ** 0.5, 128) == 1
    assert lib.VIEW_VALUE_LISTS == p[2].view.flags and ctypes.sizeof(lib.CacheView) == p[2].VIEW_BYTES


# ---- 5. off ------------------------------------------------------------------------------------------------------------------------
def test_value_lists_off_by_config_and_by_environment(tbw, monkeypatch):
    bsz, hkv, hq, T = 1, 2, 8, 512
    K0, V0, [(q, k, v)] = _inputs(41, bsz, hq, hkv, T)
    off = _attn(hq, hkv, engine="dot2", value_lists=False)
    p = _fused(off, K0, V0)
    o_off, _ = off.decode_fused(q, k, v, p)
    assert not p[2].value_lists and p[0].key_rows and _form() == FORM_SB
    monkeypatch.setenv("MUSTAFAR_VALUE_LISTS", "0")
    env = _attn(hq, hkv, engine="dot2")
    p = _fused(env, K0, V0)
    o_env, _ = env.decode_fused(q, k, v, p)
    assert not p[2].value_lists and _form() == FORM_SB and torch.equal(o_env, o_off)
    monkeypatch.delenv("MUSTAFAR_VALUE_LISTS")
    assert _fused(_attn(hq, hkv, engine="dot2"), K0, V0)[2].value_lists
    # where the launch form does not read lists nothing is retiled either: MHA, the matrix pipe, two blocks per workgroup, the default rule
    assert not _fused(_attn(8, 8), K0.repeat(1, 4, 1, 1), V0.repeat(1, 4, 1, 1))[2].value_lists
    assert not _fused(_attn(hq, hkv, engine="mfma"), K0, V0)[2].value_lists
    _lib().load().mustafar_tune(1, 1)
    assert not _fused(_attn(hq, hkv, engine="dot2"), K0, V0)[2].value_lists
    _lib().load().mustafar_tune(1, 0)
    assert not _fused(_attn(hq, hkv, engine="dot2"), K0, V0)[2].value_lists
