"""GPU: nibble-row key blocks (include/mustafar_hip.h: MUSTAFAR_VIEW_KEY_NIBBLE_ROWS).

`MustafarAttention.to_fused()` retiles the key BASE of an arena into token rows with 4-bit channel steps where the launch reads them and
the value base took the lists over pairs of blocks.  Held here, at Hq 8, Hkv 2, batch 2, D = 128, four blocks per workgroup
(mustafar_tune(1, 2), as tests/test_gpu_key_rows.py), windows of 40 rows:
  1. the device retile, both directions, against tests/key_nibble_rows_ref.py byte for byte and bit for bit back to tiles: the special
     blocks (kept +0 / -0 among them), bases of 1, 5, 9 and 65 blocks, two heads of unequal size;
  2. fused decode at T = 256 (one workgroup of four blocks) and T = 320 (a last workgroup of one block), both vector engines, with and
     without a mask: against a float64 dense model within the suite's fp16 bound, and against the same call on the rows with channel bytes;
     bit-equal to the tile path on exactly representable data; the special blocks as K;
  3. growth: an extent in tiles behind a base in nibble rows, one graph with a device-side T across a trigger;
  4. the negative control: a corrupted step row fails the comparison;
  5. what keeps tiles or the rows with channel bytes: the matrix pipe, G != 4, two blocks per workgroup, the knobs."""
import math

import numpy as np
import pytest
import torch

import key_nibble_rows_ref as ref
from oracle import oracle as orc
from tests import exact_data as xd
from tests.util import DENSE_ULPS, NATIVE_ULPS, excess

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 32
W = 8           # rows of the window beyond R: 40 in all
FORM_SB = 3
HQ, HKV, BSZ = 8, 2, 2


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


def _attn(form="nibble", hq=HQ, hkv=HKV, **kw):
    """form: "nibble" (key_nibble_rows=True: at every size; the default takes the form from hook.NIBBLE_ROWS_FROM tokens on), "rows"
    (key_nibble_rows=False: channel bytes), "tiles" (no base form on either side)."""
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    knobs = {"nibble": dict(key_nibble_rows=True), "rows": dict(key_nibble_rows=False), "tiles": dict(key_rows=False, value_lists=False)}[form]
    return MustafarAttention(MustafarConfig(num_attention_heads=hq, num_key_value_heads=hkv, k_sparsity=0.7, v_sparsity=0.7, api="fused",
                                            arena=True, **dict(knobs, **kw)))


def _is(past, form):
    k, v = past[0], past[2]
    return {"nibble": k.key_nibble_rows and k.key_rows and v.value_pair_lists, "rows": k.key_rows and not k.key_nibble_rows and v.value_pair_lists,
            "tiles": not k.key_rows and not k.key_nibble_rows and not v.value_lists}[form]


def _inputs(seed, T, w=W, steps=1, bsz=BSZ, hq=HQ, hkv=HKV):
    g = torch.Generator(device="cpu").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g).half().to(DEV)
    K0, V0 = rnd(bsz, hkv, T + R + w, 128), rnd(bsz, hkv, T + R + w, 128)
    return K0, V0, [(rnd(bsz, hq, 1, 128), rnd(bsz, hkv, 1, 128), rnd(bsz, hkv, 1, 128)) for _ in range(steps)]


def _past(attn, K0, V0, T, kp=None):
    """A cache of T tokens (any multiple of 64) from pruned rows (kp: the pruned K rows [B x Hkv, T, 128]), the rest of K0 / V0 as the window."""
    from mustafar_amd.cache import CompressedArena
    from mustafar_amd.hook import Past
    B = K0.shape[0] * K0.shape[1]
    if kp is None:
        kp = attn.dh_prune_key(K0[:, :, :T]).reshape(B, T, 128)
    vp = attn.dh_prune_value(V0[:, :, :T]).reshape(B, T, 128)
    return attn.to_fused(Past(CompressedArena.from_pruned(kp.clone(), "key"), K0[:, :, T:].clone(), CompressedArena.from_pruned(vp, "value"),
                              V0[:, :, T:].clone(), T, K0.shape[2]))


def _form():
    return (_lib().load().mustafar_last_decode_choice() >> 8) & 15


def _window(p):
    return (p[0], p[1].clone(), p[2], p[3].clone(), p[4], p[5])


def _dense64(q, k, v, K0, V0, T, kp=None, mask=None):
    """softmax(q K^T / sqrt(d)) V in float64 over the pruned first T tokens, the window and the step's own row."""
    prune = lambda x: torch.from_numpy(orc.prune_magnitude(x.cpu().numpy(), 0.7)).to(DEV)
    Kp = prune(K0[:, :, :T]) if kp is None else kp.reshape(K0.shape[0], K0.shape[1], T, 128)
    K = torch.cat([Kp, K0[:, :, T:], k], dim=2).double().repeat_interleave(HQ // HKV, dim=1)
    V = torch.cat([prune(V0[:, :, :T]), V0[:, :, T:], v], dim=2).double().repeat_interleave(HQ // HKV, dim=1)
    s = torch.matmul(q.double(), K.transpose(2, 3)) / math.sqrt(128.0)
    if mask is not None:
        s = s + mask.double()
    return torch.matmul(torch.softmax(s, -1), V)


# ---- 1. retile round trip ----------------------------------------------------------------------------------------------------------
def _special_arena(blocks):
    """A key arena over the first `blocks` blocks of ref.special_heads(), its kept zeros written into the stream as +0 / -0."""
    from mustafar_amd.cache import CompressedArena
    vals, kept = ref.special_heads()
    vals, kept = vals[:, :64 * blocks], kept[:, :64 * blocks]
    x = vals.copy()
    x[kept & ((vals & 0x7FFF) == 0)] = 0x3C00   # (a zero is not kept by from_pruned: a one stands in, and the stream is patched below)
    a = CompressedArena.from_pruned(torch.from_numpy(x.view(np.float16)).to(DEV), "key")
    idx, bmp = a.idx.cpu().numpy().view(np.uint32), a.bmp.cpu().numpy().view(np.uint64)
    for h in range(2):
        at, bits = [], []
        for t, d in zip(*np.nonzero(kept[h] & ((vals[h] & 0x7FFF) == 0))):
            tile, tok = (t // 64) * 128 + d, int(t % 64)
            m = int(bmp[h, tile])
            at.append(2 * int(idx[h, tile]) + (bin(m >> (64 - tok)).count("1") if tok else 0))
            bits.append(int(vals[h, t, d]) - (65536 if vals[h, t, d] >= 32768 else 0))
        if at:
            a.nz.view(torch.int16)[h, torch.tensor(at, device=DEV)] = torch.tensor(bits, dtype=torch.int16, device=DEV)
    return a


@pytest.mark.parametrize("data", ["special_1", "special_5", "special_9", "special_4160"])
def test_retile_round_trip_is_bit_exact_and_nibble_rows_equal_the_reference(data):
    from mustafar_amd.cache import CompressedArena
    from tests.test_gpu_key_rows import _special
    if data == "special_4160":   # the 65-block case of the existing round trips: a second trip of the table scan
        x = _special(4160)
        a = CompressedArena.from_pruned(torch.from_numpy(x).to(DEV), "key")
    else:
        a = _special_arena(int(data.split("_")[1]))
    H, T = a.heads, a.tokens
    base = a.to_reference()
    bmp0, idx0, nz0 = base[0].clone(), base[1].clone(), [s.clone() for s in base[2]]
    table, rows = ref.tiles_to_rows(bmp0.cpu().numpy().view(np.uint64), idx0.cpu().numpy().view(np.uint32),
                                    [s.cpu().numpy().view(np.uint16) for s in nz0], T)
    if data == "special_9":
        assert rows[0].size != rows[1].size and sorted(set((table[0] & 0xFF).tolist())) == [2, 4, 40, 42, 44, 46, 64, 128]
        assert any((s.view(torch.int16) == -32768).any() for s in nz0), "a kept -0 is in the stream"
    assert a.to_key_nibble_rows() and a.key_nibble_rows and a.key_rows and a.bmp.numel() == 0
    assert not a.to_key_rows() and a.key_nibble_rows, "one form at a time"
    assert np.array_equal(a.idx.cpu().numpy().view(np.uint32), table)
    got = a.nz.cpu().numpy().view(np.uint8)
    for h in range(H):
        assert np.array_equal(got[h, :rows[h].size], rows[h]), f"rows of head {h}"
    assert a.bytes_in_use() == H * (T // 64) * 4 + sum(r.size for r in rows)
    a.require_tiles()
    assert not a.key_rows and not a.key_nibble_rows
    back = a.to_reference()
    assert torch.equal(back[0], bmp0) and torch.equal(back[1], idx0)
    for h in range(H):
        assert torch.equal(back[2][h].view(torch.int16), nz0[h].view(torch.int16)), f"stream of head {h}"
    a.keep_tiles = False
    assert a.to_key_rows() and a.key_rows and not a.key_nibble_rows   # to_key_rows() still gives the rows with channel bytes
    v = CompressedArena.from_pruned(torch.from_numpy(_special(256)).to(DEV), "value")
    assert not v.to_key_nibble_rows() and v.form is None, "a value arena does not take the form"


# ---- 2. decode parity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "mask"])
@pytest.mark.parametrize("engine", ["valu", "dot2"])
@pytest.mark.parametrize("T", [256, 320])
def test_decode_with_nibble_rows_against_the_dense_model_and_the_rows_with_channel_bytes(tbw, T, engine, masked):
    K0, V0, [(q, k, v)] = _inputs(T + 3, T)
    mask = None
    if masked:
        from tests.test_gpu_mask import _left_padding_mask
        mask = _left_padding_mask(BSZ, T + R + W + 1, [0, 37])
    want = _dense64(q, k, v, K0, V0, T, mask=mask)
    outs = {}
    for form in ("nibble", "rows"):
        attn = _attn(form, engine=engine)
        past = _past(attn, K0, V0, T)
        assert _is(past, form), form
        outs[form], _ = attn.decode_fused(q, k, v, past, attention_mask=mask, defer_trigger=True)
        assert _form() == FORM_SB and _is(past, form), "the super-block kernel ran and left the form alone"
        print(f"T {T} {engine} mask {masked} {form}: excess over the dense model {excess(outs[form], want, DENSE_ULPS):.3f}")
        assert excess(outs[form], want, DENSE_ULPS) <= 1.0, form
    print(f"nibble rows against rows: {excess(outs['nibble'], outs['rows'], NATIVE_ULPS):.3f}")
    assert excess(outs["nibble"], outs["rows"], NATIVE_ULPS) <= 1.0


def test_exact_data_gives_bit_equal_outputs_with_the_tile_path(tbw):
    """K and q of small dyadic integers: every product and every partial sum of a score is exact in fp32, so neither the order of the sum
    nor the direction of a chain matters, and the scores are the same bits -- and with them everything behind (the value side: pair lists
    against pair lists)."""
    T = 320
    rng = np.random.default_rng(3)
    K0 = torch.from_numpy(xd.dyadic(rng, (BSZ, HKV, T + R + W, 128), 3, 2)).to(DEV)
    q = torch.from_numpy(xd.dyadic(rng, (BSZ, HQ, 1, 128), 3, 2)).to(DEV)
    _, V0, [(_, k, v)] = _inputs(4, T)
    outs = {}
    for form, knobs in (("nibble", {}), ("tile keys", dict(key_rows=False, key_nibble_rows=None))):
        attn = _attn(engine="valu", **knobs)
        past = _past(attn, K0, V0, T)
        if form == "tile keys":   # (with key rows off to_fused() takes the lists per block: pair lists are asked for, so that only K differs)
            past[2].require_tiles(sticky=False)
            assert past[2].to_value_pair_lists()
        assert past[0].key_nibble_rows == (form == "nibble") and past[0].key_rows == (form == "nibble") and past[2].value_pair_lists
        outs[form], _ = attn.decode_fused(q, k, v, past, defer_trigger=True)
        assert _form() == FORM_SB
    assert torch.equal(outs["nibble"], outs["tile keys"])


def test_the_special_blocks_as_k(tbw):
    """The special blocks as the key cache at T = 320: widths 128, 64, 4, 2 and 40 .. 46, chains with spacers in both directions, long
    padding, an empty back share -- four heads of different blocks."""
    T = 320
    vals, _ = ref.special_heads()
    heads = [vals[0, :T], vals[1, :T], vals[0, 256:256 + T], vals[1, 128:128 + T]]
    kp = torch.from_numpy(np.stack(heads).view(np.float16)).to(DEV)
    K0, V0, [(q, k, v)] = _inputs(9, T)
    want = _dense64(q, k, v, K0, V0, T, kp=kp)
    outs = {}
    for form in ("nibble", "tiles"):
        attn = _attn(form, engine="valu")
        past = _past(attn, K0, V0, T, kp=kp)
        assert _is(past, form)
        outs[form], _ = attn.decode_fused(q, k, v, past, defer_trigger=True)
        assert _form() == FORM_SB and excess(outs[form], want, DENSE_ULPS) <= 1.0, form
    assert excess(outs["nibble"], outs["tiles"], NATIVE_ULPS) <= 1.0


# ---- 3. growth ---------------------------------------------------------------------------------------------------------------------
def test_an_extent_in_tiles_behind_a_base_in_nibble_rows_across_a_trigger(tbw):
    T = 512
    K0, V0, steps = _inputs(21, T, w=250, steps=6 + 3, bsz=1)
    res = {}
    for form in ("nibble", "tiles"):
        attn = _attn(form, engine="dot2")
        past = attn.to_fused(attn.build_cache(K0.clone(), V0.clone()))
        outs = []
        for q, k, v in steps:
            o, past = attn.decode_fused(q, k, v, past, defer_trigger=True)
            if attn.trigger_due(past):
                past = attn.run_triggers([past])[0]
            outs.append(o)
        assert len(past[0].extents) == 1 and _is(past, form) and not any(e.key_rows for e in past[0].extents)
        assert _form() == FORM_SB
        res[form] = (outs, past)
    for i, (a, b) in enumerate(zip(res["nibble"][0], res["tiles"][0])):
        assert excess(a, b, NATIVE_ULPS) <= 1.0, f"step {i}"
    a, b = res["nibble"][1][0].to_reference(), res["tiles"][1][0].to_reference()   # (retiles the base back: the whole cache in the reference layout)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(torch.cat(list(a[2])), torch.cat(list(b[2])))


def test_one_graph_with_a_device_side_t_across_a_trigger(tbw):
    T = 512
    K0, V0, steps = _inputs(22, T, w=253, steps=3, bsz=1)
    attn, tiles = _attn(engine="dot2"), _attn("tiles", engine="dot2")
    past, past_t = attn.to_fused(attn.build_cache(K0.clone(), V0.clone())), tiles.to_fused(tiles.build_cache(K0.clone(), V0.clone()))
    assert _is(past, "nibble") and _is(past_t, "tiles")
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    t_dev = torch.full((1,), T, dtype=torch.int32, device=DEV)
    gq, gk, gv = (x.clone() for x in steps[0])
    attn.decode_fused(gq, gk, gv, _window(past))   # scratch outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g_out, _ = attn.decode_fused(gq, gk, gv, past, step_counter=counter, t_device=t_dev, t_capacity=T + 256)
    assert past[0].key_nibble_rows, "a capture leaves the rows alone"
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
    assert len(past[0].extents) == 1 and past[0].key_nibble_rows
    t_dev.fill_(T + 256)
    counter.fill_(past[1].len - (R + 253))
    q, k, v = steps[0]
    gq.copy_(q); gk.copy_(k); gv.copy_(v)
    g.replay()
    o_t, _ = tiles.decode_fused(q, k, v, past_t, defer_trigger=True)
    torch.cuda.synchronize()
    assert excess(g_out, o_t, NATIVE_ULPS) <= 1.0


# ---- 4. the negative control -------------------------------------------------------------------------------------------------------
def test_a_corrupted_step_row_fails_the_comparison(tbw):
    """q is key token 7, so that token carries most of the weight without drowning the rest (a score near 7 against scores near 0); the
    first step row of block 0's front share is overwritten with steps of one: the first eight values of every token -- a fifth of token
    7's score -- meet the channels 0 .. 7 of q instead of their own, and every position behind them shifts."""
    T = 256
    K0, V0, [(q, k, v)] = _inputs(51, T, bsz=1)
    q = K0[:, :, 7:8].repeat_interleave(HQ // HKV, dim=1).contiguous()
    attn, tiles = _attn(engine="valu"), _attn("tiles", engine="valu")
    want, _ = tiles.decode_fused(q, k, v, _past(tiles, K0, V0, T), defer_trigger=True)
    past = _past(attn, K0, V0, T)
    good, _ = attn.decode_fused(q, k, v, _window(past), defer_trigger=True)
    assert excess(good, want, NATIVE_ULPS) <= 1.0
    arena = past[0]
    assert arena.key_nibble_rows and int(arena.idx[0, 0]) >> 8 == 0
    raw = arena.nz.view(torch.uint8)
    raw[0, :256] = 0x11   # head 0, block 0, front share, step row 0: all 64 tokens
    bad, _ = attn.decode_fused(q, k, v, _window(past), defer_trigger=True)
    assert arena.key_nibble_rows and _form() == FORM_SB
    assert excess(bad, want, NATIVE_ULPS) > 1.0, "the comparison does not see wrong channels"


# ---- 5. what keeps tiles or the rows with channel bytes ------------------------------------------------------------------------------
def test_other_engines_groups_and_launch_shapes_keep_tiles_or_the_rows_with_channel_bytes(tbw, monkeypatch):
    T = 256
    K0, V0, [(q, k, v)] = _inputs(5, T)
    fused = lambda attn, K=K0, V=V0: attn.to_fused(attn.build_cache(K.clone(), V.clone()))
    assert _is(fused(_attn(engine="dot2")), "nibble")
    p = fused(_attn(engine="mfma"))                                    # the matrix pipe
    assert not p[0].key_rows and not p[0].key_nibble_rows
    p = fused(_attn(hq=8, hkv=8), K0.repeat(1, 4, 1, 1), V0.repeat(1, 4, 1, 1))   # MHA: G = 1
    assert not p[0].key_rows and not p[0].key_nibble_rows
    p = fused(_attn(hq=8, hkv=4), K0.repeat(1, 2, 1, 1), V0.repeat(1, 2, 1, 1))   # GQA-2
    assert not p[0].key_rows and not p[0].key_nibble_rows
    assert _is(fused(_attn("rows", engine="dot2")), "rows")              # key_nibble_rows=False: channel bytes
    p = fused(_attn(engine="dot2", value_pair_lists=False))            # no pair lists: channel bytes next to the lists per block
    assert p[0].key_rows and not p[0].key_nibble_rows and p[2].value_lists and not p[2].value_pair_lists
    monkeypatch.setenv("MUSTAFAR_KEY_NIBBLE_ROWS", "0")
    assert _is(fused(_attn(engine="dot2")), "rows")
    monkeypatch.delenv("MUSTAFAR_KEY_NIBBLE_ROWS")
    # the default: by size
    from mustafar_amd.hook import MustafarAttention
    auto = _attn(engine="dot2", key_nibble_rows=None)
    assert _is(fused(auto), "rows") and T < MustafarAttention.NIBBLE_ROWS_FROM
    monkeypatch.setattr(MustafarAttention, "NIBBLE_ROWS_FROM", T)
    assert _is(fused(auto), "nibble")
    # a value base that went back to tiles: the key base follows at the next call, and the result is the tile arenas'
    attn = _attn(engine="dot2")
    p = fused(attn)
    p[2].require_tiles()
    o, _ = attn.decode_fused(q, k, v, _window(p))
    assert not p[0].key_nibble_rows and _form() == FORM_SB
    tiles = _attn("tiles", engine="dot2")
    o_t, _ = tiles.decode_fused(q, k, v, fused(tiles))
    assert excess(o, o_t, NATIVE_ULPS) <= 1.0
    # two blocks per workgroup: the launch reads no base form
    assert _lib().load().mustafar_tune(1, 1) == 0
    p = fused(_attn(engine="dot2"))
    assert not p[0].key_rows and not p[0].key_nibble_rows
