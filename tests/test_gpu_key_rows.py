"""GPU: token-row key blocks (ABI 113; include/mustafar_hip.h: MUSTAFAR_VIEW_KEY_ROWS).

`MustafarAttention.to_fused()` retiles the key BASE of an arena into token rows where the launch of the call shape reads them (the GQA-4
one-pass super-block kernel on the two vector engines); everything else gets tiles back through `CompressedArena.require_tiles()`.
Held here, all at G = 4, D = 128, one or two kv heads, batch 1-2, T in {256, 512, 1280} at four blocks per workgroup (mustafar_tune(1, 2):
the shapes are far below the size at which the default shape rule picks that launch; a launch of TWO blocks per workgroup measured slower
on rows and keeps tiles, which section 5 holds), and T = 320 / 448 for workgroups with one and three blocks:
  1. the device retile, both directions, against tests/key_rows_ref.py and bit for bit back to the base arrays;
  2. decode parity: key_rows on against key_rows off and against the native two-call sequence, both engines, mask, LSE; bit-equal
     outputs on data whose scores are exact;
  3. growth: extents in tiles behind a base in rows, a graph with a device-side T, a graph recorded ahead of the trigger, 34 replays
     with alternating queries;
  4. fallbacks: multi-query, shared segment, to_reference(), consolidate(), an engine switch -- and the refusals;
  5. MUSTAFAR_KEY_ROWS=0 / key_rows=False: nothing is retiled."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import key_rows_ref as ref
from oracle import oracle as orc
from tests import exact_data as xd
from tests.util import NATIVE_ULPS, excess

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 32
FORM_SB = 3


def _lib():
    from mustafar_amd import _lib as lib
    return lib


@pytest.fixture(params=[2], ids=["four_blocks_per_wg"])
def tbw(request):
    """The super-block kernel at small shapes: mustafar_tune(1, n) gives a workgroup n block pairs (and keeps the small form out).  Rows are
    read at four blocks per workgroup only (mustafar_decode_reads_key_rows)."""
    L = _lib().load()
    assert L.mustafar_tune(1, request.param) == 0
    yield request.param
    L.mustafar_tune(1, 0)


def _attn(hq, hkv, api="fused", arena=True, **kw):
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    return MustafarAttention(MustafarConfig(num_attention_heads=hq, num_key_value_heads=hkv, k_sparsity=0.7, v_sparsity=0.7, api=api,
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
def _special(T):
    rng = np.random.default_rng(T)
    x = orc.prune_magnitude(rng.standard_normal((2, T, 128)).astype(np.float16), 0.7)
    x[0, 3] = 0                                    # an all-zero token
    x[0, 10] = 0
    x[0, 10, :42] = np.float16(1.5)                # 42 kept channels, what a magnitude tie leaves: w = 42
    x[1, 70, 1:] = 0                               # a row that keeps 1 channel ...
    x[1, 71] = np.float16(2.5)                     # ... beside one that keeps 128: w = 128
    x[1, 128:192] = 0                              # an all-zero block: w = 2
    return x


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "compress_reference.npz"))["rand_B2_t256_s0.7__x"].view(np.float16)


@pytest.mark.parametrize("data", ["special_256", "special_1280", "special_4160", "golden"])   # 4160: 65 blocks, a second trip of the table scan
def test_retile_round_trip_is_bit_exact_and_rows_equal_the_reference(data, golden_dir):
    from mustafar_amd.cache import CompressedArena
    x = _golden(golden_dir) if data == "golden" else _special(int(data.split("_")[1]))
    H, T = x.shape[0], x.shape[1]
    a = CompressedArena.from_pruned(torch.from_numpy(x).to(DEV), "key")
    base = a.to_reference()
    bmp0, idx0, nz0 = base[0].clone(), base[1].clone(), [s.clone() for s in base[2]]
    table, rows = ref.tiles_to_rows(bmp0.cpu().numpy().view(np.uint64), idx0.cpu().numpy().view(np.uint32),
                                    [s.cpu().numpy().view(np.uint16) for s in nz0], T)
    if data != "golden":
        w = table & 0xFF
        assert w[0, 0] == 42 and w[1, 1] == 128 and w[1, 2] == 2
    before = a.bytes_in_use()
    assert a.to_key_rows() and a.key_rows and a.bmp.numel() == 0
    assert np.array_equal(a.idx.cpu().numpy().view(np.uint32), table)
    got = a.nz.cpu().numpy().view(np.uint8)
    for h in range(H):
        assert np.array_equal(got[h, :rows[h].size], rows[h]), f"rows of head {h}"
    assert a.bytes_in_use() == H * (T // 64) * 4 + sum(r.size for r in rows) and before > 0
    a.require_tiles()
    assert not a.key_rows
    back = a.to_reference()
    assert torch.equal(back[0], bmp0) and torch.equal(back[1], idx0)
    for h in range(H):
        assert torch.equal(back[2][h].view(torch.int16), nz0[h].view(torch.int16)), f"stream of head {h}"
    a.require_tiles()   # (nothing to do)


# ---- 2. decode parity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["valu", "dot2"])
@pytest.mark.parametrize("bsz,hkv,T", [(1, 2, 256), (2, 1, 512), (2, 2, 1280)])
def test_decode_with_key_rows_equals_tiles_and_the_native_sequence(tbw, engine, bsz, hkv, T):
    hq = 4 * hkv
    K0, V0, [(q, k, v)] = _inputs(T + tbw, bsz, hq, hkv, T)
    outs = {}
    for rows in (True, False):
        attn = _attn(hq, hkv, engine=engine, key_rows=rows)
        past = _fused(attn, K0, V0)
        assert past[0].key_rows == rows
        o, _ = attn.decode_fused(q, k, v, past)
        assert _form() == FORM_SB and past[0].key_rows == rows, "the super-block kernel ran and left the form alone"
        outs[rows] = o
    native = _attn(hq, hkv, api="native", arena=False)
    want, _ = native.decode(q, k, v, native.build_cache(K0.clone(), V0.clone()))
    for rows in (True, False):
        assert excess(outs[rows], want, NATIVE_ULPS) <= 1.0, (rows, excess(outs[rows], want, NATIVE_ULPS))
    assert excess(outs[True], outs[False], NATIVE_ULPS) <= 1.0


@pytest.mark.parametrize("engine", ["valu", "dot2"])
def test_mask_and_lse_with_key_rows(tbw, engine):
    from tests.test_gpu_mask import _left_padding_mask
    bsz, hkv, hq, T = 2, 2, 8, 512
    K0, V0, [(q, k, v)] = _inputs(11, bsz, hq, hkv, T)
    kv_len = T + R + 40 + 1
    mask = _left_padding_mask(bsz, kv_len, [0, 37])
    res = {}
    for rows in (True, False):
        attn = _attn(hq, hkv, engine=engine, key_rows=rows)
        past = _fused(attn, K0, V0)
        assert past[0].key_rows == rows
        o_m, _ = attn.decode_fused(q, k, v, _fused(attn, K0, V0), attention_mask=mask)
        o, lse, _ = attn.decode_fused(q, k, v, past, return_lse=True)
        assert _form() == FORM_SB
        res[rows] = (o_m, o, lse)
    assert excess(res[True][0], res[False][0], NATIVE_ULPS) <= 1.0 and excess(res[True][1], res[False][1], NATIVE_ULPS) <= 1.0
    # the LSE: fp32 of fp16 scores; rows and tiles differ by the fp16 rounding of a score at most (2^-11 relative, scores of a few units)
    torch.testing.assert_close(res[True][2], res[False][2], rtol=0, atol=2.0 ** -8)


def test_exact_scores_give_bit_equal_outputs_on_the_exact_engine(tbw):
    """K and q of small dyadic integers: every product and every partial sum of a score is exact in fp32, so the order of the sum does
    not matter and the scores of the two key phases are the same bits -- and with them everything behind."""
    bsz, hkv, hq, T = 2, 2, 8, 512
    rng = np.random.default_rng(3)
    K0 = torch.from_numpy(xd.dyadic(rng, (bsz, hkv, T + R + 8, 128), 3, 2)).to(DEV)
    q = torch.from_numpy(xd.dyadic(rng, (bsz, hq, 1, 128), 3, 2)).to(DEV)
    _, V0, [(_, k, v)] = _inputs(4, bsz, hq, hkv, T, w=8)
    outs = []
    for rows in (True, False):
        attn = _attn(hq, hkv, engine="valu", key_rows=rows)
        past = _fused(attn, K0, V0)
        assert past[0].key_rows == rows
        outs.append(attn.decode_fused(q, k, v, past)[0])
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("engine", ["valu", "dot2"])
@pytest.mark.parametrize("T", [320, 448])
def test_workgroups_with_an_odd_number_of_blocks(tbw, engine, T):
    """5 and 7 blocks at four per workgroup: the last workgroup holds one block (one pair idle, the other with a lone block A) or three (a
    pair with a lone block).  The hook compresses in 256-token steps, so the arenas are made directly."""
    from mustafar_amd.cache import CompressedArena
    from mustafar_amd.hook import Past
    bsz, hkv, hq = 1, 2, 8
    K0, V0, [(q, k, v)] = _inputs(T, bsz, hq, hkv, T)
    outs = {}
    for rows in (True, False):
        attn = _attn(hq, hkv, engine=engine, key_rows=rows)
        kp = attn.dh_prune_key(K0[:, :, :T]).reshape(bsz * hkv, T, 128)
        vp = attn.dh_prune_value(V0[:, :, :T]).reshape(bsz * hkv, T, 128)
        past = attn.to_fused(Past(CompressedArena.from_pruned(kp, "key"), K0[:, :, T:].clone(), CompressedArena.from_pruned(vp, "value"),
                                  V0[:, :, T:].clone(), T, K0.shape[2]))
        assert past[0].key_rows == rows
        outs[rows], _ = attn.decode_fused(q, k, v, past, defer_trigger=True)
        assert _form() == FORM_SB
    assert excess(outs[True], outs[False], NATIVE_ULPS) <= 1.0


# ---- 3. growth ---------------------------------------------------------------------------------------------------------------------
def test_extents_in_tiles_behind_a_base_in_rows(tbw):
    """Two triggers through run_triggers: the base stays rows, the extents are tiles, the outputs equal the tile arena's bit for bit on
    the exact engine's exact scores and within the bound otherwise."""
    bsz, hkv, hq, T = 1, 2, 8, 512
    K0, V0, steps = _inputs(21, bsz, hq, hkv, T, w=250, steps=6 + 256 + 3)
    res = {}
    for rows in (True, False):
        attn = _attn(hq, hkv, engine="dot2", key_rows=rows)
        past = _fused(attn, K0, V0)
        outs = []
        for q, k, v in steps:
            o, past = attn.decode_fused(q, k, v, past, defer_trigger=True)
            if attn.trigger_due(past):
                past = attn.run_triggers([past])[0]
            outs.append(o)
        assert len(past[0].extents) == 2 and past[0].key_rows == rows and not any(e.key_rows for e in past[0].extents)
        assert _form() == FORM_SB
        res[rows] = (outs, past)
    for i, (a, b) in enumerate(zip(res[True][0], res[False][0])):
        assert excess(a, b, NATIVE_ULPS) <= 1.0, f"step {i}"
    a, b = res[True][1][0].to_reference(), res[False][1][0].to_reference()   # (retiles the base back: the whole cache in the reference layout)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(torch.cat(list(a[2])), torch.cat(list(b[2])))


def test_graphs_over_a_base_in_rows_device_t_capture_ahead_and_alternating_replays(tbw):
    bsz, hkv, hq, T = 1, 2, 8, 512
    K0, V0, steps = _inputs(22, bsz, hq, hkv, T, w=253, steps=3)
    attn, tiles = _attn(hq, hkv, engine="dot2"), _attn(hq, hkv, engine="dot2", key_rows=False)
    past, past_t = _fused(attn, K0, V0), _fused(tiles, K0, V0)
    assert past[0].key_rows and not past_t[0].key_rows
    # ONE graph with a device-side T, recorded ahead of the trigger over the current base (EXT instantiation, capacity T + 256)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    t_dev = torch.full((1,), T, dtype=torch.int32, device=DEV)
    gq, gk, gv = (x.clone() for x in steps[0])
    attn.decode_fused(gq, gk, gv, (past[0], past[1].clone(), past[2], past[3].clone(), past[4], past[5]))   # scratch outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g_out, _ = attn.decode_fused(gq, gk, gv, past, step_counter=counter, t_device=t_dev, t_capacity=T + 256)
    assert past[0].key_rows, "a capture leaves the rows alone"
    # 34 replays with two alternating queries on one scratch (the e round trip's invariant), against eager calls over the tile arena
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
    # the trigger fires: the same graph reads the extent (tiles) behind the base (rows)
    past = attn.advance(past, 1)
    past_t2 = past_t
    o_t, past_t2 = tiles.decode_fused(gq, gk, gv, past_t2, defer_trigger=True)
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
    assert len(past[0].extents) == 1 and past[0].key_rows
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
    bsz, hkv, hq, T = 1, 2, 8, 512
    K0, V0, [(q, k, v)] = _inputs(31, bsz, hq, hkv, T)
    attn, tiles = _attn(hq, hkv, engine="dot2"), _attn(hq, hkv, engine="dot2", key_rows=False)
    # to_reference()
    p, pt = _fused(attn, K0, V0), _fused(tiles, K0, V0)
    assert p[0].key_rows
    a, b = p[0].to_reference(), pt[0].to_reference()
    assert not p[0].key_rows and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(torch.cat(list(a[2])), torch.cat(list(b[2])))
    # consolidate() returns a tile arena; the next to_fused() may retile it again
    p = _fused(attn, K0, V0)
    c = p[0].consolidate()
    assert c is p[0] and not c.key_rows
    assert attn.to_fused(p)[0].key_rows
    # decode_multi (the multi-query entry point reads tiles)
    p, pt = _fused(attn, K0, V0), _fused(tiles, K0, V0)
    g = torch.Generator(device="cpu").manual_seed(5)
    q2 = torch.randn(bsz, hq, 2, 128, generator=g).half().to(DEV)
    k2, v2 = torch.randn(bsz, hkv, 2, 128, generator=g).half().to(DEV), torch.randn(bsz, hkv, 2, 128, generator=g).half().to(DEV)
    assert p[0].key_rows
    om, _ = attn.decode_multi(q2, k2, v2, p)
    ot, _ = tiles.decode_multi(q2, k2, v2, pt)
    assert not p[0].key_rows and torch.equal(om, ot)
    # an engine switch to the matrix pipe on a rows arena: retiled back, the tile arena's bits
    p, pt = _fused(attn, K0, V0), _fused(tiles, K0, V0)
    assert p[0].key_rows
    attn.cfg.engine = tiles.cfg.engine = "mfma"
    o1, _ = attn.decode_fused(q, k, v, p)
    o2, _ = tiles.decode_fused(q, k, v, pt)
    assert not p[0].key_rows and torch.equal(o1, o2)


def test_a_shared_segment_call_gets_tiles_and_a_per_sequence_segment_reads_rows(tbw):
    from mustafar_amd import partial
    bsz, hkv, hq, T = 1, 2, 8, 512
    K0, V0, [(q, k, v)] = _inputs(32, bsz, hq, hkv, T)
    attn, tiles = _attn(hq, hkv, engine="dot2"), _attn(hq, hkv, engine="dot2", key_rows=False)
    p, pt = _fused(attn, K0, V0), _fused(tiles, K0, V0)
    assert p[0].key_rows
    # the window-less call over a per-sequence segment runs the same launch: it reads the rows
    o1 = attn.decode_segment(q, p[0], p[2], T)
    o2 = tiles.decode_segment(q, pt[0], pt[2], T)
    assert p[0].key_rows and _form() == FORM_SB
    assert excess(o1[0], o2[0], NATIVE_ULPS) <= 1.0
    torch.testing.assert_close(o1[1], o2[1], rtol=0, atol=2.0 ** -8)
    # the shared-segment entry point reads tiles: the arena is retiled back, once, and gives the tile arena's bits
    q3 = torch.randn(3, hq, 1, 128, generator=torch.Generator(device="cpu").manual_seed(6)).half().to(DEV)
    s1 = partial.SharedSegment(p[0], p[2], T, hkv).decode(attn, q3)
    s2 = partial.SharedSegment(pt[0], pt[2], T, hkv).decode(tiles, q3)
    assert not p[0].key_rows
    for a, b in zip(s1, s2):
        assert torch.equal(a, b)


def test_refusals_under_capture_and_at_the_c_boundary(tbw):
    bsz, hkv, hq, T = 1, 2, 8, 512
    K0, V0, [(q, k, v)] = _inputs(33, bsz, hq, hkv, T)
    attn = _attn(hq, hkv, engine="dot2")
    p = _fused(attn, K0, V0)
    assert p[0].key_rows
    attn.decode_fused(q, k, v, (p[0], p[1].clone(), p[2], p[3].clone(), p[4], p[5]))   # scratch outside the capture
    attn.cfg.engine = "mfma"
    attn.decode_fused(q, k, v, _fused(_attn(hq, hkv, engine="mfma"), K0, V0))            # (the matrix pipe's scratch too)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="require_tiles"):
        with torch.cuda.graph(g):
            attn.decode_fused(q, k, v, p, step_counter=counter)
    assert p[0].key_rows
    # a direct C call of an entry point that does not read rows
    L, lib = _lib().load(), _lib()
    other = _fused(_attn(hq, hkv, engine="dot2", key_rows=False), K0, V0)
    assert L.mustafar_cache_rehouse(None, p[0].view_ptr(), other[0].view_ptr(), p[0].heads, T, 0) == 1
    lse = torch.empty(hq, dtype=torch.float32, device=DEV)
    ws = torch.empty(L.mustafar_shared_segment_workspace_bytes(T, hkv, 4, 1, 128), dtype=torch.uint8, device=DEV)
    out = torch.empty_like(q)
    assert L.mustafar_decode_shared_segment(None, p[0].view_ptr(), p[2].view_ptr(), T, hkv, 4, 1, q.data_ptr(), out.data_ptr(),
                                            lse.data_ptr(), ws.data_ptr(), 128 ** 0.5, 128) == 1
    assert lib.VIEW_KEY_ROWS == p[0].view.flags and ctypes.sizeof(lib.CacheView) == p[0].VIEW_BYTES


# ---- 5. off ------------------------------------------------------------------------------------------------------------------------
def test_key_rows_off_by_config_and_by_environment(tbw, monkeypatch):
    bsz, hkv, hq, T = 1, 2, 8, 512
    K0, V0, [(q, k, v)] = _inputs(41, bsz, hq, hkv, T)
    off = _attn(hq, hkv, engine="dot2", key_rows=False)
    p = _fused(off, K0, V0)
    o_off, _ = off.decode_fused(q, k, v, p)
    assert not p[0].key_rows and _form() == FORM_SB
    monkeypatch.setenv("MUSTAFAR_KEY_ROWS", "0")
    env = _attn(hq, hkv, engine="dot2")
    p = _fused(env, K0, V0)
    o_env, _ = env.decode_fused(q, k, v, p)
    assert not p[0].key_rows and _form() == FORM_SB and torch.equal(o_env, o_off)
    monkeypatch.delenv("MUSTAFAR_KEY_ROWS")
    assert _fused(_attn(hq, hkv, engine="dot2"), K0, V0)[0].key_rows
    # where the launch form does not read rows nothing is retiled either: MHA, the matrix pipe, the default shape rule at this size
    assert not _fused(_attn(8, 8), K0.repeat(1, 4, 1, 1), V0.repeat(1, 4, 1, 1))[0].key_rows
    assert not _fused(_attn(hq, hkv, engine="mfma"), K0, V0)[0].key_rows
    _lib().load().mustafar_tune(1, 1)
    p = _fused(_attn(hq, hkv, engine="dot2"), K0, V0)
    o_two, _ = _attn(hq, hkv, engine="dot2").decode_fused(q, k, v, p)
    assert not p[0].key_rows and _form() == FORM_SB                         # the super-block launch of TWO blocks per workgroup keeps tiles
    _lib().load().mustafar_tune(1, 0)
    assert not _fused(_attn(hq, hkv, engine="dot2"), K0, V0)[0].key_rows   # (and the small form takes a launch of this size by default)
