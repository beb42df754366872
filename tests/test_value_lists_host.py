"""CPU: sorted channel lists of a value base (include/mustafar_hip.h: MUSTAFAR_VIEW_VALUE_LISTS) without a GPU -- the NumPy reference of
both retile directions (tests/value_lists_ref.py, what tests/test_gpu_value_lists.py holds the device kernels to) against the oracle's
compression of small inputs, the symbols, the refusals and the answers of mustafar_decode_reads_value_lists."""
import ctypes
import os
import re

import numpy as np
import pytest

import value_lists_ref as ref
from mustafar_amd import _lib
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_value_cache(x):
    """Oracle compression of pruned rows x [H, T, 128] -> (bmp uint64 [H, 2 T], idx uint32 [H, 2 T + 1], uint16 streams)."""
    H = x.shape[0]
    bmp, idx, nzs = orc.convert_value_batched(np.ascontiguousarray(x))
    return bmp.reshape(H, -1).view(np.uint64), idx.reshape(H, -1).view(np.uint32), [n.view(np.uint16).copy() for n in nzs]


def special_rows(seed=0, H=2, T=320):
    """Pruned rows with every special block.  Head 0: block 0 a channel kept by all 64 tokens next to one kept by none (depth 64, cnt 0);
    block 1 all zero; block 2 all lists equal and of depth 10 = 2 mod 4 (m_r constant, a half word); block 3 a token of 42 equal
    magnitudes (what a tie leaves).  Head 1 and block 4: random."""
    rng = np.random.default_rng(seed)
    x = orc.prune_magnitude(rng.standard_normal((H, T, 128)).astype(np.float16), 0.7)
    x[0, 0:64, 5] = np.float16(0.25)
    x[0, 0:64, 6] = 0
    x[0, 0:64, 70] = np.float16(-0.5)
    x[0, 64:128] = 0
    x[0, 128:192] = 0
    x[0, 128:138] = (rng.integers(1, 9, (10, 128)) / 8).astype(np.float16)
    x[0, 200] = 0
    x[0, 200, :42] = np.float16(1.5)
    return x


def keep_zeros(bmp, idx, nzs):
    """Turn kept values into +0 / -0 in place (the bitmap bit stays set): head 1, block 0, token 0 and token 9, their first entries."""
    for t, bits in ((0, 0x0000), (9, 0x8000)):
        tile = t
        assert int(bmp[1, tile]) != 0
        nzs[1][2 * int(idx[1, tile])] = bits
    return bmp, idx, nzs


def test_the_symbols_are_declared_bound_and_exported_and_the_abi_stays_115():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mustafar_hip.h")).read(), flags=re.S)
    syms = set(re.findall(r"\b(mustafar_\w+)\s*\(", text))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("mustafar_value_lists_plan", "mustafar_value_lists_fill", "mustafar_value_lists_to_tiles", "mustafar_decode_reads_value_lists"):
        assert s in syms and s in _lib.SIGNATURES and hasattr(raw, s), s
    assert _lib.load().mustafar_abi_version() == 115
    assert "MUSTAFAR_VIEW_VALUE_LISTS 2u" in text and _lib.VIEW_VALUE_LISTS == 2
    assert ctypes.sizeof(_lib.CacheView) == 64 and _lib.CacheView.flags.offset == 56


def test_reference_layout_and_round_trip_on_special_blocks():
    x = special_rows()
    H, T = x.shape[0], x.shape[1]
    bmp, idx, nzs = keep_zeros(*reference_value_cache(x))
    table, blocks = ref.tiles_to_lists(bmp, idx, nzs, T)
    assert (table % 4 == 0).all() and (table[:, 0] == 0).all()
    for h in range(H):
        assert blocks[h].size == 4 * int(table[h, -1])

    def header(h, b):
        blk = blocks[h][4 * int(table[h, b]):4 * int(table[h, b + 1])]
        return blk, blk[0:128].reshape(2, 64), blk[128:192].reshape(2, 32), int(blk[192:196].view(np.uint32)[0])

    # depth 64 beside cnt 0: channel 5 leads half 0 and owns all 32 value rows; channel 6 is the last lane and is in no row
    blk, perm, m, half1 = header(0, 0)
    assert perm[0, 0] == 5 and perm[0, 63] == 6 and m[0, 31] == 1 and m[0, 0] < 64 and perm[1, 0] == 70 - 64
    assert sorted(perm[0]) == list(range(64)) and sorted(perm[1]) == list(range(64))
    assert half1 == 64 + ref.half_dwords(m[0]) and blk.size == (4 * (half1 + ref.half_dwords(m[1])) + 15) // 16 * 16
    assert (np.diff(m.astype(int), axis=1) <= 0).all()
    tok = blk[256:256 + 4 * int(m[0, 0])].reshape(-1, 4)
    assert list(tok[0]) == [0, 1, 2, 3]
    # an all-zero block: a header and nothing else
    blk, perm, m, half1 = header(0, 1)
    assert blk.size == 256 and not m.any() and half1 == 64 and list(perm[0]) == list(range(64))
    # all lists equal, depth 10: five value rows of 64 lanes, three token rows, the last word a half word
    blk, perm, m, half1 = header(0, 2)
    assert list(m[0]) == [64] * 5 + [0] * 27 and list(perm[1]) == list(range(64))
    assert ref.half_dwords(m[0]) == 64 * (3 + 5) and half1 == 64 + 512 and blk.size == 256 + 2 * 2048
    # a kept +0 at token 0 and a kept -0 at a later token are entries
    vals, kept = ref.expand_block(bmp[1], idx[1], nzs[1], 0)
    assert kept[0].sum() == (x[1, 0] != 0).sum() and (vals[0][kept[0]] == 0).sum() == 1 and (vals[9][kept[9]] == 0x8000).sum() == 1
    b2, i2, n2 = ref.lists_to_tiles(table, blocks, T)
    assert np.array_equal(b2, bmp) and np.array_equal(i2, idx)
    assert all(np.array_equal(a, b) for a, b in zip(n2, nzs))


@pytest.mark.parametrize("sparsity", [0.5, 0.7, 0.9])
def test_round_trip_and_size_across_sparsities(sparsity):
    rng = np.random.default_rng(int(sparsity * 10))
    x = orc.prune_magnitude(rng.standard_normal((1, 128, 128)).astype(np.float16), sparsity)
    bmp, idx, nzs = reference_value_cache(x)
    table, blocks = ref.tiles_to_lists(bmp, idx, nzs, 128)
    # the size formula: per half, sum over the channels of 2 bytes x cnt rounded up to even + 1 byte x cnt rounded up to a multiple of 4
    for b in range(2):
        vals, kept = ref.expand_block(bmp[0], idx[0], nzs[0], b)
        want = 256
        for half in range(2):
            cnt = kept[:, 64 * half:64 * half + 64].sum(0)
            want += int((2 * ((cnt + 1) // 2 * 2) + (cnt + 3) // 4 * 4).sum())
        assert 4 * int(table[0, b + 1] - table[0, b]) == (want + 15) // 16 * 16
    b2, i2, n2 = ref.lists_to_tiles(table, blocks, 128)
    assert np.array_equal(b2, bmp) and np.array_equal(i2, idx) and np.array_equal(n2[0], nzs[0])


def test_a_table_of_65_blocks_continues_behind_entry_63():
    """The 4160-token input of tests/test_gpu_value_lists.py (special_4160: two heads, 65 blocks -- one more than a 64-lane trip of the
    device's table scan; 66 table entries per head): entries 64 and 65 of each head's table continue entry 63 by the sizes of blocks 63
    and 64, read from the blocks' own headers, and the round trip is bit exact."""
    T = 4160
    bmp, idx, nzs = keep_zeros(*reference_value_cache(special_rows(seed=T, T=T)))
    table, blocks = ref.tiles_to_lists(bmp, idx, nzs, T)
    assert table.shape == (2, 66)

    def dwords(h, b):   # header, half 0 (up to the offset of half 1), half 1, padded to 16 bytes
        blk = blocks[h][4 * int(table[h, b]):]
        half1, m1 = int(blk[192:196].view(np.uint32)[0]), blk[128 + 32:192]
        return (half1 + ref.half_dwords(m1) + 3) // 4 * 4

    for h in range(2):
        assert int(table[h, 64]) == int(table[h, 63]) + dwords(h, 63) and int(table[h, 65]) == int(table[h, 64]) + dwords(h, 64)
        assert blocks[h].size == 4 * int(table[h, 65]) and int(table[h, 64]) > 64 * 64
    assert table[0, 64] != table[1, 64]   # (the heads' tables differ: a wrong pitch between them would show)
    b2, i2, n2 = ref.lists_to_tiles(table, blocks, T)
    assert np.array_equal(b2, bmp) and np.array_equal(i2, idx)
    assert all(np.array_equal(a, b) for a, b in zip(n2, nzs))


def test_reads_value_lists_equals_reads_key_rows_over_a_grid_of_shapes():
    L = _lib.load()
    flags = [0, _lib.ENGINE_FLAGS["valu"], _lib.ENGINE_FLAGS["dot2"], _lib.ENGINE_FLAGS["mfma"], _lib.STRUCTURE_FLAGS["two_launch"],
             _lib.STRUCTURE_FLAGS["one_pass"], 1 << 6]
    seen = set()
    for groups in (1, 2, 4, 8):
        for T in (0, 256, 1024 + 32, 4096, 7936, 16128, 32512, 64 * 5000):
            for gy in (0, 1, 8, 64, 128):
                for pad in (0, 8):
                    ld = (T + 32 + 256 + 31) // 32 * 32 + pad
                    for f in flags:
                        a, b = L.mustafar_decode_reads_value_lists(groups, T, gy, ld, f), L.mustafar_decode_reads_key_rows(groups, T, gy, ld, f)
                        assert a == b, (groups, T, gy, ld, f)
                        seen.add(a)
    assert seen == {0, 1}
    assert L.mustafar_decode_reads_value_lists(4, 7936, 64, 8224, 0) == 1      # c3
    assert L.mustafar_decode_reads_value_lists(4, 7936, 8, 8224, 0) == 0       # 8k x batch 1: two blocks per workgroup


def test_entry_points_refuse_a_value_list_view_without_a_gpu():
    """Every native entry point but the one-pass super-block launch answers MUSTAFAR_EINVAL for a view flagged value lists, before any
    launch (so it can be asked here)."""
    L = _lib.load()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    lists = _lib.CacheView(None, p, p, None, 0, 5, 40, _lib.VIEW_VALUE_LISTS)
    rows = _lib.CacheView(None, p, p, None, 0, 4, 16 * 40, _lib.VIEW_KEY_ROWS)
    tiles = _lib.CacheView(p, p, p, p, 0, 0, 64, 0)
    v, r, t = ctypes.byref(lists), ctypes.byref(rows), ctypes.byref(tiles)
    assert L.mustafar_cache_rehouse(None, v, t, 1, 256, 0) == 1 and L.mustafar_cache_rehouse(None, t, v, 1, 256, 0) == 1
    assert L.mustafar_cache_append_bitmap_value(None, p, 1, 64, 128, v, 256, p) == 1
    assert L.mustafar_cache_append_pack_value(None, p, 1, 64, 128, v, 256) == 1
    assert L.mustafar_cache_consolidate_extents(None, v, p, 1, 1, 256, 0) == 1
    assert L.mustafar_decode_shared_segment(None, t, v, 256, 1, 4, 1, p, p, p, p, 11.3, 128) == 1
    assert L.mustafar_value_lists_plan(None, v, 1, 256, p, p) == 1              # the source of a retile to lists is tiles ...
    assert L.mustafar_value_lists_fill(None, v, v, 1, 256) == 1
    assert L.mustafar_value_lists_to_tiles(None, t, t, 1, 256, p) == 1          # ... and the source of a retile back is lists
    assert L.mustafar_value_lists_fill(None, t, t, 1, 256) == 1
    assert L.mustafar_value_lists_fill(None, t, r, 1, 256) == 1                 # (key rows are not value lists, either way)
    assert L.mustafar_key_rows_to_tiles(None, v, t, 1, 256, p) == 1
    assert L.mustafar_value_lists_fill(None, t, ctypes.byref(_lib.CacheView(None, p, p, None, 0, 4, 40, 2)), 1, 256) == 1   # a table without its last entry
    assert L.mustafar_value_lists_plan(None, t, 1, 256 + 32, p, p) == 1         # tokens % 64
    # a fused call: the key side has no such form, and neither two launches nor the matrix pipe read lists
    tail = (p, p, p, None, None, 1, 64, p, 256 + 64, p, p, 1, 256, 4, 4, 11.3, None, None, 0, 1)
    klists = _lib.CacheView(p, p, p, p, 0, 0, 64, _lib.VIEW_VALUE_LISTS)
    assert L.mustafar_decode_attention_view(None, ctypes.byref(klists), t, *tail, 0) == 1
    assert L.mustafar_decode_attention_view(None, t, ctypes.byref(_lib.CacheView(p, p, p, p, 0, 0, 64, 3)), *tail, 0) == 1
    assert L.mustafar_decode_attention_view(None, t, v, *tail, _lib.STRUCTURE_FLAGS["two_launch"]) == 1
    assert L.mustafar_decode_attention_view(None, t, v, *tail, _lib.ENGINE_FLAGS["mfma"]) == 1
    assert L.mustafar_decode_attention_view(None, r, v, *tail, _lib.ENGINE_FLAGS["mfma"]) == 1
