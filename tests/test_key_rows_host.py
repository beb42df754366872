"""CPU: token-row key blocks (ABI 113; include/mustafar_hip.h: MUSTAFAR_VIEW_KEY_ROWS) without a GPU -- the NumPy reference of both
retile directions (tests/key_rows_ref.py, what tests/test_gpu_key_rows.py holds the device kernels to) against the oracle's compression
of small inputs, and the answers of mustafar_decode_reads_key_rows for the benchmark's shapes."""
import ctypes
import os
import re

import numpy as np
import pytest

import key_rows_ref as ref
from mustafar_amd import _lib
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_key_cache(x):
    """Oracle compression of pruned rows x [H, T, 128] -> (bmp uint64 [H, 2 T], idx uint32 [H, 2 T + 1], uint16 streams)."""
    H = x.shape[0]
    bmp, idx, nzs = orc.convert_key_batched(np.ascontiguousarray(x))
    return bmp.reshape(H, -1).view(np.uint64), idx.reshape(H, -1).view(np.uint32), [n.view(np.uint16) for n in nzs]


def special_rows(seed=0, H=2, T=192):
    """Pruned rows with every special block: a tie row (w = 42), rows that keep 1 and 128 channels (w = 128 beside a 1), an all-zero
    token, an all-zero block."""
    rng = np.random.default_rng(seed)
    x = orc.prune_magnitude(rng.standard_normal((H, T, 128)).astype(np.float16), 0.7)
    x[0, 3] = 0                                   # an all-zero token
    x[0, 10] = 0
    x[0, 10, :42:1] = np.float16(1.5)             # a token with 42 kept channels: what a magnitude tie leaves (block 0 of head 0: w = 42)
    x[1, 70, 1:] = 0                              # a token that keeps one channel ...
    x[1, 71] = (rng.standard_normal(128).astype(np.float16) + np.float16(3)).astype(np.float16)
    x[1, 71][x[1, 71] == 0] = np.float16(1)       # ... beside one that keeps all 128 (block 1 of head 1: w = 128)
    x[1, 128:192] = 0                             # an all-zero block (w = 2)
    return x


def test_abi_113_declares_binds_and_exports_the_new_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mustafar_hip.h")).read(), flags=re.S)
    syms = set(re.findall(r"\b(mustafar_\w+)\s*\(", text))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("mustafar_key_rows_plan", "mustafar_key_rows_fill", "mustafar_key_rows_to_tiles", "mustafar_decode_reads_key_rows"):
        assert s in syms and s in _lib.SIGNATURES and hasattr(raw, s), s
    assert _lib.load().mustafar_abi_version() >= 113
    assert "MUSTAFAR_VIEW_KEY_ROWS 1u" in text and _lib.VIEW_KEY_ROWS == 1
    assert ctypes.sizeof(_lib.CacheView) == 64 and _lib.CacheView.flags.offset == 56   # seven 8-byte words, then the flags


def test_reference_layout_and_round_trip_on_oracle_compression():
    x = special_rows()
    T = x.shape[1]
    bmp, idx, nzs = reference_key_cache(x)
    table, rows = ref.tiles_to_rows(bmp, idx, nzs, T)
    w = table & 0xFF
    assert w[0, 0] == 42 and w[1, 1] == 128 and w[1, 2] == 2 and (w % 2 == 0).all() and (w >= 2).all()
    for h in range(x.shape[0]):   # blocks lie back to back, in rows of 256 bytes
        first = 0
        for b in range(T // 64):
            assert table[h, b] >> 8 == first
            first += ref.rows_of(int(w[h, b]))
        assert rows[h].size == 256 * first
    # a token's slots: its non-zero channels in ascending order, then value +0 / channel 0
    for h, b, t in ((0, 0, 10), (0, 0, 3), (1, 1, 6), (1, 1, 7), (0, 2, 5)):
        wb, first = int(w[h, b]), int(table[h, b] >> 8)
        blk = rows[h][256 * first:256 * (first + ref.rows_of(wb))]
        c = blk[:256 * ((wb + 3) // 4)].reshape(-1, 64, 4)[:, t].reshape(-1)
        v = blk[256 * ((wb + 3) // 4):].view(np.uint16).reshape(-1, 64, 2)[:, t].reshape(-1)
        row = x[h, 64 * b + t].view(np.uint16)
        keep = np.flatnonzero(row & 0x7FFF)
        assert np.array_equal(c[:keep.size], keep) and np.array_equal(v[:keep.size], row[keep])
        assert not c[keep.size:].any() and not v[keep.size:].any()
    b2, i2, n2 = ref.rows_to_tiles(table, rows, T)
    assert np.array_equal(b2, bmp) and np.array_equal(i2, idx)
    assert all(np.array_equal(a, b) for a, b in zip(n2, nzs))


@pytest.mark.parametrize("sparsity", [0.5, 0.7, 0.9])
def test_round_trip_across_sparsities(sparsity):
    rng = np.random.default_rng(int(sparsity * 10))
    x = orc.prune_magnitude(rng.standard_normal((1, 128, 128)).astype(np.float16), sparsity)
    bmp, idx, nzs = reference_key_cache(x)
    table, rows = ref.tiles_to_rows(bmp, idx, nzs, 128)
    kept = 128 - max(1, int(sparsity * 128)) + 1
    assert ((table & 0xFF) >= kept).all() and ((table & 0xFF) <= kept + 4).all()   # the kept count, a tie or two more
    b2, i2, n2 = ref.rows_to_tiles(table, rows, 128)
    assert np.array_equal(b2, bmp) and np.array_equal(i2, idx) and np.array_equal(n2[0], nzs[0])


def test_a_table_of_65_blocks_continues_behind_entry_63():
    """The 4160-token input of tests/test_gpu_key_rows.py (special_4160: two heads, 65 blocks -- one more than a 64-lane trip of the
    device's table scan): entry 64 of each head's table is entry 63's first row + its rows, and the round trip is bit exact."""
    from tests.test_gpu_key_rows import _special
    T = 4160
    bmp, idx, nzs = reference_key_cache(_special(T))
    table, rows = ref.tiles_to_rows(bmp, idx, nzs, T)
    assert table.shape == (2, 65)
    for h in range(2):
        first, w = table[h].astype(np.int64) >> 8, table[h].astype(np.int64) & 0xFF
        assert first[64] == first[63] + ref.rows_of(int(w[63])) and first[64] > 64 * ref.rows_of(2)
        assert rows[h].size == 256 * (first[64] + ref.rows_of(int(w[64])))
    assert table[0, 64] != table[1, 64]   # (the heads' tables differ: a wrong pitch between them would show)
    b2, i2, n2 = ref.rows_to_tiles(table, rows, T)
    assert np.array_equal(b2, bmp) and np.array_equal(i2, idx)
    assert all(np.array_equal(a, b) for a, b in zip(n2, nzs))


# (name, q heads, kv heads, L, batch) of bench.py's configurations; R = 32 rows stay in the window
_SHAPES = {"c1": (32, 32, 1024, 1), "c2": (32, 32, 4096, 1), "c3": (32, 8, 8192, 8), "c4": (32, 8, 32768, 4), "c5": (32, 8, 16384, 16),
           "b1": (32, 8, 8192, 1), "4k_b1": (32, 8, 4096, 1), "mha": (32, 32, 8192, 8), "gqa2": (32, 16, 8192, 8)}
# super-block form at four blocks per workgroup (from 768 workgroups on): c3, c4, c5 yes; 8k x batch 1 is 248 workgroups of two blocks
# (measured slower on rows: excluded); 4k x batch 1 runs the small form; MHA and GQA-2 run v_fma_mix pairs (G < 4)
_WANT = {"c1": 0, "c2": 0, "c3": 1, "c4": 1, "c5": 1, "b1": 0, "4k_b1": 0, "mha": 0, "gqa2": 0}


def _reads(name, flags=0):
    Hq, Hkv, Lq, batch = _SHAPES[name]
    groups = Hq // Hkv
    T = ((Lq - 32) // 256) * 256
    G = 4 if groups % 4 == 0 else 2 if groups % 2 == 0 else 1
    ld = (T + 32 + 256 + 31) // 32 * 32
    return _lib.load().mustafar_decode_reads_key_rows(groups, T, batch * Hkv * (groups // G), ld, flags)


@pytest.mark.parametrize("name", sorted(_SHAPES))
def test_reads_key_rows_for_the_benchmark_shapes(name):
    assert _reads(name) == _WANT[name]
    assert _reads(name, _lib.ENGINE_FLAGS["valu"]) == _WANT[name] and _reads(name, _lib.ENGINE_FLAGS["dot2"]) == _WANT[name]
    assert _reads(name, _lib.ENGINE_FLAGS["mfma"]) == 0                  # the matrix pipe keeps tiles
    assert _reads(name, _lib.STRUCTURE_FLAGS["two_launch"]) == 0         # and so do two launches
    assert _reads(name, 1 << 6) == 0                                     # undefined flag bits


def test_reads_key_rows_rejects_what_the_launch_rejects():
    L = _lib.load()
    assert L.mustafar_decode_reads_key_rows(4, 7936, 64, 8224, 0) == 1
    assert L.mustafar_decode_reads_key_rows(4, 7936, 64, 8224 + 8, 0) == 0    # row pitch % 32: two launches
    assert L.mustafar_decode_reads_key_rows(4, 7936 + 32, 64, 8256, 0) == 0   # T % 64
    assert L.mustafar_decode_reads_key_rows(4, 0, 64, 320, 0) == 0
    assert L.mustafar_decode_reads_key_rows(4, 64 * 5000, 64, 64 * 5000 + 320, 0) == 0   # rows so long that a workgroup takes more than four blocks


def test_entry_points_refuse_a_token_row_view_without_a_gpu():
    """Every native entry point but the one-pass super-block launch answers MUSTAFAR_EINVAL for a view flagged token rows, before any
    launch (so it can be asked here)."""
    L = _lib.load()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    rows = _lib.CacheView(None, p, p, None, 0, 4, 16 * 40, _lib.VIEW_KEY_ROWS)
    tiles = _lib.CacheView(p, p, p, p, 0, 0, 64, 0)
    r, t = ctypes.byref(rows), ctypes.byref(tiles)
    assert L.mustafar_cache_rehouse(None, r, t, 1, 256, 0) == 1 and L.mustafar_cache_rehouse(None, t, r, 1, 256, 0) == 1
    assert L.mustafar_cache_append_bitmap_key(None, p, 1, 64, 128, r, 256, p) == 1
    assert L.mustafar_cache_append_pack_key(None, p, 1, 64, 128, r, 256) == 1
    assert L.mustafar_cache_consolidate_extents(None, r, p, 1, 1, 256, 0) == 1
    assert L.mustafar_decode_shared_segment(None, r, t, 256, 1, 4, 1, p, p, p, p, 11.3, 128) == 1
    assert L.mustafar_key_rows_plan(None, r, 1, 256, p, p) == 1              # the source of a retile to rows is tiles ...
    assert L.mustafar_key_rows_fill(None, r, r, 1, 256) == 1
    assert L.mustafar_key_rows_to_tiles(None, t, t, 1, 256, p) == 1          # ... and the source of a retile back is rows
    assert L.mustafar_key_rows_fill(None, t, t, 1, 256) == 1
    # a fused call: the value side has no such form, an unknown flag is refused, and two launches do not read rows
    tail = (p, p, p, None, None, 1, 64, p, 256 + 64, p, p, 1, 256, 4, 4, 11.3, None, None, 0, 1)
    vrows = _lib.CacheView(p, p, p, p, 0, 0, 64, _lib.VIEW_KEY_ROWS)
    assert L.mustafar_decode_attention_view(None, t, ctypes.byref(vrows), *tail, 0) == 1
    assert L.mustafar_decode_attention_view(None, ctypes.byref(_lib.CacheView(p, p, p, p, 0, 0, 64, 2)), t, *tail, 0) == 1
    assert L.mustafar_decode_attention_view(None, r, t, *tail, _lib.STRUCTURE_FLAGS["two_launch"]) == 1
    assert L.mustafar_decode_attention_view(None, r, t, *tail, _lib.ENGINE_FLAGS["mfma"]) == 1
