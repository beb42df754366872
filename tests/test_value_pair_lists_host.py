"""CPU: sorted channel lists over pairs of blocks (include/mustafar_hip.h: MUSTAFAR_VIEW_VALUE_PAIR_LISTS) without a GPU --
the NumPy reference of both retile directions (tests/value_pair_lists_ref.py, what tests/test_gpu_value_pair_lists.py holds the device
kernels to) on the special pairs, the header's arithmetic (csrc/value_pair_lists.h, walked by tools/value_pair_lists_check.cpp) against
that reference, the symbols, every refusal of the view rule and the answers of mustafar_decode_reads_value_pair_lists."""
import ctypes
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import value_pair_lists_ref as ref
from mustafar_amd import _lib
from oracle import oracle as orc
from tests.test_value_lists_host import keep_zeros, reference_value_cache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.addressof((ctypes.c_uint64 * 64)())


def special_pair_rows(seed=0, H=2, T=448):
    """Pruned rows with every special pair (T >= 448).  Head 0: pair 0 a channel kept by all 128 tokens next to one kept by none (depth
    128: 64 value rows, 32 words; cnt 0); pair 1 all zero; pair 2 all lists equal and of depth 10 = 2 mod 4, five tokens in each block
    (m_r constant, a half word).  Head 1 and the rest: random.  T = 448 is seven blocks: pair 3 is a trailing half pair."""
    rng = np.random.default_rng(seed)
    x = orc.prune_magnitude(rng.standard_normal((H, T, 128)).astype(np.float16), 0.7)
    x[0, 0:128, 5] = np.float16(0.25)
    x[0, 0:128, 6] = 0
    x[0, 0:128, 70] = np.float16(-0.5)
    x[0, 128:256] = 0
    x[0, 256:384] = 0
    x[0, 256:261] = (rng.integers(1, 9, (5, 128)) / 8).astype(np.float16)
    x[0, 320:325] = (rng.integers(1, 9, (5, 128)) / 8).astype(np.float16)
    return x


def cache_of(vals, kept):
    """(values uint16 [T, 128], kept bool [T, 128]) of one head -> its reference-layout value cache (bmp, idx, [stream])."""
    T = vals.shape[0]
    bmp = np.zeros((1, 2 * T), dtype=np.uint64)
    idx = np.zeros((1, 2 * T + 1), dtype=np.uint32)
    stream = []
    for b in range(T // 64):
        for half in range(2):
            for t in range(64):
                tile = b * 128 + 64 * half + t
                chans = np.flatnonzero(kept[64 * b + t, 64 * half:64 * half + 64])
                bmp[0, tile] = sum(1 << (63 - int(c)) for c in chans)
                n8 = (len(chans) + 7) // 8 * 8
                idx[0, tile + 1] = idx[0, tile] + n8 // 2
                stream.append(np.concatenate([vals[64 * b + t, 64 * half + chans], np.zeros(n8 - len(chans), dtype=np.uint16)]))
    return bmp, idx, [np.concatenate(stream)]


def pattern(ntok):
    """The pattern of tools/value_pair_lists_check.cpp."""
    t, c = np.meshgrid(np.arange(ntok), np.arange(128), indexing="ij")
    kept = (t * 7 + c * 13 + (t * c) % 11) % 10 < 3
    vals = np.where(kept, 0x3c00 + ((t * 131 + c * 17) & 511), 0).astype(np.uint16)
    return vals, kept


def check_cases():
    """name -> (values, kept) of the pairs tools/value_pair_lists_check.cpp walks."""
    cases = {}
    b = pattern(128)
    cases["pattern"] = b
    v, k = b[0].copy(), b[1].copy()
    k[:, 5], v[:, 5], k[:, 6], v[:, 6], k[:, 70], v[:, 70] = True, 0x3400, False, 0, True, 0xb800
    cases["depth_128_beside_cnt_0"] = (v, k)
    cases["all_zero"] = (np.zeros((128, 128), np.uint16), np.zeros((128, 128), bool))
    v, k = np.zeros((128, 128), np.uint16), np.zeros((128, 128), bool)
    for t in (0, 1, 2, 3, 4, 64, 65, 66, 67, 68):
        k[t], v[t] = True, 0x3000 + np.arange(128)
    cases["equal_lists_depth_10"] = (v, k)
    cases["trailing_half_pair"] = pattern(64)
    cases["dense"] = (np.repeat((0x3000 + np.arange(128, dtype=np.uint16))[:, None], 128, 1), np.ones((128, 128), bool))
    v, k = b[0].copy(), b[1].copy()
    for t, c, bits in ((0, 3, 0x0000), (9, 3, 0x8000), (64, 100, 0x8000)):
        k[t, c], v[t, c] = True, bits
    cases["kept_zeros"] = (v, k)
    v, k = np.zeros((128, 128), np.uint16), np.zeros((128, 128), bool)
    k[np.arange(128), np.arange(128)], v[np.arange(128), np.arange(128)] = True, 0x4000
    cases["depth_1"] = (v, k)
    return cases


def test_the_symbols_are_declared_bound_and_exported_and_the_abi_stays_115():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mustafar_hip.h")).read(), flags=re.S)
    syms = set(re.findall(r"\b(mustafar_\w+)\s*\(", text))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("mustafar_value_pair_lists_plan", "mustafar_value_pair_lists_fill", "mustafar_value_pair_lists_to_tiles",
              "mustafar_decode_reads_value_pair_lists"):
        assert s in syms and s in _lib.SIGNATURES and hasattr(raw, s), s
    assert _lib.load().mustafar_abi_version() == 115
    assert "MUSTAFAR_VIEW_VALUE_PAIR_LISTS 4u" in text and _lib.VIEW_VALUE_PAIR_LISTS == 4
    from mustafar_amd.cache import BASE_FORMS, VALUE_PAIR_LISTS
    assert VALUE_PAIR_LISTS in BASE_FORMS and VALUE_PAIR_LISTS.flag == 4 and VALUE_PAIR_LISTS.which == "value"
    assert [VALUE_PAIR_LISTS.table_columns(nb) for nb in (1, 2, 3, 4, 65)] == [3, 3, 5, 5, 67]


def test_reference_layout_and_round_trip_on_special_pairs():
    x = special_pair_rows()
    H, T = x.shape[0], x.shape[1]
    bmp, idx, nzs = keep_zeros(*reference_value_cache(x))
    table, blocks = ref.tiles_to_pair_lists(bmp, idx, nzs, T)
    assert table.shape == (H, 2 * 4 + 1) and (table[:, 0::2] % 4 == 0).all() and (table[:, 0] == 0).all()
    for h in range(H):
        assert blocks[h].size == 4 * int(table[h, -1])

    def header(h, p):
        hdr = blocks[h][4 * int(table[h, 2 * p]):4 * int(table[h, 2 * p]) + 256]
        return hdr[0:128].reshape(2, 64), hdr[128:256].reshape(2, 64), int(table[h, 2 * p + 1] - table[h, 2 * p]), int(table[h, 2 * p + 2] - table[h, 2 * p])

    # depth 128 beside cnt 0: channel 5 leads half 0 and owns all 64 value rows; channel 6 is the last lane and is in no row
    perm, m, half1, size = header(0, 0)
    assert perm[0, 0] == 5 and perm[0, 63] == 6 and m[0, 63] == 1 and m[0, 0] < 64 and perm[1, 0] == 70 - 64 and m[1, 63] == 1
    assert sorted(perm[0]) == list(range(64)) and sorted(perm[1]) == list(range(64))
    assert half1 == 64 + ref.half_dwords(m[0]) and size == (half1 + ref.half_dwords(m[1]) + 3) // 4 * 4
    assert (np.diff(m.astype(int), axis=1) <= 0).all()
    at = 4 * (int(table[0, 0]) + 64)
    assert list(blocks[0][at:at + 4]) == [0, 1, 2, 3]
    # an all-zero pair: a header and nothing else
    perm, m, half1, size = header(0, 1)
    assert size == 64 and half1 == 64 and not m.any() and list(perm[0]) == list(range(64))
    # all lists equal, depth 10 over both blocks: five value rows of 64 lanes, three token rows, the last word a half word
    perm, m, half1, size = header(0, 2)
    assert list(m[0]) == [64] * 5 + [0] * 59 and list(perm[1]) == list(range(64))
    assert half1 == 64 + 64 * (3 + 5) and size == 64 + 2 * 512
    at = 4 * (int(table[0, 4]) + 64)
    assert list(blocks[0][at:at + 4]) == [0, 1, 2, 3] and list(blocks[0][at + 768:at + 772]) == [4, 64, 65, 66]
    # a trailing half pair: tokens below 64 only
    vals, kept = ref.expand_pair(bmp[1], idx[1], nzs[1], 3, T // 64)
    assert vals.shape == (64, 128)
    perm, m, half1, size = header(1, 3)
    assert int(m[0, 0]) == int((kept[:, :64].sum(0) > 0).sum()) and not m[:, 32:].any()
    # a kept +0 at token 0 and a kept -0 at a later token are entries
    vals, kept = ref.expand_pair(bmp[1], idx[1], nzs[1], 0, T // 64)
    assert kept[0].sum() == (x[1, 0] != 0).sum() and (vals[0][kept[0]] == 0).sum() == 1 and (vals[9][kept[9]] == 0x8000).sum() == 1
    b2, i2, n2 = ref.pair_lists_to_tiles(table, blocks, T)
    assert np.array_equal(b2, bmp) and np.array_equal(i2, idx)
    assert all(np.array_equal(a, b) for a, b in zip(n2, nzs))


def test_the_words_of_a_pair_are_fewer_than_those_of_its_two_blocks():
    """What the form is for: a wave walks ceil(longest list / 4) words per half -- over a pair against twice the larger of two blocks."""
    import value_lists_ref as blocks_ref
    rng = np.random.default_rng(1)
    x = orc.prune_magnitude(rng.standard_normal((1, 1024, 128)).astype(np.float16), 0.7)
    bmp, idx, nzs = reference_value_cache(x)
    pair_words = block_words = 0
    for p in range(8):
        _, kept = ref.expand_pair(bmp[0], idx[0], nzs[0], p, 16)
        for half in range(2):
            k = kept[:, 64 * half:64 * half + 64]
            pair_words += ref.half_words(k.sum(0))
            block_words += 2 * max(ref.half_words(k[:64].sum(0)), ref.half_words(k[64:].sum(0)))
    assert pair_words < 0.95 * block_words, (pair_words, block_words)
    table, blocks = ref.tiles_to_pair_lists(bmp, idx, nzs, 1024)
    t64, b64 = blocks_ref.tiles_to_lists(bmp, idx, nzs, 1024)
    assert blocks[0].size <= b64[0].size, "one header per pair: the container does not grow"


@pytest.mark.skipif(shutil.which("c++") is None, reason="needs a host C++ compiler")
def test_the_headers_arithmetic_gives_the_references_bytes_on_the_special_pairs(tmp_path):
    exe = str(tmp_path / "value_pair_lists_check")
    subprocess.check_call(["c++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tools", "value_pair_lists_check.cpp")])   # (a program of its own: the sanitizers' runtimes are linked in)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    got = {}
    for line in out.stdout.splitlines():
        f = line.split()
        assert f[-3:] == ["round", "trip", "ok"], line
        got[f[0]] = (int(f[1]), int(f[4]), int(f[6], 16))
    cases = check_cases()
    assert sorted(got) == sorted(cases)
    for name, (vals, kept) in cases.items():
        T = vals.shape[0]
        bmp, idx, nzs = cache_of(vals, kept)
        table, blocks = ref.tiles_to_pair_lists(bmp, idx, nzs, T)
        assert table.shape == (1, 3)
        assert got[name] == (blocks[0].size, int(table[0, 1]), zlib.crc32(blocks[0].tobytes())), name
        b2, i2, n2 = ref.pair_lists_to_tiles(table, blocks, T)
        assert np.array_equal(b2, bmp) and np.array_equal(i2, idx) and np.array_equal(n2[0], nzs[0]), name


def test_a_table_of_65_blocks_has_33_pairs_and_ends_in_a_half_pair():
    T = 4160
    bmp, idx, nzs = keep_zeros(*reference_value_cache(special_pair_rows(seed=T, T=T)))
    table, blocks = ref.tiles_to_pair_lists(bmp, idx, nzs, T)
    assert table.shape == (2, 67) and (np.diff(table.astype(np.int64), axis=1) >= 0).all()
    for h in range(2):
        assert blocks[h].size == 4 * int(table[h, 66]) and int(table[h, 64]) > 64 * 64
    assert table[0, 64] != table[1, 64]   # (the heads' tables differ: a wrong pitch between them would show)
    b2, i2, n2 = ref.pair_lists_to_tiles(table, blocks, T)
    assert np.array_equal(b2, bmp) and np.array_equal(i2, idx)
    assert all(np.array_equal(a, b) for a, b in zip(n2, nzs))


def test_reads_value_pair_lists_equals_reads_key_rows_over_a_grid_of_shapes():
    L = _lib.load()
    flags = [0, _lib.ENGINE_FLAGS["valu"], _lib.ENGINE_FLAGS["dot2"], _lib.ENGINE_FLAGS["mfma"], _lib.STRUCTURE_FLAGS["two_launch"],
             _lib.STRUCTURE_FLAGS["one_pass"], 1 << 6]
    seen = set()
    for groups in (1, 2, 4, 8):
        for T in (0, 64, 192, 256, 1024 + 32, 4096, 4160, 7936, 16128, 32512, 64 * 5000):
            for gy in (0, 1, 8, 64, 128):
                for pad in (0, 8):
                    ld = (T + 32 + 256 + 31) // 32 * 32 + pad
                    for f in flags:
                        a, b = L.mustafar_decode_reads_value_pair_lists(groups, T, gy, ld, f), L.mustafar_decode_reads_key_rows(groups, T, gy, ld, f)
                        assert a == b, (groups, T, gy, ld, f)
                        seen.add(a)
    assert seen == {0, 1}
    assert L.mustafar_decode_reads_value_pair_lists(4, 7936, 64, 8224, 0) == 1      # c3
    assert L.mustafar_decode_reads_value_pair_lists(4, 7936, 8, 8224, 0) == 0       # 8k x batch 1: two blocks per workgroup


def _pairs_view(tokens, **wrong):
    fields = dict(bmp=None, nz=P, idx=P, nz_offset=None, bmp_head_stride=0, idx_head_stride=2 * ((tokens // 64 + 1) // 2) + 1, nz_head_stride=40,
                  flags=_lib.VIEW_VALUE_PAIR_LISTS)
    fields.update(wrong)
    return _lib.CacheView(*fields.values())


_MALFORMED = {"flag of the lists per block": dict(flags=_lib.VIEW_VALUE_LISTS), "flag of key rows": dict(flags=_lib.VIEW_KEY_ROWS),
              "both list flags": dict(flags=6), "null idx": dict(idx=None), "null nz": dict(nz=None), "nz_head_stride 0": dict(nz_head_stride=0),
              "table pitch one short": None}


@pytest.mark.parametrize("what", sorted(_MALFORMED))
@pytest.mark.parametrize("tokens", [256, 320])   # (320: five blocks, three pairs, seven table entries)
def test_every_refusal_of_the_view_rule(what, tokens):
    L = _lib.load()
    wrong = _MALFORMED[what] or dict(idx_head_stride=2 * ((tokens // 64 + 1) // 2))
    bad, good = ctypes.byref(_pairs_view(tokens, **wrong)), ctypes.byref(_pairs_view(tokens))
    tiles = ctypes.byref(_lib.CacheView(P, P, P, P, 0, 0, 64, 0))
    assert L.mustafar_value_pair_lists_to_tiles(None, bad, tiles, 1, tokens, P) == 1
    assert L.mustafar_value_pair_lists_fill(None, tiles, bad, 1, tokens) == 1
    # a tile view is the source of the way there and the target of the way back; shapes
    assert L.mustafar_value_pair_lists_plan(None, good, 1, tokens, P, P) == 1 and L.mustafar_value_pair_lists_fill(None, good, good, 1, tokens) == 1
    assert L.mustafar_value_pair_lists_to_tiles(None, good, good, 1, tokens, P) == 1
    assert L.mustafar_value_pair_lists_plan(None, tiles, 1, tokens + 32, P, P) == 1 and L.mustafar_value_pair_lists_plan(None, tiles, 0, tokens, P, P) == 1
    assert L.mustafar_value_pair_lists_plan(None, tiles, 1, tokens, None, P) == 1 and L.mustafar_value_pair_lists_plan(None, tiles, 1, tokens, P, None) == 1
    # a table with a column too many is no table of this pass
    assert L.mustafar_value_pair_lists_fill(None, tiles, ctypes.byref(_pairs_view(tokens, idx_head_stride=2 * ((tokens // 64 + 1) // 2) + 2)), 1, tokens) == 1
    # the fused call at c3's shape, where the launch reads the form and the view rule is all that stands in front of it
    T, batch, cap, ld = 7936, 256, 288, 8224
    assert L.mustafar_decode_reads_value_pair_lists(4, T, 64, ld, 0) == 1
    wrong = _MALFORMED[what] or dict(idx_head_stride=2 * ((T // 64 + 1) // 2))
    tail = (P, P, P, None, None, 1, cap, P, ld, P, P, 1, T, batch, 4, 11.3, None, None, 0, 1)
    kt = _lib.CacheView(P, P, P, P, 0, 0, 64, 0)
    if what != "flag of the lists per block":   # (with that flag it is a view of the other list form, and its pitch of 125 fits 124 blocks)
        assert L.mustafar_decode_attention_view(None, ctypes.byref(kt), ctypes.byref(_pairs_view(T, **wrong)), *tail, 0) == 1


def test_entry_points_refuse_a_pair_list_view_without_a_gpu():
    """Every native entry point but the one-pass super-block launch answers MUSTAFAR_EINVAL for a view flagged pair lists, before any
    launch (so it can be asked here)."""
    L = _lib.load()
    v, t = ctypes.byref(_pairs_view(256)), ctypes.byref(_lib.CacheView(P, P, P, P, 0, 0, 64, 0))
    r = ctypes.byref(_lib.CacheView(None, P, P, None, 0, 4, 16 * 40, _lib.VIEW_KEY_ROWS))
    assert L.mustafar_cache_rehouse(None, v, t, 1, 256, 0) == 1 and L.mustafar_cache_rehouse(None, t, v, 1, 256, 0) == 1
    assert L.mustafar_cache_append_bitmap_value(None, P, 1, 64, 128, v, 256, P) == 1
    assert L.mustafar_cache_append_pack_value(None, P, 1, 64, 128, v, 256) == 1
    assert L.mustafar_cache_consolidate_extents(None, v, P, 1, 1, 256, 0) == 1
    assert L.mustafar_decode_shared_segment(None, t, v, 256, 1, 4, 1, P, P, P, P, 11.3, 128) == 1
    assert L.mustafar_value_lists_to_tiles(None, v, t, 1, 256, P) == 1 and L.mustafar_value_lists_fill(None, t, v, 1, 256) == 1   # the other list form
    assert L.mustafar_key_rows_to_tiles(None, v, t, 1, 256, P) == 1 and L.mustafar_value_pair_lists_fill(None, t, r, 1, 256) == 1
    # a fused call: the key side has no such form, and neither two launches nor the matrix pipe nor a launch of two blocks per workgroup reads it
    tail = (P, P, P, None, None, 1, 64, P, 256 + 64, P, P, 1, 256, 4, 4, 11.3, None, None, 0, 1)
    kpairs = _lib.CacheView(P, P, P, P, 0, 0, 64, _lib.VIEW_VALUE_PAIR_LISTS)
    assert L.mustafar_decode_attention_view(None, ctypes.byref(kpairs), t, *tail, 0) == 1
    assert L.mustafar_decode_attention_view(None, t, v, *tail, _lib.STRUCTURE_FLAGS["two_launch"]) == 1
    assert L.mustafar_decode_attention_view(None, t, v, *tail, _lib.ENGINE_FLAGS["mfma"]) == 1
    assert L.mustafar_decode_attention_view(None, r, v, *tail, _lib.ENGINE_FLAGS["mfma"]) == 1
    assert L.mustafar_decode_reads_value_pair_lists(4, 256, 1, 320, 0) == 0 and L.mustafar_decode_attention_view(None, t, v, *tail, 0) == 1


def test_the_knobs_of_the_hook(monkeypatch):
    from mustafar_amd.cache import KEY_ROWS, VALUE_LISTS, VALUE_PAIR_LISTS
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    mk = lambda **kw: MustafarAttention(MustafarConfig(num_attention_heads=8, num_key_value_heads=2, api="fused", arena=True, **kw))
    wants = lambda a: [a._wants_form(f) for f in (KEY_ROWS, VALUE_LISTS, VALUE_PAIR_LISTS)]
    assert wants(mk()) == [True, True, True]
    assert wants(mk(value_pair_lists=False)) == [True, True, False]
    assert wants(mk(value_lists=False)) == [True, False, False], "the knob of the lists turns both list forms off"
    assert wants(mk(engine="mfma")) == [False, False, False]
    monkeypatch.setenv("MUSTAFAR_VALUE_PAIR_LISTS", "0")
    assert wants(mk()) == [True, True, False]
    monkeypatch.delenv("MUSTAFAR_VALUE_PAIR_LISTS")
    monkeypatch.setenv("MUSTAFAR_VALUE_LISTS", "0")
    assert wants(mk()) == [True, False, False]
