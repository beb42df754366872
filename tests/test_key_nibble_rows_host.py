"""CPU: nibble-row key blocks (include/mustafar_hip.h: MUSTAFAR_VIEW_KEY_NIBBLE_ROWS) without a GPU -- the NumPy reference of
both retile directions (tests/key_nibble_rows_ref.py, what tests/test_gpu_key_nibble_rows.py holds the device kernels to) on the special
blocks and on the oracle's compression, the header's arithmetic (csrc/key_nibble_rows.h, walked by tools/key_nibble_rows_check.cpp under
the address and undefined-behaviour sanitizers) against it, the bytes the form takes on the benchmark's data rule, the view rule and the
new symbols."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import key_nibble_rows_ref as ref
from mustafar_amd import _lib
from oracle import oracle as orc
from test_key_rows_host import reference_key_cache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1


@pytest.fixture(scope="module")
def encoded():
    """name -> (vals, kept, w, bytes) of the special blocks, encoded once."""
    out = {}
    for name in ref.SPECIAL_NAMES:
        vals, kept = ref.special_block(name)
        out[name] = (vals, kept) + ref.encode_block(vals, kept)
    return out


def test_the_special_blocks_are_what_they_are_meant_to_be(encoded):
    w = {n: e[2] for n, e in encoded.items()}
    assert w["full_beside_two"] == 128 and w["front_alone"] == 2 and w["ends"] == 4
    assert [w[f"w_mod8_{r}"] % 8 for r in (0, 2, 4, 6)] == [0, 2, 4, 6]
    gaps = set()
    for t in range(64):   # gaps of exactly 14, 15, 28 and 29 in both chains
        for part, ch in enumerate(ref.split(encoded["steps_14_15_28_29"][1][t], ref.front_of(w["steps_14_15_28_29"]))):
            gaps |= {(part, abs(a - b)) for a, b in zip(ch[1:], ch[:-1])}
    assert {(p, g) for p in (0, 1) for g in (14, 15, 28, 29)} <= gaps
    vals, kept = encoded["kept_zeros"][:2]
    assert (vals[0][kept[0]] == ref.PZERO).all() and (vals[2][kept[2]] == ref.NZERO).all() and kept[0].sum() == 40
    steps = [s[3] for s in ref.slots_of(encoded["front_alone"][3], 2)]
    assert len(steps) == 64 * 2 and all(s[1] == 0 for s in ref.slots_of(encoded["front_alone"][3], 2))   # no back share at all


def test_round_trip_of_every_special_block_is_the_identity_and_every_slot_stays_in_the_table(encoded):
    for name, (vals, kept, w, blk) in encoded.items():
        assert w % 2 == 0 and 2 <= w <= 128 and len(blk) == 256 * ref.rows_of(w), name
        v2, k2 = ref.decode_block(blk, w)
        assert np.array_equal(k2, kept) and np.array_equal(v2, vals), name   # (a kept +0 / -0 is an entry and comes back as one)
        slots = ref.slots_of(blk, w)
        assert len(slots) == 64 * w and all(-1 <= s[4] <= 128 for s in slots), name          # padding and spacers included
        assert all(0 <= s[4] <= 127 for s in slots if 1 <= s[3] <= 14), name                 # an entry is a channel
        assert all(s[5] == 0 for s in slots if s[3] in (0, 15)), name                        # padding and spacers carry +0
        if w > 2:   # w is the smallest width: two slots fewer and some token does not fit
            assert not all(ref.token_fits(kept[t], w - 2) for t in range(64)), name


def test_tiles_to_nibble_rows_to_tiles_is_the_identity_on_bitmaps_offsets_and_streams():
    vals, kept = ref.special_heads()   # two heads of unequal size, nine blocks each
    T = vals.shape[1]
    tiles = [ref.to_tiles(vals[h], kept[h]) for h in range(2)]
    bmp, idx, nzs = np.stack([t[0] for t in tiles]), np.stack([t[1] for t in tiles]), [t[2] for t in tiles]
    table, rows = ref.tiles_to_rows(bmp, idx, nzs, T)
    assert rows[0].size != rows[1].size
    for h in range(2):
        first = 0
        for b in range(T // 64):
            assert table[h, b] >> 8 == first
            first += ref.rows_of(int(table[h, b] & 0xFF))
        assert rows[h].size == 256 * first
    b2, i2, n2 = ref.rows_to_tiles(table, rows, T)
    assert np.array_equal(b2, bmp) and np.array_equal(i2, idx) and all(np.array_equal(a, b) for a, b in zip(n2, nzs))


@pytest.mark.parametrize("blocks", [1, 5])
def test_round_trip_on_oracle_compression(blocks):
    rng = np.random.default_rng(blocks)
    x = orc.prune_magnitude(rng.standard_normal((2, 64 * blocks, 128)).astype(np.float16), 0.7)
    x[1, 3] = 0
    bmp, idx, nzs = reference_key_cache(x)
    table, rows = ref.tiles_to_rows(bmp, idx, nzs, 64 * blocks)
    b2, i2, n2 = ref.rows_to_tiles(table, rows, 64 * blocks)
    assert np.array_equal(b2, bmp) and np.array_equal(i2, idx) and all(np.array_equal(a, b) for a, b in zip(n2, nzs))


def test_bytes_per_token_on_the_benchmark_data_rule():
    """N(0, 1) fp16 pruned by the reference rule: at 70 % no more than 110 bytes per token and kv head (token rows with channel bytes: 126
    and the table).  Measured: 168.2 at 50 %, 108.1 at 70 %, 76.2 at 80 % (100 blocks x 2 heads)."""
    rng = np.random.default_rng(0)
    got = {}
    for sparsity in (0.5, 0.7, 0.8):
        got[sparsity] = ref.bytes_per_token(orc.prune_magnitude(rng.standard_normal((2, 64 * 24, 128)).astype(np.float16), sparsity))
    print("bytes per token and kv head:", got)
    assert got[0.7] <= 110.0
    assert got[0.8] < got[0.7] < got[0.5]


def test_the_host_program_agrees_with_the_reference_under_sanitizers(tmp_path, encoded):
    exe = str(tmp_path / "key_nibble_rows_check")
    subprocess.check_call(["c++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tools", "key_nibble_rows_check.cpp")])   # (a program of its own: the sanitizers' runtimes are linked in)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = [l.split() for l in out.stdout.strip().splitlines()]
    assert [l[0] for l in lines] == list(ref.SPECIAL_NAMES)
    for name, w, size, crc in lines:
        _, _, rw, blk = encoded[name]
        assert (int(w), int(size), int(crc, 16)) == (rw, len(blk), ref.crc_of(rw, blk)), name


def test_the_header_declares_and_the_library_exports_the_new_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mustafar_hip.h")).read(), flags=re.S)
    syms = set(re.findall(r"\b(mustafar_\w+)\s*\(", text))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("mustafar_key_nibble_rows_plan", "mustafar_key_nibble_rows_fill", "mustafar_key_nibble_rows_to_tiles",
              "mustafar_decode_reads_key_nibble_rows"):
        assert s in syms and s in _lib.SIGNATURES and hasattr(raw, s), s
    assert _lib.load().mustafar_abi_version() == 115
    assert "MUSTAFAR_VIEW_KEY_NIBBLE_ROWS 8u" in text and _lib.VIEW_KEY_NIBBLE_ROWS == 8
    L = _lib.load()
    for args in ((4, 7936, 64, 8224, 0), (4, 7936, 64, 8232, 0), (4, 1792, 8, 2112, 0), (1, 7936, 256, 8224, 0),
                 (4, 7936, 64, 8224, _lib.ENGINE_FLAGS["mfma"])):
        assert L.mustafar_decode_reads_key_nibble_rows(*args) == L.mustafar_decode_reads_key_rows(*args), args
    assert L.mustafar_decode_reads_key_nibble_rows(4, 7936, 64, 8224, 0) == 1


_P = ctypes.addressof((ctypes.c_uint64 * 64)())
_GOOD = dict(bmp=None, nz=_P, idx=_P, nz_offset=None, bmp_head_stride=0, idx_head_stride=4, nz_head_stride=16 * 40, flags=_lib.VIEW_KEY_NIBBLE_ROWS)
_MALFORMED = {"flag of the rows with channel bytes": dict(flags=_lib.VIEW_KEY_ROWS), "flag of pair lists": dict(flags=_lib.VIEW_VALUE_PAIR_LISTS),
              "two flags": dict(flags=_lib.VIEW_KEY_NIBBLE_ROWS | _lib.VIEW_KEY_ROWS), "no table": dict(idx=None), "no rows": dict(nz=None),
              "no head stride": dict(nz_head_stride=0), "a head stride that is no whole row": dict(nz_head_stride=16 * 40 + 8),
              "a table shorter than the blocks": dict(idx_head_stride=3)}


def _view(**kw):
    f = dict(_GOOD, **kw)
    return _lib.CacheView(f["bmp"], f["nz"], f["idx"], f["nz_offset"], f["bmp_head_stride"], f["idx_head_stride"], f["nz_head_stride"], f["flags"])


@pytest.mark.parametrize("what", sorted(_MALFORMED))
def test_the_view_rule_refuses_a_malformed_view(what):
    L = _lib.load()
    tiles = ctypes.byref(_lib.CacheView(_P, _P, _P, _P, 0, 0, 64, 0))
    bad = ctypes.byref(_view(**_MALFORMED[what]))
    assert L.mustafar_key_nibble_rows_to_tiles(None, bad, tiles, 1, 256, _P) == EINVAL
    assert L.mustafar_key_nibble_rows_fill(None, tiles, bad, 1, 256) == EINVAL


def test_entry_points_answer_einval_for_a_wrong_source_form_and_outside_the_one_launch():
    L = _lib.load()
    p = _P
    nib, tiles = _view(), _lib.CacheView(p, p, p, p, 0, 0, 64, 0)
    rows = _view(flags=_lib.VIEW_KEY_ROWS)
    n, t, r = ctypes.byref(nib), ctypes.byref(tiles), ctypes.byref(rows)
    assert L.mustafar_key_nibble_rows_plan(None, n, 1, 256, p, p) == EINVAL and L.mustafar_key_nibble_rows_plan(None, r, 1, 256, p, p) == EINVAL
    assert L.mustafar_key_nibble_rows_fill(None, n, n, 1, 256) == EINVAL and L.mustafar_key_nibble_rows_fill(None, t, t, 1, 256) == EINVAL
    assert L.mustafar_key_nibble_rows_fill(None, t, r, 1, 256) == EINVAL
    assert L.mustafar_key_nibble_rows_to_tiles(None, t, t, 1, 256, p) == EINVAL and L.mustafar_key_nibble_rows_to_tiles(None, r, t, 1, 256, p) == EINVAL
    assert L.mustafar_key_rows_to_tiles(None, n, t, 1, 256, p) == EINVAL and L.mustafar_key_rows_fill(None, t, n, 1, 256) == EINVAL
    assert L.mustafar_value_pair_lists_to_tiles(None, n, t, 1, 256, p) == EINVAL
    # every other native entry point
    assert L.mustafar_cache_rehouse(None, n, t, 1, 256, 0) == EINVAL and L.mustafar_cache_rehouse(None, t, n, 1, 256, 0) == EINVAL
    assert L.mustafar_cache_append_bitmap_key(None, p, 1, 64, 128, n, 256, p) == EINVAL
    assert L.mustafar_cache_append_pack_key(None, p, 1, 64, 128, n, 256) == EINVAL
    assert L.mustafar_cache_consolidate_extents(None, n, p, 1, 1, 256, 0) == EINVAL
    assert L.mustafar_decode_shared_segment(None, n, t, 256, 1, 4, 1, p, p, p, p, 11.3, 128) == EINVAL
    # a fused call: the value side has no such form; nibble rows are read next to pair lists only; not by two launches or the matrix pipe
    tail = (p, p, p, None, None, 1, 64, p, 256 + 64, p, p, 1, 256, 4, 4, 11.3, None, None, 0, 1)
    pairs = ctypes.byref(_lib.CacheView(None, p, p, None, 0, 5, 16 * 40, _lib.VIEW_VALUE_PAIR_LISTS))
    lists = ctypes.byref(_lib.CacheView(None, p, p, None, 0, 5, 16 * 40, _lib.VIEW_VALUE_LISTS))
    assert L.mustafar_decode_attention_view(None, t, n, *tail, 0) == EINVAL
    assert L.mustafar_decode_attention_view(None, n, t, *tail, 0) == EINVAL
    assert L.mustafar_decode_attention_view(None, n, lists, *tail, 0) == EINVAL
    assert L.mustafar_decode_attention_view(None, n, pairs, *tail, _lib.STRUCTURE_FLAGS["two_launch"]) == EINVAL
    assert L.mustafar_decode_attention_view(None, n, pairs, *tail, _lib.ENGINE_FLAGS["mfma"]) == EINVAL
    assert L.mustafar_decode_attention_view(None, n, pairs, *tail, 0) == EINVAL   # (this shape runs two blocks per workgroup: no form is read)


def test_the_hook_prefers_nibble_rows_only_where_pair_lists_are_wanted(monkeypatch):
    from mustafar_amd.cache import BASE_FORMS, KEY_NIBBLE_ROWS, KEY_ROWS, ROW_FORMS
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    assert KEY_NIBBLE_ROWS in BASE_FORMS and ROW_FORMS == (KEY_ROWS, KEY_NIBBLE_ROWS) and KEY_NIBBLE_ROWS.flag == 8
    mk = lambda **kw: MustafarAttention(MustafarConfig(num_attention_heads=8, num_key_value_heads=2, api="fused", arena=True, **kw))
    assert mk()._wants_form(KEY_NIBBLE_ROWS)
    for off in (dict(key_nibble_rows=False), dict(key_rows=False), dict(value_pair_lists=False), dict(value_lists=False), dict(engine="mfma")):
        assert not mk(**off)._wants_form(KEY_NIBBLE_ROWS), off
    assert mk(key_nibble_rows=False)._wants_form(KEY_ROWS)
    monkeypatch.setenv("MUSTAFAR_KEY_NIBBLE_ROWS", "0")
    assert not mk()._wants_form(KEY_NIBBLE_ROWS) and mk()._wants_form(KEY_ROWS)
