"""CPU: the head_dim-64 surface of the C ABI and of the hook, checked without a GPU (no kernel runs)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mustafar_decode_attention_hd", "mustafar_decode_workspace_bytes_hd")


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "mustafar_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"^\s*(?:int|int64_t)\s+(\w+)\s*\(", text, flags=re.M))


def test_new_symbols_are_declared_bound_and_exported():
    from mustafar_amd import _lib
    syms = _header_symbols()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert s in syms and s in _lib.SIGNATURES and hasattr(raw, s)
    assert _lib.load().mustafar_abi_version() >= 107


def _hd_args(**kw):
    one = 16   # never dereferenced: validation fails first (16-byte aligned, so that only the argument under test is wrong)
    a = dict(k_bmp=one, k_nz=one, k_idx=one, k_off=one, v_bmp=one, v_nz=one, v_idx=one, v_off=one, q=one, kw=one, vw=one, kn=None, vn=None,
             wl=1, wc=64, scores=one, ld=128 + 64, out=one, ws=one, split=1, T=128, BH=4, groups=1, sqrt_d=8.0, extra=None, mask=None,
             mstride=0, mheads=0, flags=0, head_dim=64)
    a.update(kw)
    return a


def _call(L, a):
    return L.mustafar_decode_attention_hd(None, a["k_bmp"], a["k_nz"], a["k_idx"], a["k_off"], a["v_bmp"], a["v_nz"], a["v_idx"], a["v_off"],
                                          a["q"], a["kw"], a["vw"], a["kn"], a["vn"], a["wl"], a["wc"], a["scores"], a["ld"], a["out"], a["ws"],
                                          a["split"], a["T"], a["BH"], a["groups"], ctypes.c_float(a["sqrt_d"]), a["extra"], a["mask"],
                                          a["mstride"], a["mheads"], a["flags"], a["head_dim"])


@pytest.mark.parametrize("bad", [
    dict(head_dim=96), dict(head_dim=0), dict(head_dim=256),           # unsupported head_dim
    dict(q=None), dict(out=None), dict(ws=None), dict(kw=None), dict(scores=None), dict(k_bmp=None), dict(v_off=None),   # null operands
    dict(ld=128 + 63), dict(ld=100), dict(ld=128 + 64 + 4),            # ld_scores too short / not a multiple of 8
    dict(extra=16, ld=128 + 8),                                        # with a step counter ld_scores must cover the capacity
    dict(T=100), dict(groups=9, BH=9), dict(BH=6, groups=4), dict(wl=0), dict(wl=65), dict(wc=2048, wl=1, ld=128 + 2048),
    dict(sqrt_d=0.0), dict(split=0), dict(kw=24), dict(kn=40),         # misaligned window / new row
    dict(flags=1 << 4),                                                 # two launches: no head_dim-64 form
    dict(flags=1 << 7), dict(flags=4),                                  # undefined flag bits / engine
    dict(mask=16, mheads=0), dict(mask=16, mheads=3),                   # mask rows per head that do not divide the batch
])
def test_decode_hd_rejects_bad_arguments_without_a_launch(bad):
    from mustafar_amd import _lib
    assert _call(_lib.load(), _hd_args(**bad)) == 1


def test_decode_hd_t0_needs_no_cache_pointers_but_checks_the_rest():
    from mustafar_amd import _lib
    L = _lib.load()
    # T = 0 without cache pointers passes the cache check and fails on the missing query only
    args = _hd_args(T=0, ld=64, k_bmp=None, k_nz=None, k_idx=None, k_off=None, v_bmp=None, v_nz=None, v_idx=None, v_off=None, q=None)
    assert _call(L, args) == 1


def test_workspace_helper_by_head_dim():
    from mustafar_amd import _lib
    L = _lib.load()
    for T, BH, g in [(0, 8, 4), (7936, 256, 4), (32512, 256, 4), (4096, 7, 7), (64, 1, 1)]:
        assert L.mustafar_decode_workspace_bytes_hd(T, BH, g, 3, 128) == L.mustafar_decode_workspace_bytes(T, BH, g, 3)
        ws = L.mustafar_decode_workspace_bytes_hd(T, BH, g, 1, 64)
        assert ws >= (T // 64 // 1024 + 16) * BH * 66 * 4 and ws > 0
        assert ws <= (T // 64 + 16) * BH * 66 * 4   # at most one slab per block and window chunk
    assert L.mustafar_decode_workspace_bytes_hd(7936, 256, 4, 1, 96) == 0
    assert L.mustafar_decode_workspace_bytes_hd(7936, 6, 4, 1, 64) == 0


def test_conversion_entry_points_keep_d64_out_of_the_onepass_forms():
    """D = 64 is two-pass only: the one-pass conversion, the cache append and the trigger batch reject it on the host."""
    from mustafar_amd import _lib
    L = _lib.load()
    one = ctypes.c_void_p(16)
    assert L.mustafar_convert_onepass(None, one, 2, 64, 64, 1, one, one, one, one, one, one) == 1
    assert L.mustafar_convert_pack(None, one, 2, 64, 64, one, one) == 1
    assert L.mustafar_cache_append_kv(None, one, one, 64 * 64, 2, 64, 64, 1, 1, None, None, 0, one, one, 0, 0, one, one) == 1
    # the two-pass calls validate their shapes at D = 64 too
    assert L.mustafar_compress_bitmap_key(None, one, 2, 100, 64, one, one, one) == 1
    assert L.mustafar_compress_pack_value(None, one, 0, 64, 64, one, one, one, one) == 1
    assert L.mustafar_prune_magnitude(None, one, one, 4, 64, 65) == 1
    assert L.mustafar_prune_magnitude(None, one, one, 4, 64, 0) == 1
    assert L.mustafar_prune_magnitude(None, one, one, 4, 96, 10) == 1


def test_hook_construction_rules_for_head_dim_64():
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    MustafarAttention(MustafarConfig(num_attention_heads=32, num_key_value_heads=8, head_dim=64, api="fused"))
    for kw in (dict(api="native"), dict(api="reference"), dict(api="fused", arena=True)):
        with pytest.raises(ValueError, match="api='fused', arena=False"):
            MustafarAttention(MustafarConfig(head_dim=64, **kw))
    MustafarAttention(MustafarConfig(head_dim=128, api="native"))   # other head dims behave as before
    MustafarAttention(MustafarConfig(head_dim=128, api="fused", arena=True))
