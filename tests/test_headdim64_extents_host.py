"""CPU: the head_dim-64 extent surface of the C ABI (ABI 108), of the hook's configuration and the run shapes the GPU tests of
tests/test_gpu_headdim64_extents.py rely on.  No kernel runs: every call here must fail validation before a launch."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mustafar_decode_attention_extents_hd", "mustafar_trigger_compress_batch_hd", "mustafar_trigger_finish_batch_hd")
# name -> (B', T_base, extents, bpw, S1): the straddle shapes (T = T_base + 256 extents is a row of tests/hd64_util.RUN_SHAPES)
# bpw3x: the same T as bpw3 from a base of 148 blocks + 3 extents, so that one run of 3 crosses base -> extent (block 148) and the next
# but one crosses extent -> extent (block 152); in bpw3 itself the second extent starts on a run boundary (block 156 = 3 x 52).
EXT_SHAPES = {"bpw3": (64, 9728, 2, 3, 54), "bpw3x": (64, 9472, 3, 3, 54), "bpw2": (64, 7424, 2, 2, 62)}


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "mustafar_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"^\s*(?:int|int64_t)\s+(\w+)\s*\(", text, flags=re.M))


def test_new_symbols_are_declared_bound_and_exported():
    from mustafar_amd import _lib
    syms = _header_symbols()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert s in syms and s in _lib.SIGNATURES and hasattr(raw, s), s
    assert _lib.load().mustafar_abi_version() >= 108


def _view(**kw):
    from mustafar_amd import _lib
    a = dict(bmp=16, nz=16, idx=16, nz_offset=16, bmp_head_stride=0, idx_head_stride=0, nz_head_stride=0)
    a.update(kw)
    return _lib.CacheView(**a)


def _dec_args(**kw):
    one = 16   # never dereferenced: validation fails first
    a = dict(k_base=_view(), v_base=_view(), T_base=256, k_ext=one, v_ext=one, q=one, kw=one, vw=one, kn=None, vn=None, wl=1, wc=64,
             scores=one, ld=512 + 64, out=one, ws=one, split=1, T=512, BH=4, groups=1, sqrt_d=8.0, extra=None, mask=None, mstride=0,
             mheads=0, flags=0, t_dev=None, head_dim=64)
    a.update(kw)
    return a


def _dec(L, a):
    r = lambda v: ctypes.byref(v) if v is not None else None
    return L.mustafar_decode_attention_extents_hd(None, r(a["k_base"]), r(a["v_base"]), a["T_base"], a["k_ext"], a["v_ext"], a["q"], a["kw"],
                                                  a["vw"], a["kn"], a["vn"], a["wl"], a["wc"], a["scores"], a["ld"], a["out"], a["ws"],
                                                  a["split"], a["T"], a["BH"], a["groups"], ctypes.c_float(a["sqrt_d"]), a["extra"], a["mask"],
                                                  a["mstride"], a["mheads"], a["flags"], a["t_dev"], a["head_dim"])


@pytest.mark.parametrize("bad", [
    dict(head_dim=96), dict(head_dim=0),
    dict(T_base=320, T=576, ld=576 + 64),                   # T_base % 256 != 0
    dict(T_base=0, T=256), dict(T_base=-256, T=0),          # no base
    dict(T=640, ld=640 + 64), dict(T=256 + 64, ld=384),     # (T - T_base) % 256 != 0
    dict(T=128),                                            # T < T_base
    dict(T=256 + 513 * 256, ld=256 + 513 * 256 + 64),       # more than 512 extents
    dict(k_ext=None), dict(v_ext=None),                     # null tables with T > T_base
    dict(k_base=None), dict(v_base=None),
    dict(T=256, ld=256 + 64, t_dev=16),                     # a device-side T with a capacity of exactly the base
    dict(kw=24), dict(vw=8), dict(kn=40),                   # misaligned windows / new row
    dict(q=None), dict(out=None), dict(ws=None), dict(scores=None),
    dict(ld=512 + 63), dict(ld=512 + 60), dict(extra=16, wc=128, ld=512 + 64),
    dict(groups=9, BH=9), dict(BH=6, groups=4), dict(wl=0), dict(wl=65), dict(sqrt_d=0.0), dict(split=0),
    dict(flags=1 << 4), dict(flags=1 << 7), dict(flags=4),
    dict(mask=16, mheads=0), dict(mask=16, mheads=3),
])
def test_decode_extents_hd_rejects_bad_arguments_without_a_launch(bad):
    from mustafar_amd import _lib
    assert _dec(_lib.load(), _dec_args(**bad)) == 1


def test_decode_extents_hd_checks_the_base_views():
    from mustafar_amd import _lib
    L = _lib.load()
    for kw in (dict(bmp=None), dict(idx=None), dict(nz=None), dict(nz_offset=None), dict(bmp_head_stride=128), dict(idx_head_stride=256),
               dict(nz_head_stride=-1)):
        assert _dec(L, _dec_args(k_base=_view(**kw))) == 1, kw
        assert _dec(L, _dec_args(v_base=_view(**kw))) == 1, kw
    # head_dim 128 forwards to mustafar_decode_attention_extents, which validates on its own (T_base % 256)
    assert _dec(L, _dec_args(head_dim=128, T_base=320, T=576)) == 1


def _item(**kw):
    from mustafar_amd import _lib
    ext = dict(bmp_head_stride=256, idx_head_stride=257, nz_head_stride=64)
    a = dict(k_window=64, v_window=64, k_dst=_view(**ext), v_dst=_view(**ext), k_table_slot=None, v_table_slot=None, k_head_total=16,
             v_head_total=16, overflow_flag=16)
    a.update(kw)
    return (_lib.TriggerItem * 1)(_lib.TriggerItem(**a))


def _compress(L, items=None, n=1, hs=320 * 64, Bp=2, t=256, D=64, kk=44, kv=44, kr=512, vr=512):
    return L.mustafar_trigger_compress_batch_hd(None, n, items if items is not None else _item(), hs, Bp, t, D, kk, kv, kr, vr, None)


def test_trigger_compress_hd_rejects_bad_arguments_without_a_launch():
    from mustafar_amd import _lib
    L = _lib.load()
    assert _compress(L, D=128) == 1 and _compress(L, D=96) == 1
    assert _compress(L, t=128) == 1 and _compress(L, t=512, hs=512 * 64) == 1 and _compress(L, t=64) == 1
    assert _compress(L, n=0) == 1 and _compress(L, Bp=0) == 1 and _compress(L, hs=255 * 64) == 1 and _compress(L, hs=320 * 64 + 4) == 1
    assert _compress(L, kk=65) == 1 and _compress(L, kv=-1) == 1
    assert _compress(L, kr=0) == 1 and _compress(L, vr=520) == 1       # no region size / more than the views' stride holds
    assert _compress(L, items=_item(overflow_flag=None)) == 1
    assert _compress(L, items=_item(k_window=72)) == 1 and _compress(L, items=_item(v_window=8)) == 1 and _compress(L, items=_item(k_window=None)) == 1
    assert _compress(L, items=_item(k_head_total=None)) == 1 and _compress(L, items=_item(v_head_total=None)) == 1
    ext = dict(bmp_head_stride=256, idx_head_stride=257, nz_head_stride=64)
    for kw in (dict(nz_head_stride=0), dict(bmp_head_stride=128), dict(idx_head_stride=256), dict(bmp=None), dict(idx=None), dict(nz=None),
               dict(nz=24)):
        v = dict(ext)
        v.update(kw)
        assert _compress(L, items=_item(k_dst=_view(**v))) == 1, kw
        assert _compress(L, items=_item(v_dst=_view(**v))) == 1, kw
    # the D = 128 batch call still refuses head_dim 64
    assert L.mustafar_trigger_compress_batch(None, 1, _item(), 320 * 64, 2, 256, 64, 44, 44, 512, 512, 16) == 1


def test_trigger_finish_hd_rejects_bad_arguments_without_a_launch():
    from mustafar_amd import _lib
    L = _lib.load()
    f = lambda items=None, n=1, hs=320 * 64, Bp=2, ln=288, drop=256, D=64: L.mustafar_trigger_finish_batch_hd(
        None, n, items if items is not None else _item(), hs, Bp, ln, drop, D)
    assert f(D=96) == 1 and f(n=0) == 1 and f(Bp=0) == 1 and f(drop=-1) == 1 and f(ln=200) == 1 and f(hs=287 * 64) == 1
    assert f(items=_item(k_window=None)) == 1 and f(items=_item(v_window=24)) == 1
    assert f(D=128, hs=287 * 128) == 1   # forwarded: the D = 128 call's own check of head_stride against rows of 128 halfs


def test_hd64_extents_configuration_rules():
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    MustafarAttention(MustafarConfig(num_attention_heads=32, num_key_value_heads=8, head_dim=64, api="fused", hd64_extents=True))
    assert MustafarConfig().hd64_extents is False
    with pytest.raises(ValueError, match="hd64_extents"):
        MustafarAttention(MustafarConfig(head_dim=128, api="fused", hd64_extents=True))
    with pytest.raises(ValueError, match="hd64_extents"):
        MustafarAttention(MustafarConfig(head_dim=128, api="native", hd64_extents=True))
    for kw in (dict(api="native"), dict(api="fused", arena=True)):
        with pytest.raises(ValueError):
            MustafarAttention(MustafarConfig(head_dim=64, hd64_extents=True, **kw))


def test_extent_run_shapes():
    """The straddle shapes: T on the 256 grid, the run shape of hd64_util.RUN_SHAPES' row of the same name (or of bpw2_full), and a
    run of bpw blocks that crosses base -> extent and extent -> extent."""
    from mustafar_amd import _lib
    from tests.hd64_util import RUN_SHAPES, run_shape
    L = _lib.load()
    assert RUN_SHAPES["bpw2"][1] % 256 != 0, "T = 8000 is not on the 256 grid: the extent test uses 7936"
    for name, (Bp, T_base, n_ext, bpw, S1) in EXT_SHAPES.items():
        T = T_base + 256 * n_ext
        assert T_base % 256 == 0 and T == RUN_SHAPES["bpw3" if name.startswith("bpw3") else "bpw2_full"][1]
        for g in (1, 4, 8):
            assert run_shape(L, T, Bp * g, g) == (S1, bpw), (name, g)
        runs = [(r * bpw, min(T // 64, r * bpw + bpw)) for r in range(S1)]
        edges = [T_base // 64 + 4 * i for i in range(n_ext)]
        crossed = [e for e in edges if any(a < e < b for a, b in runs)]
        if name == "bpw3":
            assert crossed == [T_base // 64], "bpw3: a run must cross base -> extent"
        if name == "bpw3x":
            assert crossed == edges[:2], "bpw3x: one run must cross base -> extent and another extent -> extent"
    # the small shapes of the bit-equality tests: one block per workgroup
    for T in (512, 768, 1024, 1280):
        for g in (1, 4, 8):
            assert run_shape(L, T, 2 * g, g) == (T // 64, 1)
