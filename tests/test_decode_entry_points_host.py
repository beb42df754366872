"""CPU: one table of single-fault argument sets sent through all seven fused decode entry points (no kernel runs).

Every row is a call with exactly one thing wrong, so every call must come back with 1 (MUSTAFAR_EINVAL) before anything is
launched: the pointers are made up.  The seven entry points fill one descriptor and share one dispatcher; the
table pins what each of them refuses, at head_dim 64 and 128 where the entry point takes a head_dim.  No row is a complete valid
call: a row that is not refused is a wrong row, not an expected result."""
import ctypes

import pytest

ONE = 16   # never dereferenced: validation fails first (16-byte aligned, so that only the argument under test is wrong)


def _base(**kw):
    a = dict(q=ONE, kw=ONE, vw=ONE, kn=ONE, vn=ONE, wl=1, wc=64, scores=ONE, ld=None, out=ONE, ws=ONE, split=1, T=256, BH=4, groups=1,
             sqrt_d=8.0, extra=None, mask=None, mstride=0, mheads=0, flags=0,
             T_base=256, tables=True, t_device=None)
    a.update(kw)
    if a["ld"] is None:   # the base call's ld_scores: 320 at T = 256
        a["ld"] = a["T"] + 64
    return a


def _tail(a):
    return (a["q"], a["kw"], a["vw"], a["kn"], a["vn"], a["wl"], a["wc"], a["scores"], a["ld"], a["out"], a["ws"], a["split"], a["T"],
            a["BH"], a["groups"], ctypes.c_float(a["sqrt_d"]), a["extra"], a["mask"], a["mstride"], a["mheads"], a["flags"])


def _views(nz_head_stride=0):
    from mustafar_amd._lib import CacheView
    return CacheView(ONE, ONE, ONE, ONE, 0, 0, nz_head_stride), CacheView(ONE, ONE, ONE, ONE, 0, 0, nz_head_stride)


def _arrays(name, head_dim=None, lse=False):
    def call(L, a):
        rest = ([head_dim] if head_dim else []) + ([ONE] if lse else [])
        return getattr(L, name)(None, *([ONE] * 8), *_tail(a), *rest)
    return call


def _view(L, a):
    k, v = _views()
    return L.mustafar_decode_attention_view(None, ctypes.byref(k), ctypes.byref(v), *_tail(a))


def _extents(name, head_dim=None, lse=False):
    def call(L, a):
        k, v = _views(64 if a["T"] > a["T_base"] else 0)   # (a grown cache: equally spaced stream regions)
        rest = [a["t_device"]] + ([head_dim] if head_dim else []) + ([ONE] if lse else [])
        tab = ONE if a["tables"] else None
        return getattr(L, name)(None, ctypes.byref(k), ctypes.byref(v), a["T_base"], tab, tab, *_tail(a), *rest)
    return call


# (label, head_dim or None, takes an LSE, takes extents, the call)
ENTRIES = [("decode_attention", 128, False, False, _arrays("mustafar_decode_attention")),
           ("decode_attention_view", 128, False, False, _view),
           ("decode_attention_extents", 128, False, True, _extents("mustafar_decode_attention_extents"))]
for _d in (64, 128):
    ENTRIES += [(f"decode_attention_hd@{_d}", _d, False, False, _arrays("mustafar_decode_attention_hd", _d)),
                (f"decode_attention_lse_hd@{_d}", _d, True, False, _arrays("mustafar_decode_attention_lse_hd", _d, True)),
                (f"decode_attention_extents_hd@{_d}", _d, False, True, _extents("mustafar_decode_attention_extents_hd", _d)),
                (f"decode_attention_extents_lse_hd@{_d}", _d, True, True, _extents("mustafar_decode_attention_extents_lse_hd", _d, True))]
EVERY = lambda e: True
# (id, the one wrong thing, which entries it applies to).  ld_scores faults are written relative to T (319 and 324 at T = 256).
FAULTS = [
    ("null_q", dict(q=None), EVERY), ("null_out", dict(out=None), EVERY), ("null_workspace", dict(ws=None), EVERY),
    ("null_scores", dict(scores=None), EVERY),
    ("ld_not_multiple_of_8_low", dict(ld_minus_T=63), EVERY), ("ld_not_multiple_of_8_high", dict(ld_minus_T=68), EVERY),
    ("T_100", dict(T=100, ld=320), EVERY), ("batch_not_multiple_of_groups", dict(BH=6, groups=4), EVERY),
    ("window_len_over_capacity", dict(wl=65), EVERY), ("window_capacity_2048", dict(wc=2048, ld_minus_T=2048), EVERY),
    ("sqrt_d_0", dict(sqrt_d=0.0), EVERY), ("split_k_0", dict(split=0), EVERY),
    ("flags_undefined_bit", dict(flags=1 << 7), EVERY), ("flags_engine_4", dict(flags=4), EVERY),
    ("mask_heads_0", dict(mask=ONE, mheads=0), EVERY), ("mask_heads_3", dict(mask=ONE, mheads=3), EVERY),
    ("window_len_0_with_a_window", dict(wl=0), EVERY),
    ("two_launches_at_head_dim_64", dict(flags=1 << 4), lambda e: e[1] == 64),
    ("T_base_128", dict(T_base=128), lambda e: e[3]),
    ("T_device_without_room", dict(t_device=ONE, T=256), lambda e: e[3]),
    ("T_384", dict(T=384), lambda e: e[3]),
    ("null_tables", dict(T=512, tables=False), lambda e: e[3]),
    ("half_window_less", dict(wl=0, wc=0, vw=None, kn=None, vn=None), lambda e: e[2]),   # k_window still set
]


def _cases(fault, entry):
    """The base call(s) of an entry with the fault applied: the extents entry points also over T = 512 (one appended extent's worth
    beyond T_base = 256, real views with nz_head_stride = 64 and non-null tables)."""
    for T in (256, 512) if entry[3] else (256,):
        kw = dict(fault)
        kw.setdefault("T", T)
        if "ld_minus_T" in kw:
            kw["ld"] = kw["T"] + kw.pop("ld_minus_T")
        yield _base(**kw)


@pytest.mark.parametrize("fid,fault,applies", FAULTS, ids=[f[0] for f in FAULTS])
def test_every_entry_point_refuses_the_fault(fid, fault, applies):
    from mustafar_amd import _lib
    L = _lib.load()
    tried = 0
    for entry in ENTRIES:
        if not applies(entry):
            continue
        for a in _cases(fault, entry):
            tried += 1
            assert entry[4](L, a) == 1, f"{fid}: {entry[0]} at T = {a['T']} was not refused"
    assert tried


def test_table_reaches_all_seven_entry_points():
    names = {e[0].split("@")[0] for e in ENTRIES}
    assert names == {"decode_attention", "decode_attention_view", "decode_attention_hd", "decode_attention_lse_hd",
                     "decode_attention_extents", "decode_attention_extents_hd", "decode_attention_extents_lse_hd"}
