"""CPU: the ragged-batch surface (mustafar_sequence, mustafar_ragged_set_sequences, mustafar_decode_ragged and its workspace size;
RaggedBatch / MustafarAttention.decode_ragged) checked without a GPU: every C call here fails validation before any launch -- a null
stream and addresses that are never dereferenced --, and every Python refusal comes before any device work."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mustafar_decode_ragged_workspace_bytes", "mustafar_ragged_set_sequences", "mustafar_decode_ragged")
ONE = 16   # a pointer that is never dereferenced (16-byte aligned, so that only the argument under test is wrong)
VIEW = (ONE, ONE, ONE, ONE, 0, 0, 0)


def _lib():
    from mustafar_amd import _lib as lib
    return lib.load()


def test_the_three_symbols_are_declared_bound_and_exported_at_abi_115():
    from mustafar_amd import _lib as lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mustafar_hip.h")).read(), flags=re.S)
    syms = set(re.findall(r"^\s*(?:int|int64_t)\s+(\w+)\s*\(", text, flags=re.M))
    raw = ctypes.CDLL(lib.LIB_PATH)
    for s in NEW:
        assert s in syms and s in lib.SIGNATURES and hasattr(raw, s), s
    assert _lib().mustafar_abi_version() == 115


def test_the_sequence_structure_is_the_headers():
    """176 bytes, the offsets of the header's comment."""
    from mustafar_amd import _lib as lib
    S = lib.Sequence
    assert ctypes.sizeof(S) == 176 and ctypes.sizeof(lib.CacheView) == 64
    want = dict(k_base=0, v_base=64, k_extents=128, v_extents=136, k_window=144, v_window=152, T_base=160, T=164, window_len=168,
                window_capacity=172)
    assert {name: getattr(S, name).offset for name in want} == want
    text = open(os.path.join(ROOT, "include", "mustafar_hip.h")).read()
    for name, off in want.items():
        assert re.search(rf"{name} at {off}\b", text), f"the header does not say `{name} at {off}`"


@pytest.mark.parametrize("D", [64, 128])
def test_the_workspace_is_the_multi_query_calls(D):
    L = _lib()
    for T in (0, 64, 768, 4096):
        for cap in (16, 64, 320, 1024):
            for n, kv in ((1, 1), (3, 2), (8, 8)):
                for g, nq in ((1, 1), (4, 1), (2, 3), (4, 4), (8, 8), (4, 16)):
                    got = L.mustafar_decode_ragged_workspace_bytes(T, cap, n, kv, g, nq, D)
                    assert got == L.mustafar_decode_multi_query_workspace_bytes(T, cap, n * kv, g, nq, D) and got > 0


# ---- mustafar_decode_ragged ---------------------------------------------------------------------------------------------------------------
def _decode(L, **kw):
    """One call with every argument valid but those in `kw`: (error, workspace bytes of the same shape)."""
    a = dict(table=ONE, n=3, kv=2, groups=4, n_q=2, T=768, cap=320, q=ONE, kn=ONE, vn=ONE, out=ONE, lse=ONE, ws=ONE, sqrt_d=8.0, D=64)
    a.update(kw)
    err = L.mustafar_decode_ragged(None, a["table"], a["n"], a["kv"], a["groups"], a["n_q"], a["T"], a["cap"], a["q"], a["kn"], a["vn"],
                                   a["out"], a["lse"], a["ws"], ctypes.c_float(a["sqrt_d"]), a["D"])
    return err, L.mustafar_decode_ragged_workspace_bytes(a["T"], a["cap"], a["n"], a["kv"], a["groups"], a["n_q"], a["D"])


SHAPES = [dict(n=0), dict(n=-1), dict(n=32768, kv=2), dict(n=1, kv=65536), dict(kv=0), dict(n_q=0), dict(n_q=-1), dict(n_q=17),
          dict(groups=1, n_q=65, cap=128), dict(groups=0), dict(groups=9, n_q=1), dict(D=96), dict(D=0), dict(D=256), dict(T=-64), dict(T=96),
          dict(T=800), dict(cap=1), dict(cap=1025), dict(cap=0)]


@pytest.mark.parametrize("bad", SHAPES, ids=[",".join(f"{k}{v}" for k, v in b.items()) for b in SHAPES])
def test_decode_refuses_unsupported_shapes_and_they_need_no_workspace(bad):
    err, ws = _decode(_lib(), **bad)
    assert err == 1 and ws == 0


ARGS = [dict(kn=None), dict(vn=None),                        # exactly one of k_new / v_new NULL
        dict(table=None), dict(table=ONE + 4),               # 8-byte alignment of the table
        dict(q=None), dict(q=ONE + 8), dict(out=None), dict(out=ONE + 8), dict(ws=None), dict(ws=ONE + 8), dict(lse=None), dict(lse=ONE + 2),
        dict(kn=ONE + 8), dict(vn=ONE + 8), dict(sqrt_d=0.0)]


@pytest.mark.parametrize("bad", ARGS, ids=[",".join(f"{k}{v}" for k, v in b.items()) for b in ARGS])
def test_decode_refuses_bad_arguments_before_any_launch(bad):
    err, ws = _decode(_lib(), **bad)
    assert err == 1 and ws > 0   # (the shape itself is served)


def test_decode_takes_the_bounds_of_its_shape():
    """The shapes at the edge of what the list above refuses are validated through: they fail on the one bad pointer alone."""
    L = _lib()
    for ok in (dict(n=32767, kv=2), dict(groups=8, n_q=8), dict(groups=1, n_q=64, cap=64), dict(T=0), dict(cap=2), dict(cap=1024),
               dict(kn=None, vn=None)):
        assert _decode(L, **ok)[1] > 0 and _decode(L, q=None, **ok)[0] == 1


# ---- mustafar_ragged_set_sequences ---------------------------------------------------------------------------------------------------------
def _item(**kw):
    from mustafar_amd import _lib as lib
    a = dict(k=VIEW, v=VIEW, kt=ONE, vt=ONE, kw_=ONE, vw=ONE, T_base=256, T=768, w_len=5, cap=288)
    a.update(kw)
    return lib.Sequence(lib.CacheView(*a["k"]), lib.CacheView(*a["v"]), a["kt"], a["vt"], a["kw_"], a["vw"], a["T_base"], a["T"], a["w_len"], a["cap"])


def _set(L, items, table=ONE, first=0, n=None, kv=2, n_q=2, D=64, null_items=False):
    from mustafar_amd import _lib as lib
    arr = (lib.Sequence * max(len(items), 1))(*items)
    return L.mustafar_ragged_set_sequences(None, table, first, len(items) if n is None else n, None if null_items else arr, kv, n_q, D)


CALLS = [dict(n=0), dict(n=-1), dict(first=-1), dict(table=None), dict(table=ONE + 4), dict(kv=0), dict(kv=65536), dict(D=96), dict(D=0),
         dict(n_q=0), dict(n_q=-2), dict(null_items=True)]


@pytest.mark.parametrize("bad", CALLS, ids=[",".join(f"{k}{v}" for k, v in b.items()) for b in CALLS])
def test_set_sequences_refuses_bad_calls_before_any_launch(bad):
    """(The items are valid, and empty slots at that: only the argument under test is wrong.)"""
    assert _set(_lib(), [_item(w_len=0)], **bad) == 1


ITEMS = [dict(T=96, T_base=96), dict(T=-64, T_base=0), dict(T=256, T_base=0),          # T % 64; T < 0; T > 0 needs T_base > 0
         dict(T_base=-256), dict(T_base=1024), dict(T_base=32, T=64),                  # T_base outside [0, T], T_base % 64
         dict(T_base=64), dict(T_base=128, T=384),                                     # T_base % 256 with extents behind it
         dict(T=576), dict(T=256 + 256 * 513),                                         # (T - T_base) % 256; more than 512 entries
         dict(kt=None), dict(vt=None),                                                 # tables NULL with T > T_base
         dict(k=(None,) + VIEW[1:]), dict(v=(ONE, None) + VIEW[2:]), dict(k=(ONE, ONE, None) + VIEW[3:]),   # a base view with a NULL array
         dict(v=(ONE, ONE + 8) + VIEW[2:]),                                            # a misaligned stream
         dict(k=VIEW[:3] + (None, 0, 0, 0)),                                           # neither nz_offset nor a stream stride
         dict(k=VIEW[:4] + (100, 0, 0)), dict(v=VIEW[:4] + (0, 100, 0)),               # rows shorter than the tokens
         dict(k=VIEW + (1,)), dict(v=VIEW + (2,)),                                     # flags != 0: not tiles
         dict(kw_=None), dict(vw=None), dict(kw_=ONE + 8), dict(vw=ONE + 8),           # windows NULL / misaligned
         dict(w_len=1), dict(w_len=-3), dict(w_len=289), dict(cap=1025, w_len=5), dict(cap=1)]   # n_q <= window_len <= capacity <= 1024


@pytest.mark.parametrize("bad", ITEMS, ids=[",".join(f"{k}{v}" for k, v in b.items()) for b in ITEMS])
def test_set_sequences_refuses_a_bad_item_wherever_it_stands(bad):
    """Every item is validated before the first launch: a bad item behind valid (empty) ones, and behind a launch's worth of them,
    refuses the whole call.  The same item with nothing wrong passes validation -- shown by the call failing on the table alone."""
    L = _lib()
    empty = _item(w_len=0)
    assert _set(L, [_item(**bad)]) == 1
    assert _set(L, [empty, _item(**bad)]) == 1
    assert _set(L, [empty] * 17 + [_item(**bad)]) == 1


def test_an_empty_slot_is_not_looked_at():
    """window_len == 0: every other field may hold anything.  (A valid call would launch: the table is what is wrong here, and a call
    with a valid table is left to the GPU tests.)"""
    from mustafar_amd import _lib as lib
    L = _lib()
    junk = lib.Sequence(lib.CacheView(), lib.CacheView(3, 5, 7, 9, -1, -1, -1, 9), 1, 3, 5, 7, -64, 97, 0, -5)
    assert _set(L, [junk], table=None) == 1 and _set(L, [junk, _item(w_len=1)]) == 1


# ---- the Python refusals: before any device work --------------------------------------------------------------------------------------------
def _hook(Hq=8, Hkv=2, **kw):
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    kw.setdefault("api", "fused")
    return MustafarAttention(MustafarConfig(num_attention_heads=Hq, num_key_value_heads=Hkv, **kw))


def _qkv(n, Hq, Hkv, n_q, D=128):
    return (torch.zeros((n, Hq, n_q, D), dtype=torch.float16), torch.zeros((n, Hkv, n_q, D), dtype=torch.float16),
            torch.zeros((n, Hkv, n_q, D), dtype=torch.float16))


def _past(L, bsz=1, Hkv=2, D=128, C=0):
    w = torch.zeros((bsz, Hkv, L - C, D), dtype=torch.float16)
    return (None, w, None, w.clone(), C, L)


def test_decode_ragged_refuses_before_any_device_work():
    attn = _hook()
    q, k, v = _qkv(2, 8, 2, 2)
    pasts = [_past(40), _past(50)]
    with pytest.raises(ValueError, match="api='fused'"):
        _hook(api="reference").decode_ragged(q, k, v, pasts)
    with pytest.raises(ValueError, match="one bsz-1 past per sequence"):
        attn.decode_ragged(q, k, v, pasts[:1])
    with pytest.raises(ValueError, match="sequence 1 is not a bsz-1 past"):
        attn.decode_ragged(q, k, v, [_past(40), _past(50, bsz=2)])
    with pytest.raises(ValueError, match=r"q \[bsz, 8, n_q, 128\]"):
        attn.decode_ragged(q[:, :4], k, v, pasts)
    with pytest.raises(ValueError, match=r"q \[bsz, 8, n_q, 128\]"):
        attn.decode_ragged(q, k[:, :, :1], v, pasts)
    q17, k17, v17 = _qkv(2, 8, 2, 17)
    with pytest.raises(ValueError, match="one library call: at most 16 tokens"):
        attn.decode_ragged(q17, k17, v17, pasts)
    with pytest.raises(ValueError, match="serves 1 to 8 q heads"):
        _hook(Hq=32, Hkv=2).decode_ragged(*_qkv(2, 32, 2, 1), pasts)


def test_decode_ragged_names_the_sequence_that_would_step_over_its_trigger():
    """541 rows with nothing compressed reach the trigger point of 288 + 256 rows with their third new row: four tokens do not fit."""
    from mustafar_amd.ragged import RaggedBatch
    attn = _hook()
    q, k, v = _qkv(3, 8, 2, 4)
    pasts = [_past(100), _past(541, C=256), _past(830, C=768)]
    assert [attn.fits_before_trigger(p, 4) for p in pasts] == [4, 3, 4]
    with pytest.raises(ValueError, match=r"sequence 1\b.*at most 3\b"):
        attn.decode_ragged(q, k, v, pasts)
    with pytest.raises(ValueError, match=r"sequence 1\b.*at most 3\b"):
        RaggedBatch(attn, 4).decode(q, k, v, pasts)
    assert all(p[1].shape[2] == L - C for p, (L, C) in zip(pasts, ((100, 0), (541, 256), (830, 768))))


def test_a_ragged_batch_has_a_capacity():
    from mustafar_amd.ragged import RaggedBatch
    attn = _hook()
    for bad in (0, -1, 32768, 2.5):
        with pytest.raises(ValueError, match="capacity"):
            RaggedBatch(attn, bad)
    with pytest.raises(ValueError, match="api='fused'"):
        RaggedBatch(_hook(api="reference"), 4)
    with pytest.raises(ValueError, match="1 to 2 sequences"):
        RaggedBatch(attn, 2).decode(*_qkv(3, 8, 2, 1), [_past(40)] * 3)
