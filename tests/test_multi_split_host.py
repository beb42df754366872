"""CPU: several query tokens per call over frozen and shared segments (mustafar_decode_shared_segment_multi, mustafar_decode_multi_segment,
their workspace sizes; SharedSegment.decode_multi, decode_segment_multi, decode_multi_split) checked without a GPU -- every C call here
fails validation before any launch --, the workspace formulas, and the Python refusals on CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

from tests.test_multi_query_host import ONE, VIEW, _hook, _past, _qkv
from tests.test_shared_segment_host import _fake_cache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mustafar_shared_segment_multi_workspace_bytes", "mustafar_decode_shared_segment_multi",
       "mustafar_decode_multi_segment_workspace_bytes", "mustafar_decode_multi_segment")


def _lib():
    from mustafar_amd import _lib as lib
    return lib.load()


def test_the_four_symbols_are_declared_bound_and_exported_at_abi_115():
    """The entry points came without a version change: a caller finds them by symbol."""
    from mustafar_amd import _lib as lib
    header = open(os.path.join(ROOT, "include", "mustafar_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    syms = set(re.findall(r"^\s*(?:int|int64_t)\s+(\w+)\s*\(", text, flags=re.M))
    raw = ctypes.CDLL(lib.LIB_PATH)
    for s in NEW:
        assert s in syms and s in lib.SIGNATURES and hasattr(raw, s), s
    assert _lib().mustafar_abi_version() == 115
    assert "stays 115" in header and "by symbol" in header


# ---- workspace formulas -------------------------------------------------------------------------------------------------------------------
def _bpw(R, Dd):
    return -(-8 * min(R, 64) * (Dd + 2) // (88 * Dd))


# (n_seqs, groups, n_q): R = 1, 8, 12, 15, 64, 65, 80, 84, 128, 1024
ROWS = [(1, 1, 1), (1, 4, 2), (2, 4, 3), (3, 1, 5), (2, 8, 4), (13, 1, 5), (5, 4, 4), (7, 4, 3), (2, 8, 8), (32, 8, 4), (1, 8, 128), (1024, 1, 1)]


@pytest.mark.parametrize("Dd", [64, 128])
def test_workspace_formulas(Dd):
    """ceil(T / 64 / run length) x heads x R x (D + 2) x 4, run length = blocks_per_run(min(R, 64), D); R = 1025 -> 0."""
    L = _lib()
    for n, groups, n_q in ROWS:
        R = n * groups * n_q
        for T in (64, 128, 576, 7936):
            slabs = -(-(T // 64) // _bpw(R, Dd))
            for heads in (1, 2, 3):
                assert L.mustafar_shared_segment_multi_workspace_bytes(T, heads, groups, n, n_q, Dd) == slabs * heads * R * (Dd + 2) * 4
            if R <= 64 and groups * n_q <= 8:   # the old call with groups * n_q in place of groups
                assert L.mustafar_shared_segment_multi_workspace_bytes(T, 2, groups, n, n_q, Dd) == \
                    L.mustafar_shared_segment_workspace_bytes(T, 2, groups * n_q, n, Dd)
    for groups, n_q in [(1, 1), (4, 2), (4, 12), (8, 8), (1, 65), (4, 20), (4, 64), (4, 256), (8, 128), (1, 1024)]:
        R = groups * n_q
        for T in (64, 192, 576, 7936):
            for Bp in (1, 4):
                want = -(-(T // 64) // _bpw(R, Dd)) * Bp * R * (Dd + 2) * 4
                assert L.mustafar_decode_multi_segment_workspace_bytes(T, Bp, groups, n_q, Dd) == want
    # R = 64, 65, 128, 1024 and 1025
    assert _bpw(64, Dd) == _bpw(65, Dd) == _bpw(1024, Dd) == 6
    for R in (64, 65, 128, 1024):
        assert L.mustafar_shared_segment_multi_workspace_bytes(768, 1, 1, R, 1, Dd) == 2 * R * (Dd + 2) * 4
        assert L.mustafar_decode_multi_segment_workspace_bytes(768, 1, 1, R, Dd) == 2 * R * (Dd + 2) * 4
    assert L.mustafar_shared_segment_multi_workspace_bytes(768, 1, 1, 1025, 1, Dd) == 0
    assert L.mustafar_shared_segment_multi_workspace_bytes(768, 1, 5, 41, 5, Dd) == 0      # 1025 rows
    assert L.mustafar_decode_multi_segment_workspace_bytes(768, 1, 1, 1025, Dd) == 0
    assert L.mustafar_decode_multi_segment_workspace_bytes(768, 1, 5, 205, Dd) == 0


# ---- the shared form: every argument, each with all others valid -------------------------------------------------------------------------
def _shared(L, **kw):
    from mustafar_amd import _lib as lib
    a = dict(T=128, kvh=2, groups=4, n=5, n_q=4, q=ONE, out=ONE, lse=ONE, ws=ONE, sqrt_d=8.0, D=64, k=VIEW, v=VIEW, k_null=False, v_null=False)
    a.update(kw)
    kv, vv = lib.CacheView(*a["k"]), lib.CacheView(*a["v"])
    err = L.mustafar_decode_shared_segment_multi(None, None if a["k_null"] else ctypes.byref(kv), None if a["v_null"] else ctypes.byref(vv),
                                                 a["T"], a["kvh"], a["groups"], a["n"], a["n_q"], a["q"], a["out"], a["lse"], a["ws"],
                                                 ctypes.c_float(a["sqrt_d"]), a["D"])
    return err, L.mustafar_shared_segment_multi_workspace_bytes(a["T"], a["kvh"], a["groups"], a["n"], a["n_q"], a["D"])


SHARED_SHAPES = [dict(T=0), dict(T=65), dict(T=-64), dict(groups=0), dict(groups=9), dict(n_q=0), dict(n_q=-1), dict(n=0),
                 dict(n=41, groups=5, n_q=5), dict(n=1025, groups=1, n_q=1), dict(n=1, groups=1, n_q=1025), dict(n=1 << 20, n_q=1 << 20),
                 dict(D=96), dict(D=0), dict(kvh=0), dict(kvh=65536)]


@pytest.mark.parametrize("bad", SHARED_SHAPES, ids=[",".join(f"{k}{v}" for k, v in b.items()) for b in SHARED_SHAPES])
def test_shared_form_refuses_unsupported_shapes_and_they_need_no_workspace(bad):
    err, ws = _shared(_lib(), **bad)
    assert err == 1 and ws == 0


VIEWS = [dict(k_null=True), dict(v_null=True), dict(k=(None, ONE, ONE, ONE, 0, 0, 0)), dict(v=(ONE, None, ONE, ONE, 0, 0, 0)),
         dict(k=(ONE, ONE, None, ONE, 0, 0, 0)), dict(v=(ONE, ONE + 8, ONE, ONE, 0, 0, 0)),
         dict(k=(ONE, ONE, ONE, None, 0, 0, 0)),            # no nz_offset and no stream stride
         dict(v=(ONE, ONE, ONE, ONE, 0, 0, -1)),
         dict(k=(ONE, ONE, ONE, ONE, 0, 0, 0, 1))]          # flags: token rows, not tiles
POINTERS = [dict(q=None), dict(out=None), dict(lse=None), dict(ws=None), dict(q=ONE + 8), dict(out=ONE + 2), dict(lse=ONE + 2), dict(ws=ONE + 4),
            dict(sqrt_d=0.0)]
SHARED_ARGS = POINTERS + VIEWS + [dict(k=(ONE, ONE, ONE, ONE, 127, 0, 0)),          # bitmap rows shorter than the tokens (128 tiles at D = 64)
                                  dict(v=(ONE, ONE, ONE, ONE, 0, 128, 0))]          # offset rows shorter than the tokens + 1


@pytest.mark.parametrize("bad", SHARED_ARGS, ids=[str(i) for i in range(len(SHARED_ARGS))])
def test_shared_form_refuses_bad_pointers_and_views_before_any_launch(bad):
    err, ws = _shared(_lib(), **bad)
    assert err == 1 and ws > 0


# ---- the per-sequence form ------------------------------------------------------------------------------------------------------------------
# T = 512 columns; Bp = 4 heads in two planes, n_q = 5 at GQA-4
GOOD_MASK = dict(mask=ONE + 2, mbs=512, mrs=512, mrows=5, hpm=2)


def _seg(L, **kw):
    from mustafar_amd import _lib as lib
    a = dict(T=512, T_base=256, Bp=4, groups=4, n_q=5, q=ONE, out=ONE, lse=ONE, ws=ONE, sqrt_d=8.0, D=64, k=VIEW, v=VIEW, k_null=False,
             v_null=False, kt=ONE, vt=ONE, mask=None, mbs=0, mrs=0, mrows=1, hpm=1)
    a.update(kw)
    kv, vv = lib.CacheView(*a["k"]), lib.CacheView(*a["v"])
    err = L.mustafar_decode_multi_segment(None, None if a["k_null"] else ctypes.byref(kv), None if a["v_null"] else ctypes.byref(vv), a["T_base"],
                                          a["kt"], a["vt"], a["T"], a["Bp"], a["groups"], a["n_q"], a["q"], a["out"], a["lse"], a["ws"],
                                          ctypes.c_float(a["sqrt_d"]), a["D"], a["mask"], a["mbs"], a["mrs"], a["mrows"], a["hpm"])
    return err, L.mustafar_decode_multi_segment_workspace_bytes(a["T"], a["Bp"], a["groups"], a["n_q"], a["D"])


SEG_SHAPES = [dict(T=0, T_base=0), dict(T=65, T_base=65), dict(T=-64, T_base=0), dict(groups=0), dict(groups=9), dict(n_q=0), dict(n_q=-1),
              dict(n_q=257), dict(groups=1, n_q=1025), dict(groups=5, n_q=205), dict(D=96), dict(D=0), dict(Bp=0), dict(Bp=65536)]


@pytest.mark.parametrize("bad", SEG_SHAPES, ids=[",".join(f"{k}{v}" for k, v in b.items()) for b in SEG_SHAPES])
def test_per_sequence_form_refuses_unsupported_shapes_and_they_need_no_workspace(bad):
    err, ws = _seg(_lib(), **bad)
    assert err == 1 and ws == 0
    assert _seg(_lib(), **GOOD_MASK, **bad)[0] == 1


EXTENT_RULES = [dict(T_base=64), dict(T_base=128, T=384),          # T_base % 256 with extents behind it
                dict(T=576, T_base=256),                           # (T - T_base) % 256 (T % 64 == 0)
                dict(T_base=256, T=256 + 256 * 513),               # more than 512 entries
                dict(kt=None), dict(vt=None),                      # tables NULL with T > T_base
                dict(T_base=0), dict(T_base=768), dict(T_base=-256), dict(T_base=96, T=96)]
SEG_ARGS = POINTERS + VIEWS + EXTENT_RULES + [dict(k=(ONE, ONE, ONE, ONE, 255, 0, 0)),     # bitmap rows shorter than the base's tokens
                                              dict(v=(ONE, ONE, ONE, ONE, 0, 256, 0))]     # offset rows shorter than the tokens + 1


@pytest.mark.parametrize("bad", SEG_ARGS, ids=[str(i) for i in range(len(SEG_ARGS))])
def test_per_sequence_form_refuses_bad_arguments_before_any_launch(bad):
    """Without a mask, with a NULL mask and nonsense in the other four mask arguments, and with a valid mask."""
    L = _lib()
    assert _seg(L, **bad)[0] == 1
    assert _seg(L, mask=None, mbs=-5, mrs=-5, mrows=77, hpm=0, **bad)[0] == 1
    assert _seg(L, **GOOD_MASK, **bad)[0] == 1


MASK_ARGS = [dict(mask=ONE + 1), dict(mask=ONE + 3),                       # an odd address
             dict(mrows=0), dict(mrows=3), dict(mrows=-1), dict(mrows=4),  # neither 1 nor n_q
             dict(hpm=0), dict(hpm=-1), dict(hpm=3), dict(hpm=8), dict(Bp=6, hpm=4),   # out of range, no divisor of Bp
             dict(mrs=511), dict(mrs=0),                                   # rows closer than T with mask_rows > 1
             dict(mbs=511), dict(mbs=0),                                   # planes closer than T with more than one plane
             dict(mbs=-1, hpm=4), dict(mrs=-1, mrows=1)]                   # a negative stride, even where the stride is not used


@pytest.mark.parametrize("bad", MASK_ARGS, ids=[",".join(f"{k}{v}" for k, v in b.items()) for b in MASK_ARGS])
def test_per_sequence_form_checks_the_mask_with_T_columns(bad):
    a = dict(GOOD_MASK)
    a.update(bad)
    assert _seg(_lib(), **a)[0] == 1


# ---- Python refusals, on CPU tensors ------------------------------------------------------------------------------------------------------
def _shared_seg(heads=2, tokens=128, Dd=64):
    from mustafar_amd import partial
    return partial.SharedSegment(_fake_cache(heads, tokens, Dd), _fake_cache(heads, tokens, Dd), tokens)


def test_the_segment_calls_need_the_fused_api():
    from mustafar_amd import partial
    attn = _hook(128, 8, 2, api="native")
    q, k, v = _qkv(attn, 3)
    seg = _shared_seg(Dd=128)
    with pytest.raises(ValueError, match="fused"):
        seg.decode_multi(attn, q)
    with pytest.raises(ValueError, match="fused"):
        partial.decode_segment_multi(attn, q, seg)
    with pytest.raises(ValueError, match="fused"):
        attn.decode_segment_multi(q, _fake_cache(2, 128, 128), _fake_cache(2, 128, 128), 128)
    with pytest.raises(ValueError, match="decode_multi_split needs"):
        attn.decode_multi_split(q, k, v, _past(attn, 40), [seg])


@pytest.mark.parametrize("shape", [(2, 8, 3), (2, 4, 3, 64), (2, 8, 3, 128), (2, 8, 0, 64)])
def test_the_segment_calls_refuse_a_query_of_the_wrong_shape(shape):
    from mustafar_amd import partial
    attn = _hook(64, 8, 2)
    q = torch.zeros(shape, dtype=torch.float16)
    seg = _shared_seg()
    with pytest.raises(ValueError, match="decode_segment_multi: query of shape"):
        seg.decode_multi(attn, q)
    with pytest.raises(ValueError, match="decode_segment_multi: query of shape"):
        partial.decode_segment_multi(attn, q, seg)
    with pytest.raises(ValueError, match="decode_segment_multi: query of shape"):
        attn.decode_segment_multi(q, _fake_cache(4, 128, 64), _fake_cache(4, 128, 64), 128)


def test_decode_segment_multi_refusals():
    from mustafar_amd import partial
    attn = _hook(64, 8, 2)
    q = torch.zeros((2, 8, 3, 64), dtype=torch.float16)
    seg = _shared_seg()
    with pytest.raises(ValueError, match="no attention mask"):
        partial.decode_segment_multi(attn, q, seg, attention_mask=torch.zeros((2, 1, 3, 128), dtype=torch.float16))
    with pytest.raises(ValueError, match="carries both caches"):
        partial.decode_segment_multi(attn, q, seg, tokens=128)
    with pytest.raises(ValueError, match="heads"):
        partial.decode_segment_multi(attn, q, _shared_seg(heads=4))
    with pytest.raises(ValueError, match="1 to 8 q heads"):
        partial.decode_segment_multi(_hook(64, 32, 2), torch.zeros((1, 32, 2, 64), dtype=torch.float16), seg)
    with pytest.raises(ValueError, match="float16 tensor on the GPU"):
        seg.decode_multi(attn, q)                          # a CPU tensor: named before any pointer is passed
    with pytest.raises(ValueError, match="at most 256 tokens"):
        seg.decode_multi(attn, torch.zeros((1, 8, 257, 64), dtype=torch.float16))
    # per-sequence segments
    kc, vc = _fake_cache(4, 128, 64), _fake_cache(4, 128, 64)
    with pytest.raises(ValueError, match=r"\(k_cache, v_cache, tokens\)"):
        partial.decode_segment_multi(attn, q, kc)
    with pytest.raises(ValueError, match="multiple of 64"):
        partial.decode_segment_multi(attn, q, kc, vc, 96)
    with pytest.raises(ValueError, match="at most 256 tokens"):
        partial.decode_segment_multi(attn, torch.zeros((2, 8, 257, 64), dtype=torch.float16), kc, vc, 128)
    for shape in [(2, 1, 3, 127), (2, 1, 2, 128), (1, 1, 3, 128), (2, 2, 3, 128), (2, 3, 128)]:
        with pytest.raises(ValueError, match="Attention mask should be of size"):
            partial.decode_segment_multi(attn, q, kc, vc, 128, attention_mask=torch.zeros(shape, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="float16"):
        partial.decode_segment_multi(attn, q, kc, vc, 128, attention_mask=torch.zeros((2, 1, 3, 128)))
    with pytest.raises(ValueError, match="float16 tensor on the GPU"):
        partial.decode_segment_multi(attn, q, kc, vc, 128, attention_mask=torch.zeros((2, 1, 1, 130), dtype=torch.float16))


def test_decode_multi_split_refuses_mismatched_shapes():
    attn = _hook(64, 8, 2)
    q, k, v = _qkv(attn, 3)
    with pytest.raises(ValueError, match="decode_multi_split: q"):
        attn.decode_multi_split(q, k[:, :, :2], v, _past(attn, 40), [_shared_seg()])
    with pytest.raises(ValueError, match="decode_multi_split: q"):
        attn.decode_multi_split(q[:, :4], k, v, _past(attn, 40), [_shared_seg()])
    with pytest.raises(ValueError, match="1 to 8 q heads"):
        big = _hook(64, 32, 2)
        big.decode_multi_split(*_qkv(big, 2), _past(big, 40), [_shared_seg()])


@pytest.mark.parametrize("shape", [(1, 1, 3, 170), (1, 1, 3, 172), (1, 1, 1, 43), (1, 1, 3, 43), (1, 1, 2, 171), (1, 2, 3, 171), (2, 1, 3, 171),
                                   (1, 3, 171)])
def test_decode_multi_split_refuses_a_mask_of_the_wrong_width(shape):
    """A shared entry of 128 tokens (its columns are in the mask, though never read), kv_seq_len 40, n_q 3: [1, 1, 1 or 3, 171]."""
    attn = _hook(64, 8, 2)
    with pytest.raises(ValueError, match=r"Attention mask should be of size \(1, 1, 3, 171\)"):
        attn.decode_multi_split(*_qkv(attn, 3), _past(attn, 40), [_shared_seg()], attention_mask=torch.zeros(shape, dtype=torch.float16))
    with pytest.raises(ValueError, match=r"Attention mask should be of size \(1, 1, 3, 235\)"):   # + a per-sequence entry of 64
        attn.decode_multi_split(*_qkv(attn, 3), _past(attn, 40), [_shared_seg(), (None, None, 64)],
                                attention_mask=torch.zeros((1, 1, 3, 171), dtype=torch.float16))


@pytest.mark.parametrize("w,n_q,fits", [(284, 6, 4), (287, 2, 1), (280, 16, 8), (286, 3, 2)])
def test_decode_multi_split_refuses_a_call_that_steps_over_a_trigger_point(w, n_q, fits):
    """The rule of decode_multi, checked before any frozen entry is read: the message names the largest n_q that fits."""
    attn = _hook(64, 8, 2)
    with pytest.raises(ValueError, match=f"decode_multi_split: {n_q} tokens would step over .* at most {fits} fit"):
        attn.decode_multi_split(*_qkv(attn, n_q), _past(attn, w), [_shared_seg()])
    assert attn.fits_before_trigger(_past(attn, w), fits) == fits


def test_the_single_token_methods_keep_their_refusals():
    """decode_split still refuses a mask next to a shared entry, decode_segment and SharedSegment.decode still refuse q_len != 1."""
    from mustafar_amd import partial
    attn = _hook(64, 8, 2)
    seg = _shared_seg()
    q3 = torch.zeros((2, 8, 3, 64), dtype=torch.float16)
    with pytest.raises(ValueError, match="decode_segment: query of shape"):
        seg.decode(attn, q3)
    with pytest.raises(ValueError, match="decode_segment: query of shape"):
        partial.decode_segment(attn, q3, seg)
    kv = torch.zeros((2, 2, 1, 64), dtype=torch.float16)
    with pytest.raises(ValueError, match="SharedSegment"):
        attn.decode_split(q3[:, :, :1], kv, kv, (None, kv, None, kv, 0, 1), [seg], attention_mask=torch.zeros((2, 1, 1, 130), dtype=torch.float16))
