"""CPU: the shared-segment surface (ABI 111) checked without a GPU -- every C call here fails validation before any launch -- the run-length
rule read off the public workspace size, the Python refusals, and the needle constants the exact GPU tests of
tests/test_gpu_shared_segment.py rest on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import shared_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mustafar_shared_segment_workspace_bytes", "mustafar_decode_shared_segment")
ONE = 16   # a pointer that is never dereferenced (16-byte aligned, so that only the argument under test is wrong)


def _lib():
    from mustafar_amd import _lib as lib
    return lib.load()


def test_abi_111_declares_binds_and_exports_the_new_symbols():
    from mustafar_amd import _lib as lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mustafar_hip.h")).read(), flags=re.S)
    syms = set(re.findall(r"^\s*(?:int|int64_t)\s+(\w+)\s*\(", text, flags=re.M))
    raw = ctypes.CDLL(lib.LIB_PATH)
    for s in NEW:
        assert s in syms and s in lib.SIGNATURES and hasattr(raw, s), s
    assert _lib().mustafar_abi_version() >= 111


def _call(L, **kw):
    from mustafar_amd import _lib as lib
    a = dict(T=128, kvh=2, groups=4, n=2, q=ONE, out=ONE, lse=ONE, ws=ONE, sqrt_d=8.0, D=64, k=(ONE, ONE, ONE, ONE, 0, 0, 0),
             v=(ONE, ONE, ONE, ONE, 0, 0, 0), k_null=False, v_null=False)
    a.update(kw)
    kv, vv = lib.CacheView(*a["k"]), lib.CacheView(*a["v"])
    err = L.mustafar_decode_shared_segment(None, None if a["k_null"] else ctypes.byref(kv), None if a["v_null"] else ctypes.byref(vv), a["T"],
                                           a["kvh"], a["groups"], a["n"], a["q"], a["out"], a["lse"], a["ws"], ctypes.c_float(a["sqrt_d"]),
                                           a["D"])
    return err, L.mustafar_shared_segment_workspace_bytes(a["T"], a["kvh"], a["groups"], a["n"], a["D"])


SHAPES = [dict(T=0), dict(T=-64), dict(T=96), dict(n=0), dict(n=17), dict(groups=1, n=65), dict(groups=0), dict(groups=9, n=1), dict(D=96),
          dict(D=0), dict(D=256), dict(kvh=0)]


@pytest.mark.parametrize("bad", SHAPES, ids=[",".join(f"{k}{v}" for k, v in b.items()) for b in SHAPES])
def test_unsupported_shapes_are_refused_and_need_no_workspace(bad):
    err, ws = _call(_lib(), **bad)
    assert err == 1 and ws == 0


POINTERS = [dict(q=None), dict(out=None), dict(lse=None), dict(ws=None), dict(q=ONE + 8), dict(out=ONE + 2), dict(lse=ONE + 2), dict(ws=ONE + 4),
            dict(k_null=True), dict(v_null=True), dict(k=(None, ONE, ONE, ONE, 0, 0, 0)), dict(v=(ONE, None, ONE, ONE, 0, 0, 0)),
            dict(k=(ONE, ONE, None, ONE, 0, 0, 0)), dict(v=(ONE, ONE + 8, ONE, ONE, 0, 0, 0)),
            dict(k=(ONE, ONE, ONE, None, 0, 0, 0)),           # no nz_offset and no stream stride
            dict(k=(ONE, ONE, ONE, ONE, 127, 0, 0)),          # bitmap rows shorter than the tokens (128 tiles at D = 64)
            dict(v=(ONE, ONE, ONE, ONE, 0, 128, 0)),          # offset rows shorter than the tokens + 1
            dict(v=(ONE, ONE, ONE, ONE, 0, 0, -1)), dict(sqrt_d=0.0)]


@pytest.mark.parametrize("bad", POINTERS, ids=[str(i) for i in range(len(POINTERS))])
def test_null_and_misaligned_pointers_are_refused_before_any_launch(bad):
    err, _ = _call(_lib(), **bad)
    assert err == 1


@pytest.mark.parametrize("Dd", [64, 128])
def test_workspace_is_a_whole_slab_count_and_follows_the_run_length_rule(Dd):
    """slabs x kv heads x R x (D + 2) floats; a run holds ceil(8 R (D + 2) / (88 D)) blocks: the slab bytes written and read, 8 R (D + 2)
    per run, stay at or below the run's nominal stream bytes, 88 D per block."""
    L = _lib()
    for n, groups in [(1, 1), (1, 4), (3, 3), (5, 4), (8, 4), (16, 4), (8, 8), (64, 1)]:
        R = n * groups
        want = -(-8 * R * (Dd + 2) // (88 * Dd))
        assert 2 * R * (Dd + 2) * 4 <= want * 88 * Dd and (want == 1 or 2 * R * (Dd + 2) * 4 > (want - 1) * 88 * Dd)
        for T in (64, 128, 576, 7936, 32512):
            slabs, bpw, last = su.run_shape(L, T, 2, groups, n, Dd)
            assert slabs == -(-(T // 64) // want) and 1 <= last <= bpw <= want
    assert su.run_shape(L, 32512, 1, 1, 64, Dd)[1] == 6 and su.run_shape(L, 32512, 1, 4, 8, Dd)[1] == 3
    assert su.run_shape(L, 32512, 1, 4, 1, Dd)[1] == 1


def _fake_cache(heads, tokens, Dd):
    tiles = tokens * Dd // 64
    return [torch.zeros(heads * tiles, dtype=torch.int64), torch.zeros(heads * (tiles + 1), dtype=torch.int32),
            [torch.zeros(8, dtype=torch.float16) for _ in range(heads)], torch.zeros(heads, dtype=torch.int32)]


def _hook(Dd, Hq, Hkv, **kw):
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    return MustafarAttention(MustafarConfig(num_attention_heads=Hq, num_key_value_heads=Hkv, head_dim=Dd, api="fused", **kw))


def test_shared_segment_refuses_the_wrong_number_of_heads():
    from mustafar_amd import partial
    seg = partial.SharedSegment(_fake_cache(2, 128, 64), _fake_cache(2, 128, 64), 128, kv_heads=2)
    assert seg.kv_heads == 2 and seg.tokens == 128
    with pytest.raises(ValueError, match="heads"):
        partial.SharedSegment(_fake_cache(2, 128, 64), _fake_cache(4, 128, 64), 128)
    with pytest.raises(ValueError, match="heads"):
        partial.SharedSegment(_fake_cache(4, 128, 64), _fake_cache(4, 128, 64), 128, kv_heads=2)   # batch x kv heads: not ONE copy
    with pytest.raises(ValueError, match="multiple of 64"):
        partial.SharedSegment(_fake_cache(2, 96, 64), _fake_cache(2, 96, 64), 96)
    with pytest.raises(ValueError, match="consolidate"):
        partial.SharedSegment(object(), object(), 128)
    # a segment of 4 heads against an attention of 2 kv heads: refused before any launch
    q = torch.zeros((2, 8, 1, 64), dtype=torch.float16)
    with pytest.raises(ValueError, match="heads"):
        partial.decode_segment(_hook(64, 8, 2), q, partial.SharedSegment(_fake_cache(4, 128, 64), _fake_cache(4, 128, 64), 128))
    with pytest.raises(ValueError, match="mask"):
        partial.decode_segment(_hook(64, 8, 2), q, seg, attention_mask=torch.zeros((2, 1, 1, 128), dtype=torch.float16))
    # more than 8 q heads per kv head, and a query that is no fp16 tensor on the GPU: named, before any pointer is passed
    with pytest.raises(ValueError, match="1 to 8 q heads"):
        partial.decode_segment(_hook(64, 32, 2), torch.zeros((1, 32, 1, 64), dtype=torch.float16), seg)
    with pytest.raises(ValueError, match="float16 tensor on the GPU"):
        partial.decode_segment(_hook(64, 8, 2), q, seg)
    with pytest.raises(ValueError, match="float16 tensor on the GPU"):
        partial.decode_segment(_hook(64, 8, 2), q.float(), seg)


def test_a_list_of_per_head_streams_is_concatenated_once():
    from mustafar_amd import partial
    seg = partial.SharedSegment(_fake_cache(2, 128, 64), _fake_cache(2, 128, 64), 128)
    flat = seg._k.flat
    assert flat.numel() == 16 and seg.bytes_in_use() == 2 * (2 * 128 * 8 + 2 * 129 * 4 + 2 * 4 + 16 * 2)
    seg.view_ptrs()
    assert seg._k.flat is flat


def test_decode_split_refuses_a_mask_together_with_a_shared_entry():
    from mustafar_amd import partial
    attn = _hook(64, 8, 2)
    seg = partial.SharedSegment(_fake_cache(2, 128, 64), _fake_cache(2, 128, 64), 128)
    q = torch.zeros((2, 8, 1, 64), dtype=torch.float16)
    kv = torch.zeros((2, 2, 1, 64), dtype=torch.float16)
    past = (None, kv, None, kv, 0, 1)
    mask = torch.zeros((2, 1, 1, 128 + 2), dtype=torch.float16)
    with pytest.raises(ValueError, match="SharedSegment"):
        attn.decode_split(q, kv, kv, past, [seg], attention_mask=mask)
    with pytest.raises(ValueError, match="SharedSegment"):
        attn.decode_split(q, kv, kv, past, [(None, None, 64), seg], attention_mask=mask)


# ---- the claims behind the exact GPU tests -----------------------------------------------------------------------------------------------
TABLE = [(128, 4, 8, 16, 90.5, 5.66), (128, 16, 8, 16, 90.5, 5.66), (128, 32, 4, 16, 45.25, 2.83), (128, 64, 2, 32, 45.25, 1.41),
         (64, 8, 8, 16, 128.0, 8.0), (64, 32, 2, 32, 64.0, 2.0), (64, 64, 1, 64, 64.0, 1.0),
         (64, 9, 4, 16, 64.0, 4.0), (64, 16, 4, 16, 64.0, 4.0), (128, 9, 8, 16, 90.5, 5.66)]


@pytest.mark.parametrize("Dd,R,w,lv,x,other", TABLE)
def test_needle_constants(Dd, R, w, lv, x, other):
    """Slot width, level, the needle's x and the largest other x of every row count the GPU tests use; the gap is above the project's 39,
    so every other e is exactly 0 once stored as fp16 and every other slab's weight is absorbed in fp32."""
    f32, f16 = np.float32, np.float16
    assert su.slot_width(Dd, R) == w and su.level(w) == lv and R * w <= Dd
    assert su.needle_x(Dd, w) == x and abs(su.other_x_max(Dd, w) - other) < 0.01
    gap = su.needle_x(Dd, w) - su.other_x_max(Dd, w)
    assert gap > 39
    with np.errstate(under="ignore"):
        e = f32(np.exp(f32(-gap)))
    assert f16(e) == f16(0.0)
    lmax = f32(65536.0)
    assert f32(1.0) + e * lmax == f32(1.0) and f32(2.0 ** -5) + e * lmax * f32(2.0) == f32(2.0 ** -5) and f16(e * lmax * f32(2.0)) == f16(0.0)


@pytest.mark.parametrize("Dd,n,groups", [(64, 16, 4), (128, 8, 8), (64, 3, 3)])
def test_needle_builder_gives_every_row_a_slot_of_its_own(Dd, n, groups):
    Hkv, T = 2, 128
    rng = np.random.default_rng(Dd + n)
    pos = su.assign_rows(su.edge_positions(T), n, Hkv * groups, rng, T)[0]
    K, V, q, w = su.needle_data(Dd, n, groups, Hkv, T, pos, seed=1)
    Kp = torch.from_numpy(__import__("oracle.oracle", fromlist=["x"]).prune_magnitude(K.numpy(), 0.7))
    scores = torch.einsum("shd,ktd->shkt", q[:, :, 0].double(), Kp[0].double())
    rs = np.sqrt(Dd)
    for s in range(n):
        for h in range(Hkv * groups):
            row = scores[s, h, h // groups] / rs
            assert int(row.argmax()) == pos[s, h] and abs(float(row.max()) - su.needle_x(Dd, w)) < 0.01
            row[pos[s, h]] = -1e9
            assert float(row.max()) <= su.other_x_max(Dd, w) + 0.01
    want = su.needle_expect(V, pos, groups)
    assert want.shape == (n, Hkv * groups, 1, Dd)
