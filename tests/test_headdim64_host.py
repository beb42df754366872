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


# ---- the run shapes the multi-block GPU tests rely on (tests/test_gpu_headdim64_runs.py) -------------------------------------------
def _formula(ntb, Bp):
    """about 4096 one-wave workgroups over all kv heads, at most 1008 compressed slabs per row."""
    bpw = max(1, (ntb * Bp + 2048) // 4096)
    while -(-ntb // bpw) > 1008:
        bpw += 1
    return bpw


def test_run_shape_table():
    from mustafar_amd import _lib
    from tests.hd64_util import RUN_SHAPES, run_shape
    L = _lib.load()
    for name, (Bp, T, bpw, S1, last) in RUN_SHAPES.items():
        ntb = T // 64
        assert _formula(ntb, Bp) == bpw and -(-ntb // bpw) == S1 and ntb - (S1 - 1) * bpw == last, name
        for g in range(1, 9):   # the shape depends on B', not on the group count
            assert run_shape(L, T, Bp * g, g) == (S1, bpw), (name, g)
    assert {v[2] for v in RUN_SHAPES.values()} >= {1, 2, 3, 8}
    assert any(v[4] < v[2] for v in RUN_SHAPES.values()), "no short last run in the table"
    # the first D = 64 module's shapes all get one block per workgroup: the gap the runs module closes
    for Bp, T in [(4, 4096), (6, 640), (2, 32768), (4, 1024), (4, 512), (8, 28 * 64)]:
        assert run_shape(L, T, Bp * 4, 4) == (T // 64, 1)
    assert run_shape(L, 0, 8, 4) == (0, 1)


# ---- the D = 64 needle generator and the model's mask, checked on the CPU ----------------------------------------------------------
@pytest.mark.parametrize("ks,vs", [(0.0, 0.0), (0.3, 0.3), (0.5, 0.8), (0.7, 0.7), (0.9, 0.0), (0.99, 0.99)])
@pytest.mark.parametrize("k", [1, 2, 4])
def test_needles_64_survive_the_prune_and_decide_the_output(ks, vs, k):
    import math
    import numpy as np
    import torch
    from oracle import dense_ref
    from oracle import oracle as orc
    from tests.hd64_util import D, needle_data_64, needle_expect_64
    B, Hq, Hkv, n, C = 2, 16, 2, 3000, 2944       # 8 heads per kv head: every slot in use
    rng = np.random.default_rng(k)
    pos = np.stack([rng.choice(n, k, replace=False) for _ in range(B * Hq)]).reshape(B, Hq, k)
    pos[0, 0, 0], pos[0, 1, 0], pos[1, 0, 0] = 0, n - 1, C - 1
    pos = np.stack([p if len(set(p)) == k else np.arange(k) + 7 for p in pos.reshape(-1, k)]).reshape(B, Hq, k)
    K, V, q = needle_data_64(B, Hq, Hkv, n, pos, seed=k, device="cpu")
    Kp, Vp = K.clone(), V.clone()
    Kp[:, :, :C] = torch.from_numpy(orc.prune_magnitude(K[:, :, :C].numpy(), ks))
    Vp[:, :, :C] = torch.from_numpy(orc.prune_magnitude(V[:, :, :C].numpy(), vs))
    g = Hq // Hkv
    x = torch.einsum("bkgd,bktd->bkgt", q.double().view(B, Hkv, g, D), Kp.double()).reshape(B, Hq, n) / math.sqrt(D)
    top = x.topk(k + 1, -1).values
    assert (top[..., :k] == 128).all(), "a needle's slot does not survive the prune"
    assert (top[..., k] <= 8).all(), "a non-needle token scores above 8"
    assert np.exp(np.float32(8 - 128)) == 0 and np.float16(np.exp(np.float32(8 - 128))) == 0   # every other weight: 0 in fp32 and fp16
    want = needle_expect_64(V, pos, C, g, vs=vs)
    got = dense_ref.dense_decode_layer(q, Kp, Vp, g)
    assert torch.equal(got.double(), want.double())


def test_a_needle_64_moved_by_one_token_fails_the_checker():
    import numpy as np
    from tests.hd64_util import needle_data_64, needle_expect_64
    B, Hq, Hkv, n, C = 1, 8, 2, 400, 256
    pos = np.array([[0, 63, 64, 255, 256, 300, 398, 399]])
    K, V, q = needle_data_64(B, Hq, Hkv, n, pos, seed=7, device="cpu")
    want = needle_expect_64(V, pos, C, Hq // Hkv)
    for h, d in ((0, 1), (3, 1), (4, -1), (7, -1)):      # across block, compressed / window and new-row edges
        moved = pos.copy()
        moved[0, h] += d
        miss = (needle_expect_64(V, moved, C, Hq // Hkv).float() != want.float()).any(-1).reshape(-1)
        assert miss[h] and miss.sum() == 1
    # a secondary needle wins once the primary one is masked, and only then
    pos2 = np.array([[5, -1, -1, -1, 390, -1, -1, 2]])
    K, V, q = needle_data_64(B, Hq, Hkv, n, pos, seed=7, device="cpu", pos2=pos2)
    masked = np.zeros((B, Hq, n), bool)
    masked[0, 0, 0] = masked[0, 4, 256] = True
    alt = needle_expect_64(V, pos, C, Hq // Hkv, pos2=pos2, masked=masked)
    miss = (alt.float() != want.float()).any(-1).reshape(-1)
    assert miss.tolist() == [True, False, False, False, True, False, False, False]


@pytest.mark.parametrize("Dd", [64, 128])
def test_model_mask_is_the_hooks_mask(Dd):
    import math
    import torch
    from tests import exact_data as xd
    torch.manual_seed(Dd)
    B, Hq, Hkv, n = 2, 8, 2, 300
    K, V, q = torch.randn(B, Hkv, n, Dd).half(), torch.randn(B, Hkv, n, Dd).half(), torch.randn(B, Hq, 1, Dd).half()
    out0, bound0 = xd.hook_model(q, K, V, Hq // Hkv)
    zero = torch.zeros((B, 1, 1, n), dtype=torch.float16)
    out1, bound1 = xd.hook_model(q, K, V, Hq // Hkv, mask=zero)
    assert torch.equal(out0, out1) and torch.equal(bound0, bound1)
    # finfo.min on the first p columns == those columns dropped (their weight is exp(-65504 - m) = 0)
    p = 37
    pad = zero.clone()
    pad[..., :p] = torch.finfo(torch.float16).min
    out2, bound2 = xd.hook_model(q, K, V, Hq // Hkv, mask=pad)
    out3, bound3 = xd.hook_model(q, K[:, :, p:], V[:, :, p:], Hq // Hkv)
    assert float((out2 - out3).abs().max()) <= 1e-13 and float((bound2 - bound3).abs().max()) <= 2.0 ** -25 * p * 16   # (sums in another order)
    # a finite mask per q head: the hook's own arithmetic (fp16 scores, fp16 mask addition, fp32 softmax) sits inside the bound,
    # and the mask matters (the unmasked output is outside it)
    m = (-4 * torch.rand(B, Hq, 1, n)).half()
    out4, bound4 = xd.hook_model(q, K, V, Hq // Hkv, mask=m)
    Kr, Vr = K.float().repeat_interleave(Hq // Hkv, 1), V.float().repeat_interleave(Hq // Hkv, 1)
    x = torch.matmul(q.float(), Kr.transpose(2, 3)).half() / math.sqrt(Dd)
    x = torch.max(x + m, torch.tensor(torch.finfo(torch.float16).min, dtype=torch.float16))
    hook = torch.matmul(torch.softmax(x.float(), -1), Vr).half().double()
    assert ((hook - out4).abs() <= bound4).all()
    assert not ((out0 - out4).abs() <= bound4).all()


def test_threaded_oracle_prune_is_the_oracle_prune():
    import numpy as np
    import torch
    from oracle import oracle as orc
    from tests.hd64_util import oracle_prune
    x = np.random.default_rng(4).standard_normal((3, 70000 // 3 + 1, 64)).astype(np.float16)
    x[0, :100] = np.round(x[0, :100] * 2) / 2     # ties
    for s in (0.0, 0.7, 0.99):
        assert np.array_equal(oracle_prune(torch.from_numpy(x), s).numpy().view(np.uint16), orc.prune_magnitude(x, s).view(np.uint16))
