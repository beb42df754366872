"""GPU: head_dim 64 -- prune and the two-pass conversion bit-exact against the reference's fixtures and the oracle, the fused decode
(mustafar_decode_attention_hd) against the float64 model of the hook's arithmetic and on exactly checkable needle data, and the hook end
to end at Llama-3.2-1B head geometry (32 q / 8 kv heads, D = 64) against the dense decode over the oracle-pruned cache."""
import os

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from oracle.dense_ref import dense_decode_layer
from tests.exact_data import model_ok
from tests.hd64_util import DEV, D, S, Step, _left_pad_mask, _rand, _t, needle_data_64, needle_expect_64
from tests.util import DENSE_ULPS, excess

pytestmark = pytest.mark.gpu
CHOICE_D64 = (1 << 4) | (5 << 8)   # engine 0, structure 1 (one pass), form 5 (mustafar_hip.h)


@pytest.fixture(scope="module")
def pkg():
    from mustafar_amd import _lib, compression
    return _lib.load(), compression


# ---- prune and conversions ---------------------------------------------------------------------------------------------------------
def test_prune_bit_exact(pkg, golden_dir):
    _, comp = pkg
    g = np.load(os.path.join(golden_dir, "prune_reference.npz"))
    x = g["d64_s0.7__x"]
    got = comp.prune_magnitude(_t(x.view(np.float16)), float(g["d64_s0.7__s"])).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, g["d64_s0.7__y"])
    rng = np.random.default_rng(11)
    for s in (0.0, 0.5, 0.7, 0.8, 0.99):
        x = rng.standard_normal((3, 5, 77, D)).astype(np.float16)
        x[0, 0, :10] = np.round(x[0, 0, :10] * 2) / 2                     # ties
        x[0, 1, :4] = np.float16(0.5)                                      # all equal
        x[0, 1, 4:8] = 0
        x[0, 1, 8:12] = np.float16(-0.0)                                   # -0.0 rows
        x[1, 2, :5, ::2] = -x[1, 2, :5, 1::2]                              # equal magnitudes of both signs
        got = comp.prune_magnitude(_t(x), s).cpu().numpy().view(np.uint16)
        assert np.array_equal(got, orc.prune_magnitude(x, s).view(np.uint16)), s


@pytest.mark.parametrize("which", ["key", "value"])
def test_compress_bit_exact(pkg, golden_dir, which):
    _, comp = pkg
    conv = comp.convert_key_batched if which == "key" else comp.convert_value_batched
    oconv = orc.convert_key_batched if which == "key" else orc.convert_value_batched
    g = np.load(os.path.join(golden_dir, "compress_reference.npz"))
    x = g["d64__x"]
    bmp, accum, nzs = conv(_t(x.view(np.float16)))
    assert bmp.shape == (2, 64) and accum.shape == (2, 65) and len(nzs) == 2
    assert np.array_equal(bmp.cpu().numpy(), g[f"d64__{which}__bmp"])
    assert np.array_equal(accum.cpu().numpy(), g[f"d64__{which}__accum"])
    assert np.array_equal(torch.cat(nzs).cpu().numpy().view(np.uint16), g[f"d64__{which}__packed"])
    rng = np.random.default_rng(5)
    for (B, t, s) in [(1, 64, 0.7), (3, 2048, 0.7), (5, 192, 0.5), (2, 4096, 0.8), (3, 128, 0.0), (1, 2112, 0.99)]:
        x = orc.prune_magnitude(rng.standard_normal((B, t, D)).astype(np.float16), s)
        x[B // 2, 64:128] = 0                                                  # an all-zero block (when there is one)
        x[0, :3, :5] = np.float16(-0.0)
        bmp, accum, nzs = conv(_t(x))
        obmp, oacc, onz = oconv(x)
        assert np.array_equal(bmp.cpu().numpy(), obmp) and np.array_equal(accum.cpu().numpy(), oacc), (B, t, s)
        assert np.array_equal(torch.cat(nzs).cpu().numpy().view(np.uint16), np.concatenate(onz).view(np.uint16)), (B, t, s)


# ---- fused decode through the C ABI (operands and data: tests/hd64_util.py) -----------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("C,wl", [(0, 1), (0, 70), (64, 33), (4096, 64), (4096, 130)])
def test_decode_model(pkg, groups, C, wl):
    L_, _ = pkg
    B, Hkv = 2, 2
    K, V, q = _rand(B, Hkv, C + wl, groups, seed=C + wl + groups)
    st = Step(pkg, K, V, C, groups)
    out = st.call(q)
    assert L_.mustafar_last_decode_choice() == CHOICE_D64
    model_ok(out, q, K, V, C, groups)
    # the new rows were appended at window row wl - 1
    assert torch.equal(st.kw[:, :, wl - 1], K[:, :, -1]) and torch.equal(st.vw[:, :, wl - 1], V[:, :, -1])
    # every engine flag runs the same exact engine: the same bits
    for flags in (1, 2, 3, 2 << 4):
        st2 = Step(pkg, K, V, C, groups)
        assert torch.equal(st2.call(q, flags=flags).view(torch.int16), out.view(torch.int16)), flags


@pytest.mark.parametrize("groups", [1, 4, 8])
def test_decode_model_masked(pkg, groups):
    B, Hkv, C, wl = 3, 2, 640, 90
    K, V, q = _rand(B, Hkv, C + wl, groups, seed=77 + groups)
    pads = [0, 37, 700]          # the last pad reaches into the window
    st = Step(pkg, K, V, C, groups, mask=_left_pad_mask(B, C + wl, pads))
    model_ok(st.call(q), q, K, V, C, groups, pads=pads)


@pytest.mark.parametrize("C", [32768])
@pytest.mark.parametrize("groups", [4, 8])
def test_decode_model_long(pkg, C, groups):
    B, Hkv, wl = 1, 2, 40
    K, V, q = _rand(B, Hkv, C + wl, groups, seed=groups)
    model_ok(Step(pkg, K, V, C, groups).call(q), q, K, V, C, groups)


def test_decode_graph_replay_with_window_len_extra(pkg):
    L_, _ = pkg
    B, Hkv, groups, C, w0, steps = 2, 2, 4, 1024, 20, 40
    n_all = C + w0 + steps
    K, V, q = _rand(B, Hkv, n_all, groups, seed=3)
    pads = [0, 300]
    mask = _left_pad_mask(B, C + 128, pads)                  # rows cover the window capacity
    extra = torch.zeros((1,), dtype=torch.int32, device=DEV)
    st = Step(pkg, K[:, :, :C + w0], V[:, :, :C + w0], C, groups, cap=128, mask=mask, extra=extra)
    qs = torch.empty_like(q)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        st.call(qs)                                           # warm-up (extra = 0: the first step)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st.call(qs)
    for i in range(steps):
        n = C + w0 + i
        st.kn.copy_(K[:, :, n - 1])
        st.vn.copy_(V[:, :, n - 1])
        qs.copy_(q * (1 + i % 3))
        graph.replay()
        torch.cuda.synchronize()
        model_ok(st.out, qs, K[:, :, :n], V[:, :, :n], C, groups, pads=pads)
        assert L_.mustafar_counter_add(torch.cuda.current_stream().cuda_stream, extra.data_ptr(), 1) == 0
    torch.cuda.synchronize()
    assert torch.equal(st.kw[:, :, :w0 + steps - 1], K[:, :, C:n_all - 1])


# ---- needles: exactly checkable outputs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 3, 4, 8])
def test_decode_needles_bit_exact(pkg, groups):
    B, Hkv, C, wl = 2, 2, 512, 70
    n = C + wl
    rng = np.random.default_rng(groups)
    edges = sorted({0, C - 1, C, n - 1, n - 2} | {b for b in range(0, C, 64)} | {b + 63 for b in range(0, C, 64)})
    Hq = Hkv * groups
    for i in range(0, len(edges), B * Hq):
        chunk = edges[i:i + B * Hq]
        pos = np.concatenate([chunk, rng.integers(0, n, B * Hq - len(chunk))]).reshape(B, Hq)
        K, V, q = needle_data_64(B, Hq, Hkv, n, pos, seed=i)
        out = Step(pkg, K, V, C, groups).call(q)
        want = needle_expect_64(V, pos, C, groups)
        bad = (out.float() != want.float()).any(-1)
        assert not bad.any(), f"rows {bad.nonzero().tolist()} miss their needle"


def test_head_dim_128_forwards_bit_identically(pkg):
    L_, comp = pkg
    from mustafar_amd.hook import nz_offset_from_idxs
    B, Hkv, groups, C, wl, Dd = 2, 2, 4, 512, 40, 128
    g = torch.Generator(device=DEV).manual_seed(9)
    K = torch.randn((B, Hkv, C + wl, Dd), generator=g, device=DEV).half()
    V = torch.randn((B, Hkv, C + wl, Dd), generator=g, device=DEV).half()
    q = torch.randn((B, Hkv * groups, 1, Dd), generator=g, device=DEV).half()
    outs = []
    for fn in (None, L_.mustafar_decode_attention):
        st = Step(pkg, K, V, C, groups)
        st.ws = torch.empty((L_.mustafar_decode_workspace_bytes(C, st.BH, groups, 1),), dtype=torch.uint8, device=DEV)
        outs.append(st.call(q, head_dim=128, fn=fn).clone())
        if fn is None:
            assert (L_.mustafar_last_decode_choice() >> 8) != 5
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


# ---- the hook end to end -----------------------------------------------------------------------------------------------------------
def test_hook_end_to_end_llama_3_2_1b_heads(pkg):
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    Hq, Hkv, B, prefill, steps = 32, 8, 1, 1000, 600
    attn = MustafarAttention(MustafarConfig(num_attention_heads=Hq, num_key_value_heads=Hkv, head_dim=D, api="fused", residual_length=32))
    g = torch.Generator(device=DEV).manual_seed(1)
    n_all = prefill + steps
    K = torch.randn((B, Hkv, n_all, D), generator=g, device=DEV).half()
    V = torch.randn((B, Hkv, n_all, D), generator=g, device=DEV).half()
    Kpr = torch.from_numpy(orc.prune_magnitude(K.cpu().numpy(), S)).to(DEV)   # the prune is per row: every row's pruned form at once
    Vpr = torch.from_numpy(orc.prune_magnitude(V.cpu().numpy(), S)).to(DEV)
    past = attn.build_cache(K[:, :, :prefill], V[:, :, :prefill])
    assert past[4] == 768
    triggers, worst = 0, 0.0
    for i in range(steps):
        n = prefill + i + 1
        C = past[4]
        q = torch.randn((B, Hq, 1, D), generator=g, device=DEV).half()
        out, past = attn.decode(q, K[:, :, n - 1:n], V[:, :, n - 1:n], past)
        triggers += past[4] != C
        Kd = torch.cat([Kpr[:, :, :C], K[:, :, C:n]], 2)
        Vd = torch.cat([Vpr[:, :, :C], V[:, :, C:n]], 2)
        want = dense_decode_layer(q, Kd, Vd, Hq // Hkv)
        e = excess(out, want, DENSE_ULPS)
        worst = max(worst, e)
        assert e <= 1.0, f"step {i} (kv {n}, compressed {C}): {e:.2f} x the bound"
    assert triggers >= 2 and past[4] == 768 + 256 * triggers
