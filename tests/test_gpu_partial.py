"""GPU: the log-sum-exp of the fused decode, window-less calls, the merge of partial attention states and decode_split.

Exact where the data allows it (needles: tests/exact_data.py, tests/hd64_util.py), against float64 models with derived bounds elsewhere
(tests/partial_util.py).  Every test calls a symbol or keyword of ABI 110.  Shapes are small: B' = batch x kv heads is at most 4."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import exact_data as xd
from tests import partial_util as pu
from tests.hd64_ext_util import ExtCase
from tests.hd64_util import DEV, S, Step, _left_pad_mask, needle_data_64, needle_expect_64, oracle_prune

pytestmark = pytest.mark.gpu
NEG = torch.finfo(torch.float16).min
ENGINES = {"default": 0, "valu": 1, "mfma": 2, "dot2": 3}


@pytest.fixture(scope="module")
def pkg():
    from mustafar_amd import _lib, compression
    return _lib.load(), compression


def _rand(B, Hkv, n, groups, Dd, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    K = torch.randn((B, Hkv, n, Dd), generator=g, device=DEV).half()
    V = torch.randn((B, Hkv, n, Dd), generator=g, device=DEV).half()
    q = torch.randn((B, Hkv * groups, 1, Dd), generator=g, device=DEV).half()
    return K, V, q


def _bits(t):
    return t.contiguous().view(torch.int16)


def _plain(st, q, flags=0):
    return st.call(q, flags=flags, fn=lambda *a: st.L.mustafar_decode_attention_hd(*a, st.Dd)).clone()


def _needles(Dd, B, Hq, Hkv, n, pos, seed, pos2=None):
    if Dd == 64:
        return needle_data_64(B, Hq, Hkv, n, pos, seed, pos2=pos2)
    K, V, q, _ = xd.needle_data(B, Hq, Hkv, n, pos, pos2=pos2, k_sparsity=S, seed=seed, device=DEV)
    return K, V, q


def _expect(Dd, V, pos, C, groups, pos2=None, masked_tokens=None):
    """masked_tokens [B, n] bool: tokens masked for every head of the batch entry."""
    Hq = V.shape[1] * groups
    if Dd == 64:
        m = None if masked_tokens is None else np.broadcast_to(masked_tokens[:, None], (V.shape[0], Hq, V.shape[2]))
        return needle_expect_64(V, pos, C, groups, pos2=pos2, masked=m)
    return xd.needle_expect(V, pos, C, S, Hq, pos2=pos2, masked=masked_tokens)


def _assert_lse_model(lse, q, Kp, groups, mask=None, what=""):
    want, bound = pu.lse_model(q, Kp, groups, mask=mask)
    r = pu.lse_ratio(lse, want, bound)
    print(f"{what}: |lse - model| / bound = {r:.3f}")
    assert r <= 1.0, f"{what}: |lse - model| / bound = {r:.3f}"
    return bound


# ---- 1. LSE, exact -----------------------------------------------------------------------------------------------------------------------
def _exact_lse(pkg, Dd, groups, flags=0):
    B, Hkv, C, wl = 1, 2, 512, 70
    n, Hq = C + wl, Hkv * groups
    rng = np.random.default_rng(groups)
    x1, x2 = pu.needle_x(Dd, xd.A1), pu.needle_x(Dd, xd.A2)
    # block and slab edges, the compressed / window seam, the last stored row and the step's new row
    edges = sorted({0, C - 1, C, n - 1, n - 2} | {b for b in range(0, C, 64)} | {b + 63 for b in range(0, C, 64)})
    for i in range(0, len(edges), B * Hq):
        chunk = edges[i:i + B * Hq]
        pos = np.concatenate([chunk, rng.integers(0, n, B * Hq - len(chunk))]).reshape(B, Hq)
        K, V, q = _needles(Dd, B, Hq, Hkv, n, pos, seed=i)
        st = Step(pkg, K, V, C, groups)
        out, lse = pu.call_lse(st, q, flags=flags)
        want = _expect(Dd, V, pos, C, groups)
        assert not (out.float() != want.float()).any(), "rows miss their needle"
        assert torch.equal(lse, torch.full_like(lse, x1)), f"lse {lse.tolist()} != the needle's x {x1}"
        # the output bits are the plain entry point's, and lse == NULL runs the plain launches
        ref = _plain(Step(pkg, K, V, C, groups), q, flags)
        choice = st.L.mustafar_last_decode_choice()
        assert torch.equal(_bits(out), _bits(ref))
        out0, _ = pu.call_lse(Step(pkg, K, V, C, groups), q, flags=flags, lse=False)
        assert torch.equal(_bits(out0), _bits(ref)) and st.L.mustafar_last_decode_choice() == choice
    # two equal needles, in different slabs and across the seam: x + log 2 within one fp32 ulp of that value
    pos = np.stack([rng.integers(0, C // 2, (B, Hq)), rng.integers(C // 2 + 64, n, (B, Hq))], -1)
    pos[0, 0] = (C - 1, C)
    pos[0, 1] = (63, n - 1)
    K, V, q = _needles(Dd, B, Hq, Hkv, n, pos, seed=99)
    out, lse = pu.call_lse(Step(pkg, K, V, C, groups), q, flags=flags)
    assert not (out.float() != _expect(Dd, V, pos, C, groups).float()).any()
    want = x1 + math.log(2.0)
    assert float((lse.double() - want).abs().max()) <= float(np.spacing(np.float32(want))), lse.tolist()
    # a masked primary needle: the secondary's x exactly
    pos1 = np.stack([rng.permutation(n // 2)[:Hq] for _ in range(B)])
    pos2 = np.stack([n // 2 + rng.permutation(n - n // 2)[:Hq] for _ in range(B)])
    pos2[0, 0], pos1[0, 1] = n - 1, 63
    K, V, q = _needles(Dd, B, Hq, Hkv, n, pos1, seed=7, pos2=pos2)
    mask = torch.zeros((B, 1, 1, n), dtype=torch.float16, device=DEV)
    masked = np.zeros((B, n), bool)
    for b in range(B):
        masked[b, pos1[b]] = True
    mask[torch.from_numpy(masked)[:, None, None, :].to(DEV)] = NEG
    out, lse = pu.call_lse(Step(pkg, K, V, C, groups, mask=mask), q, flags=flags)
    assert not (out.float() != _expect(Dd, V, pos1, C, groups, pos2=pos2, masked_tokens=masked).float()).any()
    assert torch.equal(lse, torch.full_like(lse, x2)), f"lse {lse.tolist()} != the secondary needle's x {x2}"


@pytest.mark.parametrize("groups", [1, 3, 4, 8])
def test_lse_exact_on_needles_64(pkg, groups):
    _exact_lse(pkg, 64, groups)


# D = 128: knobs select the one-pass kernel (8: 0 = lean pair instead of the super-block form; 11: 0 = never the small-launch kernel) and the
# row kernel (10: 0 = onepass_finish_kernel<1> instead of onepass_finish1_kernel); the forms' codes are those of mustafar_last_decode_choice
FORMS_128 = {"small": ((), 4), "sb": (((11, 0),), 3), "pair": (((8, 0), (11, 0)), 2), "small_finish": (((10, 0),), 4)}
RESET = {8: 1, 10: 1, 11: 1}


@pytest.mark.parametrize("groups,engine,form", [(1, "default", "small"), (2, "default", "sb"), (4, "valu", "small"), (4, "mfma", "sb"),
                                                (4, "dot2", "small"), (4, "dot2", "sb"), (4, "dot2", "pair"), (4, "valu", "pair"),
                                                (4, "dot2", "small_finish"), (2, "default", "pair")])
def test_lse_exact_on_needles_128(pkg, groups, engine, form):
    """The dot2 cases check that the engine's 2^15 has left the slab sums: a scaled sum would add 15 log 2 to the LSE."""
    L_ = pkg[0]
    knobs, code = FORMS_128[form]
    try:
        for k, v in knobs:
            assert L_.mustafar_tune(k, v) == 0
        _exact_lse(pkg, 128, groups, flags=ENGINES[engine] | (2 << 4))
        choice = L_.mustafar_last_decode_choice()
        assert (choice >> 4) & 1 == 1 and (choice >> 8) & 15 == code, f"{form}: choice {choice:#x}"
        if groups == 4 and engine != "default":
            assert choice & 15 == {"valu": 0, "mfma": 1, "dot2": 2}[engine]
    finally:
        for k, _ in knobs:
            L_.mustafar_tune(k, RESET[k])


# ---- 2. LSE, random data -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 3, 4, 8])
@pytest.mark.parametrize("C,wl", [(0, 1), (0, 70), (64, 33), (4096, 130)])
def test_lse_model_64(pkg, groups, C, wl):
    B, Hkv = 2, 2
    K, V, q = _rand(B, Hkv, C + wl, groups, 64, seed=C + wl + groups)
    st = Step(pkg, K, V, C, groups)
    out, lse = pu.call_lse(st, q)
    Kp, Vp = pu.pruned_rows(K, V, C)
    _assert_lse_model(lse, q, Kp, groups, what=f"D=64 g{groups} C{C} wl{wl}")
    xd.model_ok(out, q, K, V, C, groups, pruned=(Kp[:, :, :C], Vp[:, :, :C]) if C else None)
    assert torch.equal(_bits(out), _bits(_plain(Step(pkg, K, V, C, groups), q)))


def test_lse_model_64_left_padded(pkg):
    B, Hkv, groups, C, wl = 2, 2, 4, 640, 90
    K, V, q = _rand(B, Hkv, C + wl, groups, 64, seed=5)
    mask = _left_pad_mask(B, C + wl, [37, 700])          # the second pad reaches into the window
    out, lse = pu.call_lse(Step(pkg, K, V, C, groups, mask=mask), q)
    Kp, _ = pu.pruned_rows(K, V, C)
    _assert_lse_model(lse, q, Kp, groups, mask=mask, what="D=64 left padded")
    xd.model_ok(out, q, K, V, C, groups, pads=[37, 700])


def test_lse_model_64_extents_with_t_device_below_the_capacity(pkg):
    """The EXT instantiation sized for 1024 tokens with 512 in use: slabs of weight zero behind *T_device, and the LSE of the tokens in use."""
    L_ = pkg[0]
    B, Hkv, groups, T_base, n_ext, wl = 1, 2, 4, 256, 1, 40
    T = T_base + 256 * n_ext
    K, V, q = _rand(B, Hkv, T + wl, groups, 64, seed=21)
    ec = ExtCase(pkg, K, V, T_base, n_ext, groups, S, S, cap_T=1024)
    t_dev = torch.tensor([T], dtype=torch.int32, device=DEV)
    lse = torch.full((B, Hkv * groups), float("nan"), dtype=torch.float32, device=DEV)
    tail = ec._tail(q, ec.cap_T, ec.wl, None, None, 0)
    err = L_.mustafar_decode_attention_extents_lse_hd(torch.cuda.current_stream().cuda_stream, ec.kc.view_ptr(), ec.vc.view_ptr(), T_base,
                                                      ec.kc.table.data_ptr(), ec.vc.table.data_ptr(), *tail, t_dev.data_ptr(), 64, lse.data_ptr())
    assert err == 0 and (L_.mustafar_last_decode_choice() >> 8) & 15 == 6
    out = ec.out.clone()
    Kp = torch.cat([ec.Kp, K[:, :, T:]], 2)
    _assert_lse_model(lse, q, Kp, groups, what="D=64 extents, T_device")
    assert torch.equal(_bits(out), _bits(ec.call_ext(q, t_device=t_dev)))


def _slabs_128(T, Bp, groups, cap):
    """NS + nchunks of decode_attention's one-pass launch (spmv.hip): blocks per workgroup 4 from 768 workgroups on, else 2; one slab per
    workgroup; one window slab per 64 rows of the window capacity."""
    G = 4 if groups % 4 == 0 else 2 if groups % 2 == 0 else 1
    gy, ntb = Bp * (groups // G), T // 64
    per_wg = 4 if ((ntb + 3) // 4) * gy >= 768 else 2
    return -(-ntb // per_wg) + -(-cap // 64)


# (groups, engine, T, the row kernel the slab count is meant to reach)
CASES_128 = [(1, "default", 1024, "finish1"), (2, "default", 7680, "finish1"), (4, "valu", 2048, "finish1"), (4, "mfma", 8192, "<2>"),
             (4, "dot2", 12288, "<2>"), (4, "dot2", 17920, "<8>"), (2, "default", 17920, "<8>"), (4, "dot2", 3072, "<1>")]


@pytest.mark.parametrize("groups,engine,T,variant", CASES_128)
def test_lse_model_128(pkg, groups, engine, T, variant):
    L_ = pkg[0]
    B, Hkv, wl, cap = 1, 2, 40, 64
    NSL = _slabs_128(T, B * Hkv, groups, cap)
    assert {"finish1": NSL <= 64, "<1>": NSL <= 64, "<2>": 64 < NSL <= 128, "<8>": NSL > 128}[variant], (NSL, variant)
    K, V, q = _rand(B, Hkv, T + wl, groups, 128, seed=T // 64 + groups)
    Kp, Vp = pu.pruned_rows(K, V, T)
    flags = ENGINES[engine] | (2 << 4)
    try:
        if variant == "<1>":
            assert L_.mustafar_tune(10, 0) == 0
        st = Step(pkg, K, V, T, groups, cap=cap, pruned=(Kp[:, :, :T], Vp[:, :, :T]))
        out, lse = pu.call_lse(st, q, flags=flags)
        ref = _plain(Step(pkg, K, V, T, groups, cap=cap, pruned=(Kp[:, :, :T], Vp[:, :, :T])), q, flags)
    finally:
        L_.mustafar_tune(10, 1)
    _assert_lse_model(lse, q, Kp, groups, what=f"D=128 g{groups} {engine} T{T} ({NSL} slabs, {variant})")
    xd.model_ok(out, q, K, V, T, groups, pruned=(Kp[:, :, :T], Vp[:, :, :T]))
    assert torch.equal(_bits(out), _bits(ref))


def _hook(Dd, Hq, Hkv, **kw):
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    return MustafarAttention(MustafarConfig(num_attention_heads=Hq, num_key_value_heads=Hkv, head_dim=Dd, k_sparsity=S, v_sparsity=S,
                                            api="fused", **kw))


def test_lse_model_128_extents_through_the_hook(pkg):
    """An arena that has grown by one extent (the trigger runs inside the loop): decode_fused(return_lse=True) over base views + table."""
    B, Hq, Hkv, groups, prefill = 1, 8, 2, 4, 288 + 250
    attn = _hook(128, Hq, Hkv, arena=True)
    K, V, _ = _rand(B, Hkv, prefill + 12, groups, 128, seed=3)
    g = torch.Generator(device=DEV).manual_seed(4)
    past = attn.to_fused(attn.build_cache(K[:, :, :prefill].contiguous(), V[:, :, :prefill].contiguous()))
    assert past[4] == 256
    for i in range(12):
        n = prefill + i + 1
        C = past[4]
        q = torch.randn((B, Hq, 1, 128), generator=g, device=DEV).half()
        out, lse, past = attn.decode_fused(q, K[:, :, n - 1:n], V[:, :, n - 1:n], past, return_lse=True)
        if C == 512:
            assert past[0].extents, "the cache did not grow by an extent"
        Kp, Vp = pu.pruned_rows(K[:, :, :n], V[:, :, :n], C)
        _assert_lse_model(lse, q, Kp, groups, what=f"D=128 hook step {i} (C {C})")
        xd.model_ok(out, q, K[:, :, :n], V[:, :, :n], C, groups, pruned=(Kp[:, :, :C], Vp[:, :, :C]))
    assert past[4] == 512


def test_return_lse_names_the_calls_it_cannot_serve(pkg):
    K, V, q = _rand(1, 2, 40, 4, 128, seed=1)
    attn = _hook(128, 8, 2)
    with pytest.raises(ValueError, match="no compressed tokens"):
        attn.decode_fused(q, K[:, :, 39:], V[:, :, 39:], attn.build_cache(K[:, :, :39], V[:, :, :39]), return_lse=True)
    attn = _hook(128, 8, 2, structure="two_launch")
    K, V, q = _rand(1, 2, 300, 4, 128, seed=1)
    with pytest.raises(ValueError, match="two_launch"):
        attn.decode_fused(q, K[:, :, 299:], V[:, :, 299:], attn.build_cache(K[:, :, :299].contiguous(), V[:, :, :299].contiguous()), return_lse=True)


# ---- 3. window-less ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dd", [64, 128])
@pytest.mark.parametrize("T", [64, 4096])
def test_window_less_calls(pkg, Dd, T):
    B, Hkv, groups = 1, 2, 4
    Hq = Hkv * groups
    # window buffers poisoned with NaN live somewhere else in memory: none is passed, none may matter
    poison = torch.full((2, B, Hkv, 64, Dd), float("nan"), dtype=torch.float16, device=DEV)
    # exact: needles on the edges of the segment
    rng = np.random.default_rng(T + Dd)
    edges = [0, 63, T - 64, T - 1] + ([64, 2047, 2048, T // 2 + 63] if T > 64 else [])
    pos = np.concatenate([edges, rng.integers(0, T, B * Hq)])[:B * Hq].reshape(B, Hq)
    K, V, q = _needles(Dd, B, Hq, Hkv, T, pos, seed=T)
    Kp, Vp = pu.pruned_rows(K, V, T)
    out, lse = pu.Segment(pkg, Kp, Vp, groups).call(q)
    assert not (out.float() != _expect(Dd, V, pos, T, groups).float()).any()
    assert torch.equal(lse, torch.full_like(lse, pu.needle_x(Dd, xd.A1)))
    # random data, plain and with a mask whose rows are longer than the segment (the pointer moved to the segment's first column)
    K, V, q = _rand(B, Hkv, T, groups, Dd, seed=T + 1)
    Kp, Vp = pu.pruned_rows(K, V, T)
    seg = pu.Segment(pkg, Kp, Vp, groups)
    out, lse = seg.call(q)
    _assert_lse_model(lse, q, Kp, groups, what=f"D={Dd} window-less T{T}")
    xd.model_ok(out, q, K, V, T, groups, pruned=(Kp, Vp))
    full = _left_pad_mask(B, T + 100, [100 + T // 2 - 7])
    m = full[..., 100:]
    assert m.data_ptr() == full.data_ptr() + 200
    out, lse = seg.call(q, mask=m)
    _assert_lse_model(lse, q, Kp, groups, mask=m[..., :T], what=f"D={Dd} window-less T{T} masked")
    xd.model_ok(out, q, K, V, T, groups, pads=[T // 2 - 7], pruned=(Kp, Vp))
    assert torch.isnan(poison).all()


# ---- 4. the merge kernel alone -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dd", [64, 128])
@pytest.mark.parametrize("n", [1, 2, 3, 64])
def test_merge_kernel(pkg, Dd, n):
    L_ = pkg[0]
    BH = 7   # (not a multiple of the rows per workgroup)
    g = torch.Generator(device=DEV).manual_seed(n + Dd)
    outs = torch.randn((n, BH, Dd), generator=g, device=DEV).half()
    lses = (torch.randn((n, BH), generator=g, device=DEV) * 4 + 3).float()
    lses[n // 2, 1] = float("-inf")                      # a part that is empty for one row
    lses[:, 2] = float("-inf")                           # a row whose parts are all empty
    if n > 1:
        lses[0, 3], lses[1:, 3] = 150.0, -50.0           # LSEs 200 apart: the weight is exactly 0
    for strides in ((None, None), (BH * Dd + 24, BH + 5)):
        for want_lse in (True, False):
            out, lse = pu.call_merge(L_, outs, lses, *strides, want_lse=want_lse)
            want, want_lse_v, bound = pu.merge_model(outs, lses)
            r = float(((out.double() - want).abs() / bound).max())
            print(f"merge D={Dd} n={n} strides={strides}: |out - model| / bound = {r:.3f}")
            assert r <= 1.0
            assert not out[2].any(), "every part empty: out = 0"
            if n > 1:
                assert torch.equal(_bits(out[3]), _bits(outs[0, 3])), "a part 200 below must weigh exactly nothing"
            if n == 1:
                keep = [r_ for r_ in range(BH) if r_ != 2 and not (r_ == 1)]
                assert torch.equal(_bits(out[keep]), _bits(outs[0, keep])), "one part: its own bits"
            if want_lse:
                assert lse[2] == float("-inf")
                fin = torch.isfinite(want_lse_v)
                err = (lse.double() - want_lse_v)[fin].abs()
                assert float((err / (2.0 ** -21 * (want_lse_v[fin].abs() + 1))).max()) <= 1.0
                assert torch.equal(torch.isfinite(lse), fin)


# ---- 5. split against whole, exact ---------------------------------------------------------------------------------------------------
def _segment_cache(kind, Kp, Vp, attn):
    """The pruned rows [B, Hkv, t, D] of one frozen segment as the cache kind asked for: (k_cache, v_cache, tokens)."""
    from mustafar_amd.cache import CompressedArena
    from mustafar_amd.cache64 import ExtentCache64
    from mustafar_amd.hook import _compress
    B, Hkv, t, Dd = Kp.shape
    kc = _compress(Kp.reshape(B * Hkv, t, Dd).contiguous(), "key")
    vc = _compress(Vp.reshape(B * Hkv, t, Dd).contiguous(), "value")
    if kind == "arena":
        return CompressedArena.from_reference(kc, "key", t), CompressedArena.from_reference(vc, "value", t), t
    if kind == "ext64":
        return ExtentCache64(kc, "key", B * Hkv, t), ExtentCache64(vc, "value", B * Hkv, t), t
    return kc, vc, t


def _live_past(attn, K, V, lo, n):
    """The live cache over tokens [lo, n - 1): prefill of the raw rows (the hook prunes and compresses its first ((len - R) // 256) * 256)."""
    return attn.to_fused(attn.build_cache(K[:, :, lo:n - 1].contiguous(), V[:, :, lo:n - 1].contiguous()))


@pytest.mark.parametrize("Dd,kind,live_kw", [(64, "tuple", {}), (64, "ext64", {"hd64_extents": True}), (128, "arena", {"arena": True}),
                                             (128, "tuple", {})])
def test_split_equals_whole_on_needles(pkg, Dd, kind, live_kw):
    B, Hkv, groups = 1, 2, 4
    Hq = Hkv * groups
    F, n = 512, 512 + 256 + 40 + 1             # frozen tokens (a multiple of 64), then a live cache of 256 compressed + 40 window rows + the new row
    C_all = F + 256                            # tokens that are pruned in either part
    attn = _hook(Dd, Hq, Hkv, **live_kw)
    rng = np.random.default_rng(Dd)
    pos = np.array([[0, F - 1, F, F + 255, F + 256, n - 1, 64, n - 2]])      # needles in either part, on the cut and on the seams
    both = np.stack([rng.integers(0, F, (B, Hq)), rng.integers(F, n, (B, Hq))], -1)   # two equal needles, one in each part
    both[0, 0], both[0, 1] = (F - 1, F), (0, n - 1)
    for p in (pos, both):
        K, V, q = _needles(Dd, B, Hq, Hkv, n, p, seed=int(p.sum()) % 1000)
        Kp, Vp = pu.pruned_rows(K, V, C_all)
        frozen = [_segment_cache(kind, Kp[:, :, :F], Vp[:, :, :F], attn)]
        past = _live_past(attn, K, V, F, n)
        assert past[4] == 256
        out, new = attn.decode_split(q, K[:, :, n - 1:], V[:, :, n - 1:], past, frozen)
        want = _expect(Dd, V, p, C_all, groups)
        miss = xd.needle_misses(out, want)
        assert not miss.any(), f"rows {miss.nonzero().tolist()} differ from the whole"
        assert new[5] == n - F and new[4] == 256


# ---- 6. split against whole, random --------------------------------------------------------------------------------------------------
def _split_bound(parts, lse_bounds, out_all, bound_all):
    """The model's bound of the whole + the parts' own roundings and LSE errors carried through the merge: parts = [(out_i fp64, W_i)],
    W_i the part's share of the whole's denominator.  bound = bound_all + sum_i W_i (2^-11 |out_i| + 2^-25)
    + 2 max_j bound_lse_j * sum_i W_i |out_i - out|."""
    extra = sum(W[..., None, None] * (2.0 ** -11 * o.abs() + 2.0 ** -25) for o, W in parts)
    worst = torch.stack(lse_bounds).amax(0)
    spread = sum(W[..., None, None] * (o - out_all).abs() for o, W in parts)
    return bound_all + extra + 2 * worst[..., None, None] * spread


EXT64, ARENA = {"hd64_extents": True}, {"arena": True}
# (head_dim, kind of the frozen segments and of the live cache, hook options, cuts between the frozen segments and the live cache, masked);
# the masked cases run with two frozen segments: the second batch entry's left padding covers the first and reaches into the second
SPLITS = [(64, "tuple", {}, (256,), False), (64, "tuple", {}, (192, 448), False), (64, "tuple", {}, (192, 448), True),
          (64, "ext64", EXT64, (256,), False), (64, "ext64", EXT64, (256, 512), False), (64, "ext64", EXT64, (256, 512), True),
          (128, "arena", ARENA, (256,), False), (128, "arena", ARENA, (256, 768), False), (128, "arena", ARENA, (256, 768), True)]


@pytest.mark.parametrize("Dd,kind,live_kw,cuts,masked", SPLITS)
def test_split_equals_whole_on_random_data(pkg, Dd, kind, live_kw, cuts, masked):
    B, Hkv, groups = 2, 2, 4
    Hq = Hkv * groups
    F = cuts[-1]
    n = F + 256 + 50 + 1
    C_all = F + 256
    attn = _hook(Dd, Hq, Hkv, **live_kw)
    K, V, q = _rand(B, Hkv, n, groups, Dd, seed=F + Dd)
    Kp, Vp = pu.pruned_rows(K, V, C_all)     # per-token pruning: separately compressed segments hold the same rows
    bounds_ = (0,) + tuple(cuts)
    frozen = [_segment_cache(kind, Kp[:, :, a:b], Vp[:, :, a:b], attn) for a, b in zip(bounds_[:-1], bounds_[1:])]
    mask = _left_pad_mask(B, n, [0, cuts[0] + 37]) if masked else None      # the second entry's padding reaches into the second segment
    past = _live_past(attn, K, V, F, n)
    out, new = attn.decode_split(q, K[:, :, n - 1:], V[:, :, n - 1:], past, frozen, attention_mask=mask)
    want, bound = xd.hook_model(q, Kp, Vp, groups, mask=mask)
    # the parts as the model sees them: each one's output, its share of the denominator, its LSE bound
    lse_all, _ = pu.lse_model(q, Kp, groups, mask=mask)
    parts, lse_bounds = [], []
    for a, b in list(zip(bounds_[:-1], bounds_[1:])) + [(F, n)]:
        mb = mask[..., a:b] if masked else None
        o_i, _ = xd.hook_model(q, Kp[:, :, a:b], Vp[:, :, a:b], groups, mask=mb)
        l_i, bl_i = pu.lse_model(q, Kp[:, :, a:b], groups, mask=mb)
        parts.append((o_i, torch.exp(l_i - lse_all)))
        lse_bounds.append(bl_i)
    total = _split_bound(parts, lse_bounds, want, bound)
    r = float(((out.double() - want).abs() / total).max())
    print(f"split D={Dd} {kind} cuts={cuts} masked={masked}: |split - whole model| / bound = {r:.3f}")
    assert r <= 1.0
    assert new[4] == 256 and new[5] == n - F


# ---- 7. graph -----------------------------------------------------------------------------------------------------------------------
def test_lse_under_graph_replay_64(pkg):
    L_ = pkg[0]
    B, Hq, Hkv, groups, prefill, steps = 1, 8, 2, 4, 256 + 40, 20
    attn = _hook(64, Hq, Hkv)
    K, V, _ = _rand(B, Hkv, prefill + steps, groups, 64, seed=8)
    g = torch.Generator(device=DEV).manual_seed(9)
    qs_all = torch.randn((steps, B, Hq, 1, 64), generator=g, device=DEV).half()
    past = attn.to_fused(attn.build_cache(K[:, :, :prefill].contiguous(), V[:, :, :prefill].contiguous()))
    C = past[4]
    assert C == 256
    counter = torch.zeros((1,), dtype=torch.int32, device=DEV)
    q_in, k_in, v_in = torch.empty_like(qs_all[0]), torch.empty_like(K[:, :, :1]).contiguous(), torch.empty_like(V[:, :, :1]).contiguous()
    q_in.copy_(qs_all[0]); k_in.copy_(K[:, :, prefill:prefill + 1]); v_in.copy_(V[:, :, prefill:prefill + 1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        attn.decode_fused(q_in, k_in, v_in, past, step_counter=counter, return_lse=True)      # warm-up (scratch allocated outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse, _ = attn.decode_fused(q_in, k_in, v_in, past, step_counter=counter, return_lse=True)
    Kp_c, Vp_c = oracle_prune(K[:, :, :C], S), oracle_prune(V[:, :, :C], S)
    for i in range(steps):
        n = prefill + i + 1
        q_in.copy_(qs_all[i]); k_in.copy_(K[:, :, n - 1:n]); v_in.copy_(V[:, :, n - 1:n])
        graph.replay()
        torch.cuda.synchronize()
        Kp = torch.cat([Kp_c, K[:, :, C:n]], 2)
        _assert_lse_model(lse, qs_all[i], Kp, groups, what=f"graph replay {i}")
        xd.model_ok(out, qs_all[i], K[:, :, :n], V[:, :, :n], C, groups, pruned=(Kp_c, Vp_c))
        assert L_.mustafar_counter_add(torch.cuda.current_stream().cuda_stream, counter.data_ptr(), 1) == 0
    torch.cuda.synchronize()
