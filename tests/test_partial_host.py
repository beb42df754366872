"""CPU: the partial-attention surface of the C ABI (ABI 110) checked without a GPU -- every call here fails validation before any launch --
and, in fp32 / fp16 numpy, the claims the exact GPU tests of tests/test_gpu_partial.py rest on."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import exact_data as xd
from tests import partial_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mustafar_decode_attention_lse_hd", "mustafar_decode_attention_extents_lse_hd", "mustafar_merge_attention_states")
ONE = 16   # a pointer that is never dereferenced (16-byte aligned, so that only the argument under test is wrong)


def _lib():
    from mustafar_amd import _lib as lib
    return lib.load()


def test_abi_110_declares_binds_and_exports_the_new_symbols():
    from mustafar_amd import _lib as lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mustafar_hip.h")).read(), flags=re.S)
    syms = set(re.findall(r"^\s*(?:int|int64_t)\s+(\w+)\s*\(", text, flags=re.M))
    raw = ctypes.CDLL(lib.LIB_PATH)
    for s in NEW:
        assert s in syms and s in lib.SIGNATURES and hasattr(raw, s), s
    assert _lib().mustafar_abi_version() >= 110


def _args(**kw):
    a = dict(k_bmp=ONE, k_nz=ONE, k_idx=ONE, k_off=ONE, v_bmp=ONE, v_nz=ONE, v_idx=ONE, v_off=ONE, q=ONE, kw=ONE, vw=ONE, kn=None, vn=None,
             wl=1, wc=64, scores=ONE, ld=128 + 64, out=ONE, ws=ONE, split=1, T=128, BH=4, groups=1, sqrt_d=8.0, extra=None, mask=None,
             mstride=0, mheads=0, flags=0, head_dim=128, lse=ONE)
    a.update(kw)
    return a


WINDOWLESS = dict(kw=None, vw=None, kn=None, vn=None, wl=0, wc=0, extra=None, T=256, ld=256)


def _lse_hd(L, a):
    return L.mustafar_decode_attention_lse_hd(None, a["k_bmp"], a["k_nz"], a["k_idx"], a["k_off"], a["v_bmp"], a["v_nz"], a["v_idx"], a["v_off"],
                                              a["q"], a["kw"], a["vw"], a["kn"], a["vn"], a["wl"], a["wc"], a["scores"], a["ld"], a["out"],
                                              a["ws"], a["split"], a["T"], a["BH"], a["groups"], ctypes.c_float(a["sqrt_d"]), a["extra"],
                                              a["mask"], a["mstride"], a["mheads"], a["flags"], a["head_dim"], a["lse"])


def _plain_hd(L, a):
    return L.mustafar_decode_attention_hd(None, a["k_bmp"], a["k_nz"], a["k_idx"], a["k_off"], a["v_bmp"], a["v_nz"], a["v_idx"], a["v_off"],
                                          a["q"], a["kw"], a["vw"], a["kn"], a["vn"], a["wl"], a["wc"], a["scores"], a["ld"], a["out"],
                                          a["ws"], a["split"], a["T"], a["BH"], a["groups"], ctypes.c_float(a["sqrt_d"]), a["extra"],
                                          a["mask"], a["mstride"], a["mheads"], a["flags"], a["head_dim"])


def _ext_lse_hd(L, a, T_base):
    from mustafar_amd import _lib as lib
    kv = lib.CacheView(a["k_bmp"], a["k_nz"], a["k_idx"], a["k_off"], 0, 0, 0)
    vv = lib.CacheView(a["v_bmp"], a["v_nz"], a["v_idx"], a["v_off"], 0, 0, 0)
    return L.mustafar_decode_attention_extents_lse_hd(None, ctypes.byref(kv), ctypes.byref(vv), T_base, None, None, a["q"], a["kw"], a["vw"],
                                                      a["kn"], a["vn"], a["wl"], a["wc"], a["scores"], a["ld"], a["out"], a["ws"], a["split"],
                                                      a["T"], a["BH"], a["groups"], ctypes.c_float(a["sqrt_d"]), a["extra"], a["mask"],
                                                      a["mstride"], a["mheads"], a["flags"], None, a["head_dim"], a["lse"])


@pytest.mark.parametrize("bad", [
    dict(T=0, ld=64),                      # no compressed token: the two-launch form
    dict(ld=128 + 64 + 8),                 # ld_scores % 32 != 0: the two-launch form
    dict(flags=1 << 4),                    # MUSTAFAR_FLAG_TWO_LAUNCH
    dict(flags=(1 << 4) | 3),
], ids=["T0", "ld", "two_launch", "two_launch_dot2"])
def test_an_lse_is_refused_where_two_launches_would_run(bad):
    """D = 128 with lse != NULL: MUSTAFAR_EINVAL before any launch (every other argument is valid)."""
    assert _lse_hd(_lib(), _args(**bad)) == 1


def test_an_lse_is_refused_under_a_process_default_of_two_launches():
    L = _lib()
    old = L.mustafar_get_onepass()
    try:
        assert L.mustafar_set_onepass(0) == 0
        assert _lse_hd(L, _args()) == 1
    finally:
        L.mustafar_set_onepass(old)


@pytest.mark.parametrize("head_dim", [64, 128])
@pytest.mark.parametrize("mix", [
    dict(kw=ONE), dict(vw=ONE), dict(kn=ONE), dict(vn=ONE), dict(extra=ONE),   # a window pointer with lengths of zero
    dict(wc=64, ld=256 + 64),                                                  # a capacity without rows or buffers
    dict(wc=64, ld=256 + 64, kw=ONE, vw=ONE),                                  # buffers and capacity, no row
    dict(wl=1),                                                                # a row without buffers
    dict(T=0, ld=64),                                                          # nothing to attend to
    dict(ld=224),                                                              # ld_scores < T
], ids=["kw", "vw", "kn", "vn", "extra", "cap", "cap+buffers", "len", "T0", "ld"])
def test_mixed_window_less_arguments_are_refused(head_dim, mix):
    L = _lib()
    a = _args(head_dim=head_dim, **{**WINDOWLESS, **mix})
    assert _lse_hd(L, a) == 1
    if a["T"]:   # the extents form over the base views alone (T == T_base)
        assert _ext_lse_hd(L, a, a["T"]) == 1


@pytest.mark.parametrize("head_dim", [64, 128])
def test_the_old_entry_points_keep_rejecting_a_call_without_a_window(head_dim):
    a = _args(head_dim=head_dim, **WINDOWLESS)
    assert _plain_hd(_lib(), a) == 1


def _merge(L, **kw):
    a = dict(outs=1 << 20, ostride=4 * 128, lses=2 << 20, lstride=4, n=2, BH=4, D=128, out=3 << 20, lse=None)
    a.update(kw)
    return L.mustafar_merge_attention_states(None, a["outs"], a["ostride"], a["lses"], a["lstride"], a["n"], a["BH"], a["D"], a["out"], a["lse"])


@pytest.mark.parametrize("bad", [
    dict(n=0), dict(n=65), dict(n=-1), dict(D=96), dict(D=0), dict(BH=0),
    dict(out=1 << 20),                                # the first part
    dict(out=(1 << 20) + 2 * 4 * 128),                # the second part
    dict(out=(1 << 20) + 2 * (2 * 4 * 128 - 1)),      # the last half of the last part
    dict(out=(1 << 20) - 2),                          # ends one half inside the first part
    dict(lse=2 << 20),                                # lse_out inside the LSEs
    dict(outs=None), dict(lses=None), dict(out=None),
    dict(ostride=4 * 128 - 1), dict(lstride=3),       # parts that overlap each other
], ids=["n0", "n65", "n-1", "D96", "D0", "BH0", "out=part0", "out=part1", "out=last_half", "out=before", "lse_inside", "outs0", "lses0", "out0",
        "ostride", "lstride"])
def test_merge_rejects_bad_arguments_without_a_launch(bad):
    assert _merge(_lib(), **bad) == 1


# ---- the claims behind the exact GPU tests --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dd", [64, 128])
def test_needle_constants_make_the_lse_exact(Dd):
    """fp32 / fp16 numpy at both head dims' needle constants.  A needle's e is exactly 1 and log(1) == 0, so a row's LSE is its needle's
    x.  Every other token's e is exactly 0 once it is stored (fp16, what the one-pass forms store) -- at D = 64 already in fp32 --, and
    the fp32 weight of every other slab, and of every other part in a merge, is exactly 0 at D = 64.  At D = 128 the gap is 84.8 and
    exp(-84.8) = 1.4e-37 is still a normal fp32 number: there the weight is not zero but is absorbed -- 1 + w l == 1 in fp32 for every
    slab sum l a cache can hold, and v + w o == v for every V value -- which is what the exactness rests on (tests/exact_data.py)."""
    f32, f16 = np.float32, np.float16
    assert (xd.A1, xd.A2, xd.QB, xd.SLOT) == (16.0, 8.0, 8.0, 8)
    x1, x2, xo = pu.needle_x(Dd, xd.A1), pu.needle_x(Dd, xd.A2), pu.other_x_max(Dd)
    assert (x1, x2, xo) == ((128.0, 64.0, 8.0) if Dd == 64 else (90.5, 45.25, float(f16(f32(64) * f32(1.0 / np.float64(f32(np.sqrt(128.0))))))))
    assert f32(np.exp(f32(x1) - f32(x1))) == f32(1.0) and f16(f32(1.0)) == f16(1.0)      # a needle's e
    assert f32(np.log(f32(1.0))) == f32(0.0) and f32(x1) + f32(0.0) == f32(x1)           # log(1) == 0: lse == x
    for top in (x1, x2):                                                                 # (x2: the winner once the primaries are masked)
        with np.errstate(under="ignore"):
            e = f32(np.exp(f32(xo) - f32(top)))                                          # the largest e of any other token = weight of any other slab
        assert f16(e) == f16(0.0) and f16(e * f32(2.0 ** 15)) == f16(0.0)                # stored e: zero, the dot2 engine's scale included
        lmax = f32(65536.0)                                                              # more tokens than a slab sums
        if Dd == 64 and top == x1:
            assert e == f32(0.0)                                                         # exactly 0 in fp32
        assert f32(1.0) + e * lmax == f32(1.0)                                           # absorbed by the denominator
        assert f32(2.0 ** -5) + e * lmax * f32(2.0) == f32(2.0 ** -5)                    # ... and by the smallest non-zero V value
        assert f16(e * lmax * f32(2.0)) == f16(0.0)                                      # ... and a zero channel stays zero in fp16
    # merge: a part without a needle has lse <= xo + log(tokens); its weight against a part that holds one
    with np.errstate(under="ignore"):
        w = f32(np.exp(f32(xo) + f32(np.log(f32(65536.0))) - f32(x1)))
    if Dd == 64:
        assert w == f32(0.0)
        assert f32(np.exp(f32(x2) - f32(x1))) != f32(0.0)   # ... but exp(64 - 128) is not: no unmasked secondary needle in another part
    assert f32(1.0) + w == f32(1.0) and f32(2.0 ** -5) + w * f32(2.0) == f32(2.0 ** -5) and f16(w * f32(2.0)) == f16(0.0)
    # two equal needles: e = 1 twice, l = 2, and log(2) is one fp32 number; the merge of two such parts has weights 1 and 1
    assert f32(1.0) + f32(1.0) == f32(2.0) and abs(float(f32(np.log(f32(2.0)))) - np.log(2.0)) <= 2.0 ** -25


def test_merge_weight_of_a_part_200_below_is_exactly_zero():
    with np.errstate(under="ignore"):
        assert np.float32(np.exp(np.float32(-200.0))) == np.float32(0.0)


def test_lse_model_on_needles_and_its_bound_terms():
    """The float64 model of partial_util gives the needle's x on needle data and log(L) on equal scores; its bound is the three terms."""
    import torch
    K, V, q, _ = xd.needle_data(1, 4, 1, 128, np.array([[0, 63, 64, 127]]), seed=3)
    lse, bound = pu.lse_model(q, K, 4)
    assert torch.equal(lse, torch.full((1, 4), 90.5, dtype=torch.float64))
    assert float(bound.max()) < 2.0 ** -21 * 92 + 2.0 ** -10 + 128 * 2.0 ** -25
    K0 = torch.zeros((1, 1, 64, 64), dtype=torch.float16)
    lse, bound = pu.lse_model(torch.ones((1, 2, 1, 64), dtype=torch.float16), K0, 2)
    assert torch.allclose(lse, torch.full((1, 2), np.log(64.0), dtype=torch.float64), rtol=0, atol=1e-12)
    assert torch.allclose(bound, torch.full((1, 2), 2.0 ** -11 + 64 * 2.0 ** -25 / 64 + 2.0 ** -21 * (np.log(64.0) + 1), dtype=torch.float64))


def test_merge_model_cases():
    import torch
    o = torch.tensor([[[1.0, 2.0]], [[3.0, -2.0]]], dtype=torch.float16)            # [2 parts, 1 row, 2]
    out, lse, _ = pu.merge_model(o, torch.tensor([[0.0], [0.0]], dtype=torch.float32))
    assert out.tolist() == [[2.0, 0.0]] and abs(float(lse) - np.log(2.0)) < 1e-15
    out, lse, _ = pu.merge_model(o, torch.tensor([[float("-inf")], [5.0]], dtype=torch.float32))
    assert out.tolist() == [[3.0, -2.0]] and float(lse) == 5.0
    out, lse, _ = pu.merge_model(o, torch.full((2, 1), float("-inf"), dtype=torch.float32))
    assert out.tolist() == [[0.0, 0.0]] and float(lse) == float("-inf")
