"""CPU: device-side lengths in the multi-query decode surface (ABI 115: mustafar_decode_multi_query_lengths) checked without a GPU -- every
C call here fails validation before any launch --, and the Python refusals of decode_multi(step_counter=, t_device=, t_capacity=) on CPU
tensors."""
import ctypes
import os
import re

import pytest
import torch

from tests.test_multi_query_host import ARGS, ONE, VIEW, _hook, _past, _qkv
from tests.test_multi_query_mask_host import GOOD_MASK, MASK_ARGS, _masked

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from mustafar_amd import _lib as lib
    return lib.load()


def test_abi_115_declares_binds_and_exports_the_new_symbol():
    from mustafar_amd import _lib as lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mustafar_hip.h")).read(), flags=re.S)
    syms = set(re.findall(r"^\s*(?:int|int64_t)\s+(\w+)\s*\(", text, flags=re.M))
    raw = ctypes.CDLL(lib.LIB_PATH)
    s = "mustafar_decode_multi_query_lengths"
    assert s in syms and s in lib.SIGNATURES and hasattr(raw, s)
    assert lib.SIGNATURES[s][1][:27] == lib.SIGNATURES["mustafar_decode_multi_query_masked"][1] and len(lib.SIGNATURES[s][1]) == 29
    assert _lib().mustafar_abi_version() == 115


# T = 512 over a base of 256, a window of 5 rows in 288: with a length pointer a mask row reaches T + window_capacity = 800 columns
LONG_MASK = dict(GOOD_MASK, mbs=800, mrs=800)


def _lengths(L, extra=ONE, t_dev=ONE, **kw):
    """One call of the lengths entry point with every argument valid but those in `kw` (tests/test_multi_query_mask_host.py: _masked)."""
    from mustafar_amd import _lib as lib
    a = dict(T=512, T_base=256, Bp=2, groups=4, n_q=2, q=ONE, kw_=ONE, vw=ONE, kn=ONE, vn=ONE, w_len=5, cap=288, out=ONE, lse=ONE, ws=ONE,
             sqrt_d=8.0, D=64, k=VIEW, v=VIEW, k_null=False, v_null=False, kt=ONE, vt=ONE, **LONG_MASK)
    a.update(kw)
    kv, vv = lib.CacheView(*a["k"]), lib.CacheView(*a["v"])
    return L.mustafar_decode_multi_query_lengths(
        None, None if a["k_null"] else ctypes.byref(kv), None if a["v_null"] else ctypes.byref(vv), a["T_base"], a["kt"], a["vt"], a["T"],
        a["Bp"], a["groups"], a["n_q"], a["q"], a["kw_"], a["vw"], a["kn"], a["vn"], a["w_len"], a["cap"], a["out"], a["lse"], a["ws"],
        ctypes.c_float(a["sqrt_d"]), a["D"], a["mask"], a["mbs"], a["mrs"], a["mrows"], a["hpm"], extra, t_dev)


# Each with every other argument valid.  (That the valid set itself passes validation cannot be shown without a launch; it is shown by
# tests/test_gpu_multi_query_lengths.py, whose calls carry these forms.)
LENGTH_ARGS = [dict(T=256, kt=None, vt=None), dict(T=256),                              # T_device with T == T_base: nothing to grow into
               dict(T=0, T_base=0, k_null=True, v_null=True, kt=None, vt=None),
               dict(kt=None), dict(vt=None), dict(kt=None, vt=None),                    # T_device with NULL tables
               dict(extra=ONE + 2), dict(extra=ONE + 1), dict(t_dev=ONE + 2), dict(t_dev=ONE + 3),   # misaligned (4 B) length pointers
               dict(extra=ONE + 2, t_dev=None), dict(t_dev=ONE + 2, extra=None),
               dict(mrs=799), dict(mbs=799), dict(mrs=517, mbs=517),                    # mask strides below T + window_capacity
               dict(mrs=799, t_dev=None), dict(mbs=799, t_dev=None), dict(mrs=799, extra=None), dict(mbs=799, extra=None)]


@pytest.mark.parametrize("bad", LENGTH_ARGS, ids=[",".join(f"{k}{v}" for k, v in b.items()) for b in LENGTH_ARGS])
def test_each_new_length_argument_is_checked_before_any_launch(bad):
    assert _lengths(_lib(), **bad) == 1


@pytest.mark.parametrize("bad", ARGS, ids=[str(i) for i in range(len(ARGS))])
def test_two_null_lengths_refuse_what_the_masked_call_refuses(bad):
    """The argument sets of tests/test_multi_query_host.py through the two-NULL form, with a mask (rows T + window_len apart: the two-NULL form
    keeps the rule of the masked call) and without one, next to the masked call itself; and with both lengths given."""
    L = _lib()
    assert _masked(L, **bad) == 1
    assert _lengths(L, extra=None, t_dev=None, **GOOD_MASK, **bad) == 1
    assert _lengths(L, extra=None, t_dev=None, mask=None, mbs=-5, mrs=-5, mrows=77, hpm=0, **bad) == 1
    assert _lengths(L, **bad) == 1


@pytest.mark.parametrize("bad", MASK_ARGS, ids=[",".join(f"{k}{v}" for k, v in b.items()) for b in MASK_ARGS])
def test_two_null_lengths_refuse_the_masks_the_masked_call_refuses(bad):
    L = _lib()
    assert _masked(L, **bad) == 1
    assert _lengths(L, extra=None, t_dev=None, **dict(GOOD_MASK, **bad)) == 1


# ---- Python refusals, on CPU tensors ------------------------------------------------------------------------------------------------------
def _counter():
    return torch.zeros(1, dtype=torch.int32)


def test_decode_multi_refuses_t_device_without_step_counter():
    attn = _hook(64, 8, 2)
    with pytest.raises(ValueError, match="t_device is for captured graphs and needs step_counter"):
        attn.decode_multi(*_qkv(attn, 3), _past(attn, 40), t_device=_counter(), t_capacity=512)


def test_decode_multi_refuses_t_capacity_without_t_device_and_t_device_without_a_growing_cache():
    attn = _hook(64, 8, 2)
    with pytest.raises(ValueError, match="t_capacity goes with t_device"):
        attn.decode_multi(*_qkv(attn, 3), _past(attn, 40), step_counter=_counter(), t_capacity=512)
    with pytest.raises(ValueError, match="t_device needs an arena cache"):   # nothing compressed: no arena, no extent cache
        attn.decode_multi(*_qkv(attn, 3), _past(attn, 40), step_counter=_counter(), t_device=_counter(), t_capacity=512)
    attn = _hook(64, 8, 2, hd64_extents=True)
    with pytest.raises(ValueError, match="t_device needs an extent cache"):
        attn.decode_multi(*_qkv(attn, 3), _past(attn, 40), step_counter=_counter(), t_device=_counter(), t_capacity=512)


@pytest.mark.parametrize("Hq,n_q", [(8, 17), (2, 65), (16, 9)])
def test_a_replayed_call_is_one_library_call(Hq, n_q):
    """64 // groups tokens at the most with step_counter; the same call without it runs as consecutive calls and gets past this check."""
    attn = _hook(64, Hq, 2)
    with pytest.raises(ValueError, match=f"at most {64 // (Hq // 2)} tokens"):
        attn.decode_multi(*_qkv(attn, n_q), _past(attn, 40), step_counter=_counter())


def test_a_window_below_its_full_capacity_is_refused_under_replay():
    """residual_length 32: the full capacity is 288 rows; a graph keeps the windows' addresses, so nothing may be reallocated."""
    from mustafar_amd.hook import Window
    attn = _hook(64, 8, 2)
    z = torch.zeros((1, 2, 40, 64), dtype=torch.float16)
    for cap in (40, 42, 287):
        k_w, v_w = Window(z, cap), Window(z, cap)
        with pytest.raises(ValueError, match="full capacity of 288 rows"):
            attn.decode_multi(*_qkv(attn, 3), (None, k_w, None, v_w, 0, 40), step_counter=_counter())
        assert k_w.cap == cap and k_w.len == v_w.len == 40          # nothing was reallocated, nothing appended
    k_w, v_w = Window(z, 300), Window(z, 300)
    k_w.len = v_w.len = 299                                          # (a window no trigger rule leaves behind) capacity, but no room for three rows
    with pytest.raises(ValueError, match="room for this call"):
        attn.decode_multi(*_qkv(attn, 3), (None, k_w, None, v_w, 256, 256 + 299), step_counter=_counter())
    assert k_w.cap == 300 and k_w.len == 299


@pytest.mark.parametrize("shape", [(1, 1, 3, 287), (1, 1, 1, 43), (1, 1, 3, 43), (1, 1, 2, 288), (2, 1, 3, 288)])
def test_a_short_mask_is_refused_under_replay(shape):
    """Nothing compressed and a window capacity of 288 rows: a replayed call reads up to 288 columns of each row, whatever the step."""
    attn = _hook(64, 8, 2)
    with pytest.raises(ValueError, match="Attention mask should be of size"):
        attn.decode_multi(*_qkv(attn, 3), _past(attn, 40), step_counter=_counter(), attention_mask=torch.zeros(shape, dtype=torch.float16))


@pytest.mark.parametrize("bad", [torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.float32), torch.zeros(2, dtype=torch.int32),
                                 torch.zeros(1, dtype=torch.int32, device="meta"), 0],
                         ids=["int64", "float", "two", "other-device", "no-tensor"])
def test_the_device_lengths_must_be_one_int32_on_the_querys_device(bad):
    """Their addresses go to the kernels as they are: anything but one int32 on the query's device is refused by name."""
    attn = _hook(64, 8, 2)
    with pytest.raises(ValueError, match="step_counter must be an int32 tensor"):
        attn.decode_multi(*_qkv(attn, 3), _past(attn, 40), step_counter=bad)
    with pytest.raises(ValueError, match="t_device must be an int32 tensor"):
        attn.decode_multi(*_qkv(attn, 3), _past(attn, 40), step_counter=_counter(), t_device=bad, t_capacity=512)


def test_fits_before_trigger_is_public():
    attn = _hook(64, 8, 2)
    assert attn.fits_before_trigger(_past(attn, 284), 6) == 4 and attn.fits_before_trigger(_past(attn, 40), 64) == 64
    assert attn.fits_before_trigger(_past(attn, 287), 4) == 1
