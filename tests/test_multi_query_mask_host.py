"""CPU: masks and draft trees in the multi-query decode surface (ABI 114) checked without a GPU -- every C call here fails validation before
any launch --, and the Python refusals of decode_multi(attention_mask=) and accept(keep=) on CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

from tests.test_multi_query_host import ARGS, ONE, VIEW, _hook, _past, _qkv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mustafar_decode_multi_query_masked", "mustafar_window_keep_rows")


def _lib():
    from mustafar_amd import _lib as lib
    return lib.load()


def test_abi_114_declares_binds_and_exports_the_new_symbols():
    from mustafar_amd import _lib as lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mustafar_hip.h")).read(), flags=re.S)
    syms = set(re.findall(r"^\s*(?:int|int64_t)\s+(\w+)\s*\(", text, flags=re.M))
    raw = ctypes.CDLL(lib.LIB_PATH)
    for s in NEW:
        assert s in syms and s in lib.SIGNATURES and hasattr(raw, s), s
    assert _lib().mustafar_abi_version() >= 114


# T + window_len = 512 + 5 = 517 columns; Bp = 2 heads, n_q = 2
GOOD_MASK = dict(mask=ONE + 2, mbs=517, mrs=517, mrows=2, hpm=1)


def _masked(L, unmasked=False, **kw):
    """One call with every argument valid but those in `kw` (tests/test_multi_query_host.py: _call), through the masked entry point -- or,
    `unmasked`, through mustafar_decode_multi_query with the same 22 arguments."""
    from mustafar_amd import _lib as lib
    a = dict(T=512, T_base=256, Bp=2, groups=4, n_q=2, q=ONE, kw_=ONE, vw=ONE, kn=ONE, vn=ONE, w_len=5, cap=288, out=ONE, lse=ONE, ws=ONE,
             sqrt_d=8.0, D=64, k=VIEW, v=VIEW, k_null=False, v_null=False, kt=ONE, vt=ONE, **GOOD_MASK)
    a.update(kw)
    kv, vv = lib.CacheView(*a["k"]), lib.CacheView(*a["v"])
    head = (None, None if a["k_null"] else ctypes.byref(kv), None if a["v_null"] else ctypes.byref(vv), a["T_base"], a["kt"], a["vt"], a["T"],
            a["Bp"], a["groups"], a["n_q"], a["q"], a["kw_"], a["vw"], a["kn"], a["vn"], a["w_len"], a["cap"], a["out"], a["lse"], a["ws"],
            ctypes.c_float(a["sqrt_d"]), a["D"])
    if unmasked:
        return L.mustafar_decode_multi_query(*head)
    return L.mustafar_decode_multi_query_masked(*head, a["mask"], a["mbs"], a["mrs"], a["mrows"], a["hpm"])


# Each with every other argument valid.  (That the valid set itself passes validation cannot be shown without a launch; it is shown by
# tests/test_gpu_multi_query_mask.py, whose calls carry these forms: an odd element offset, mask_rows 1 and n_q, heads_per_mask 1 and kv heads.)
MASK_ARGS = [dict(mask=ONE + 1), dict(mask=ONE + 3),                       # an odd address
             dict(mrows=0), dict(mrows=3), dict(mrows=-1),
             dict(hpm=0), dict(hpm=-1), dict(hpm=3), dict(hpm=4), dict(Bp=6, hpm=4),   # out of range, no divisor of Bp
             dict(mrs=516), dict(mrs=0),                                   # rows closer than T + window_len with mask_rows > 1
             dict(mbs=516), dict(mbs=0),                                   # planes closer than T + window_len with more than one plane
             dict(mbs=-1, hpm=2), dict(mrs=-1, mrows=1, n_q=1, w_len=5)]   # a negative stride, even where the stride is not used


@pytest.mark.parametrize("bad", MASK_ARGS, ids=[",".join(f"{k}{v}" for k, v in b.items()) for b in MASK_ARGS])
def test_each_new_mask_argument_is_checked_before_any_launch(bad):
    assert _masked(_lib(), **bad) == 1


@pytest.mark.parametrize("bad", ARGS, ids=[str(i) for i in range(len(ARGS))])
def test_a_null_mask_is_refused_where_the_unmasked_call_is(bad):
    """mask == NULL and the other four mask arguments nonsense: the refusals of mustafar_decode_multi_query, through both."""
    L = _lib()
    assert _masked(L, unmasked=True, **bad) == 1
    assert _masked(L, mask=None, mbs=-5, mrs=-5, mrows=77, hpm=0, **bad) == 1
    assert _masked(L, **bad) == 1   # and with a valid mask


KEEP_GOOD = dict(kw_=ONE, vw=ONE, Bp=4, hps=2, cap=288, D=64, row0=30, n_rows=8, keep=ONE, n_keep=3)
KEEP_ARGS = [dict(n_keep=0), dict(n_keep=9), dict(n_keep=-1), dict(n_rows=0), dict(n_rows=65, n_keep=1, row0=0), dict(row0=-1),
             dict(row0=281), dict(cap=1025), dict(cap=1088, row0=1030), dict(D=96), dict(D=0), dict(D=256), dict(kw_=None), dict(vw=None),
             dict(kw_=ONE + 8), dict(vw=ONE + 4), dict(keep=None), dict(keep=ONE + 2), dict(keep=ONE + 1), dict(hps=3), dict(hps=0),
             dict(hps=8), dict(Bp=0)]


@pytest.mark.parametrize("bad", KEEP_ARGS, ids=[",".join(f"{k}{v}" for k, v in b.items()) for b in KEEP_ARGS])
def test_window_keep_rows_checks_its_arguments_before_any_launch(bad):
    a = dict(KEEP_GOOD)
    a.update(bad)
    err = _lib().mustafar_window_keep_rows(None, a["kw_"], a["vw"], a["Bp"], a["hps"], a["cap"], a["D"], a["row0"], a["n_rows"], a["keep"],
                                           a["n_keep"])
    assert err == 1


# ---- Python refusals, on CPU tensors ------------------------------------------------------------------------------------------------------
def _mask(shape, dtype=torch.float16):
    return torch.zeros(shape, dtype=dtype)


@pytest.mark.parametrize("shape", [(1, 1, 3, 42), (1, 1, 3, 44), (1, 1, 2, 43), (1, 2, 3, 43), (2, 1, 3, 43), (1, 3, 43), (1, 1, 1, 40)])
def test_decode_multi_refuses_a_mask_of_the_wrong_shape(shape):
    """kv_seq_len 40 and n_q 3: [1, 1, 1 or 3, 43] is the mask."""
    attn = _hook(64, 8, 2)
    with pytest.raises(ValueError, match="Attention mask should be of size"):
        attn.decode_multi(*_qkv(attn, 3), _past(attn, 40), attention_mask=_mask(shape))


def test_decode_multi_refuses_a_mask_of_another_dtype_or_device():
    attn = _hook(64, 8, 2)
    with pytest.raises(RuntimeError, match="float16"):
        attn.decode_multi(*_qkv(attn, 3), _past(attn, 40), attention_mask=_mask((1, 1, 3, 43), torch.float32))
    with pytest.raises(RuntimeError, match="device"):
        attn.decode_multi(*_qkv(attn, 3), _past(attn, 40), attention_mask=_mask((1, 1, 1, 43)).to("meta"))


def test_the_mask_helper_keeps_a_column_slice_and_copies_what_the_call_cannot_address():
    from mustafar_amd.hook import MustafarAttention
    wide = torch.zeros((2, 1, 3, 100), dtype=torch.float16)
    m = MustafarAttention._multi_mask(wide[..., 5:48], 2, 3, 43, wide.device)
    assert m.data_ptr() == wide.data_ptr() + 10 and m.stride() == wide.stride()          # an odd element offset: taken as it is
    m = MustafarAttention._multi_mask(wide[:1, :, :1, :43].expand(2, 1, 3, 43), 2, 3, 43, wide.device)
    assert m.is_contiguous()                                                              # rows / planes on top of each other: copied
    m = MustafarAttention._multi_mask(wide[:, :, :1, 0:86:2], 2, 1, 43, wide.device)
    assert m.shape == (2, 1, 1, 43) and m.stride(3) == 1                                  # no unit stride along a row: copied
    assert MustafarAttention._multi_mask(None, 2, 3, 43, wide.device) is None


def _closed(attn, n_q=7, bsz=2):
    k_c, k_w, v_c, v_w, C, L = attn.to_fused(_past(attn, 40, bsz=bsz))
    k_w.len = v_w.len = 40 + n_q          # what decode_multi leaves behind
    return (k_c, k_w, v_c, v_w, C, L + n_q)


def test_accept_refuses_keep_with_rejected_and_keep_without_n_q():
    attn = _hook(64, 8, 2)
    past = _closed(attn)
    keep = torch.tensor([[0, 1, 3], [0, 2, 6]])
    with pytest.raises(ValueError, match="rejected"):
        attn.accept(past, rejected=1, keep=keep, n_q=7)
    with pytest.raises(ValueError, match="n_q"):
        attn.accept(past, keep=keep)
    assert past[1].len == past[3].len == 47 and past[5] == 47


@pytest.mark.parametrize("keep", [torch.zeros((3, 2), dtype=torch.int64),       # another batch size
                                  torch.zeros((2,), dtype=torch.int64), torch.zeros((2, 1, 2), dtype=torch.int32),
                                  torch.zeros((2, 0), dtype=torch.int64), torch.zeros((2, 8), dtype=torch.int64),   # n_keep outside 1..n_q
                                  torch.zeros((2, 3), dtype=torch.float32), torch.zeros((2, 3), dtype=torch.bool), [[0, 1], [0, 2]]],
                         ids=["batch", "1d", "3d", "empty", "long", "float", "bool", "list"])
def test_accept_refuses_a_keep_of_the_wrong_shape_or_kind(keep):
    attn = _hook(64, 8, 2)
    past = _closed(attn)
    with pytest.raises(ValueError, match="keep must be an integer tensor"):
        attn.accept(past, keep=keep, n_q=7)
    assert past[1].len == past[3].len == 47


@pytest.mark.parametrize("n_q", [0, 48, 65])
def test_accept_refuses_an_n_q_the_windows_do_not_hold(n_q):
    attn = _hook(64, 8, 2)
    past = _closed(attn)
    with pytest.raises(ValueError, match="n_q must be in"):
        attn.accept(past, keep=torch.zeros((2, 1), dtype=torch.int64), n_q=n_q)
