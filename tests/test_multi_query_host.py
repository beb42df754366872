"""CPU: the multi-query decode surface (ABI 112) checked without a GPU -- every C call here fails validation before any launch --, the
workspace formula, the Python refusals of decode_multi / accept and the host bookkeeping of accept."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mustafar_decode_multi_query_workspace_bytes", "mustafar_decode_multi_query")
ONE = 16   # a pointer that is never dereferenced (16-byte aligned, so that only the argument under test is wrong)
VIEW = (ONE, ONE, ONE, ONE, 0, 0, 0)


def _lib():
    from mustafar_amd import _lib as lib
    return lib.load()


def test_abi_112_declares_binds_and_exports_the_new_symbols():
    from mustafar_amd import _lib as lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mustafar_hip.h")).read(), flags=re.S)
    syms = set(re.findall(r"^\s*(?:int|int64_t)\s+(\w+)\s*\(", text, flags=re.M))
    raw = ctypes.CDLL(lib.LIB_PATH)
    for s in NEW:
        assert s in syms and s in lib.SIGNATURES and hasattr(raw, s), s
    assert _lib().mustafar_abi_version() >= 112


def _call(L, **kw):
    """One call with every argument valid but those in `kw`: (error, workspace bytes of the same shape)."""
    from mustafar_amd import _lib as lib
    a = dict(T=512, T_base=256, Bp=2, groups=4, n_q=2, q=ONE, kw_=ONE, vw=ONE, kn=ONE, vn=ONE, w_len=5, cap=288, out=ONE, lse=ONE, ws=ONE,
             sqrt_d=8.0, D=64, k=VIEW, v=VIEW, k_null=False, v_null=False, kt=ONE, vt=ONE)
    a.update(kw)
    kv, vv = lib.CacheView(*a["k"]), lib.CacheView(*a["v"])
    err = L.mustafar_decode_multi_query(None, None if a["k_null"] else ctypes.byref(kv), None if a["v_null"] else ctypes.byref(vv), a["T_base"],
                                        a["kt"], a["vt"], a["T"], a["Bp"], a["groups"], a["n_q"], a["q"], a["kw_"], a["vw"], a["kn"], a["vn"],
                                        a["w_len"], a["cap"], a["out"], a["lse"], a["ws"], ctypes.c_float(a["sqrt_d"]), a["D"])
    return err, L.mustafar_decode_multi_query_workspace_bytes(a["T"], a["cap"], a["Bp"], a["groups"], a["n_q"], a["D"])


SHAPES = [dict(n_q=0), dict(n_q=-1), dict(n_q=17, w_len=17), dict(groups=1, n_q=65, w_len=65), dict(groups=0), dict(groups=9, n_q=1), dict(D=96),
          dict(D=0), dict(D=256), dict(Bp=0), dict(Bp=65536), dict(T=-64, T_base=0), dict(T=96, T_base=96), dict(T=544), dict(cap=1025),
          dict(cap=1088, w_len=1030)]


@pytest.mark.parametrize("bad", SHAPES, ids=[",".join(f"{k}{v}" for k, v in b.items()) for b in SHAPES])
def test_unsupported_shapes_are_refused_and_need_no_workspace(bad):
    err, ws = _call(_lib(), **bad)
    assert err == 1 and ws == 0


ARGS = [dict(T_base=64), dict(T_base=128, T=384),          # T_base % 256 with extents behind it
        dict(T=576, T_base=256),                           # (T - T_base) % 256 (T % 64 == 0)
        dict(T_base=256, T=256 + 256 * 513),               # more than 512 entries
        dict(kt=None), dict(vt=None),                      # tables NULL with T > T_base
        dict(T_base=0), dict(T_base=768), dict(T_base=-256),
        dict(w_len=1), dict(w_len=289), dict(cap=1),       # window_len < n_q, > capacity
        dict(kn=None), dict(vn=None),                      # exactly one of the new rows
        dict(q=None), dict(out=None), dict(kw_=None), dict(vw=None), dict(ws=None), dict(lse=None),
        dict(q=ONE + 8), dict(out=ONE + 2), dict(kw_=ONE + 4), dict(vw=ONE + 8), dict(kn=ONE + 8), dict(vn=ONE + 2), dict(ws=ONE + 4),
        dict(lse=ONE + 2),
        dict(k_null=True), dict(v_null=True), dict(k=(None, ONE, ONE, ONE, 0, 0, 0)), dict(v=(ONE, None, ONE, ONE, 0, 0, 0)),
        dict(k=(ONE, ONE, None, ONE, 0, 0, 0)), dict(v=(ONE, ONE + 8, ONE, ONE, 0, 0, 0)),
        dict(k=(ONE, ONE, ONE, None, 0, 0, 0)),            # no nz_offset and no stream stride
        dict(k=(ONE, ONE, ONE, ONE, 255, 0, 0)),           # bitmap rows shorter than the base's tokens (256 tiles at D = 64)
        dict(v=(ONE, ONE, ONE, ONE, 0, 256, 0)),           # offset rows shorter than the tokens + 1
        dict(v=(ONE, ONE, ONE, ONE, 0, 0, -1)), dict(sqrt_d=0.0)]


@pytest.mark.parametrize("bad", ARGS, ids=[str(i) for i in range(len(ARGS))])
def test_bad_arguments_are_refused_before_any_launch(bad):
    err, _ = _call(_lib(), **bad)
    assert err == 1


@pytest.mark.parametrize("Dd", [64, 128])
def test_workspace_equals_the_formula(Dd):
    """(ceil(T / 64 / bpw) + ceil(capacity / 64)) x Bp x R x (D + 2) x 4, bpw = ceil(8 R (D + 2) / (88 D)): the shared-segment rule."""
    L = _lib()
    for groups, n_q in [(1, 1), (4, 1), (4, 8), (3, 3), (8, 8), (1, 64)]:
        R = groups * n_q
        bpw = -(-8 * R * (Dd + 2) // (88 * Dd))
        for T in (0, 64, 576, 7936):
            for cap in (64, 288, 1024):
                for Bp in (1, 3):
                    want = (-(-(T // 64) // bpw) + -(-cap // 64)) * Bp * R * (Dd + 2) * 4
                    assert L.mustafar_decode_multi_query_workspace_bytes(T, cap, Bp, groups, n_q, Dd) == want
            if T:   # the compressed part alone is the shared call's workspace with kv_heads = Bp
                assert L.mustafar_decode_multi_query_workspace_bytes(T, 64, 2, groups, n_q, Dd) - 2 * R * (Dd + 2) * 4 == \
                    L.mustafar_shared_segment_workspace_bytes(T, 2, groups, n_q, Dd)


# ---- Python refusals and the bookkeeping of accept, on CPU tensors ------------------------------------------------------------------------
def _hook(Dd, Hq, Hkv, **kw):
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    kw.setdefault("api", "fused")
    return MustafarAttention(MustafarConfig(num_attention_heads=Hq, num_key_value_heads=Hkv, head_dim=Dd, **kw))


def _past(attn, w, C=0, bsz=1):
    """A past with CPU tensors: nothing compressed (or a claimed C with no cache behind it: never read here), a window of w rows."""
    z = torch.zeros((bsz, attn.num_key_value_heads, w, attn.head_dim), dtype=torch.float16)
    return (None, z, None, z.clone(), C, C + w)


def _qkv(attn, n_q, bsz=1):
    q = torch.zeros((bsz, attn.num_heads, n_q, attn.head_dim), dtype=torch.float16)
    kv = torch.zeros((bsz, attn.num_key_value_heads, n_q, attn.head_dim), dtype=torch.float16)
    return q, kv, kv.clone()


def test_decode_multi_needs_the_fused_api():
    attn = _hook(128, 8, 2, api="native")
    with pytest.raises(ValueError, match="fused"):
        attn.decode_multi(*_qkv(attn, 2), _past(attn, 40))


def test_decode_multi_refuses_more_than_8_q_heads_per_kv_head():
    attn = _hook(64, 32, 2)
    with pytest.raises(ValueError, match="1 to 8 q heads"):
        attn.decode_multi(*_qkv(attn, 2), _past(attn, 40))


def test_decode_multi_refuses_a_mismatched_shape():
    attn = _hook(64, 8, 2)
    q, k, v = _qkv(attn, 3)
    with pytest.raises(ValueError, match="decode_multi: q"):
        attn.decode_multi(q, k[:, :, :2], v, _past(attn, 40))


@pytest.mark.parametrize("w,n_q,fits", [(284, 6, 4), (287, 2, 1), (280, 16, 8), (286, 3, 2)])
def test_a_call_that_steps_over_a_trigger_point_is_refused_and_names_what_fits(w, n_q, fits):
    """residual_length 32, nothing compressed: the row that brings the window to 288 = 32 + 256 rows is a trigger point; it may only be
    the last row of a call."""
    attn = _hook(64, 8, 2)
    with pytest.raises(ValueError, match=f"at most {fits} fit"):
        attn.decode_multi(*_qkv(attn, n_q), _past(attn, w))
    assert attn._fits_before_trigger(_past(attn, w), fits) == fits        # the call the message names is accepted by the same rule
    assert attn._fits_before_trigger(_past(attn, 40), 64) == 64           # far from a trigger point: everything fits
    assert attn._fits_before_trigger(_past(attn, 40 + 31, C=256), 64) == 64


def test_accept_refuses_a_count_out_of_range_and_a_past_that_is_no_fused_one():
    attn = _hook(64, 8, 2)
    past = attn.to_fused(_past(attn, 40))
    for bad in (-1, 40, 41):
        with pytest.raises(ValueError, match="rejected"):
            attn.accept(past, rejected=bad)
    assert past[1].len == 40 and past[3].len == 40
    with pytest.raises(ValueError, match="decode_multi"):
        attn.accept(_past(attn, 40))


@pytest.mark.parametrize("n_q,rejected", [(6, 0), (6, 1), (6, 5)])
def test_accept_changes_the_host_lengths_only(n_q, rejected):
    """After a call of n_q tokens on a window of 40 rows the windows hold 40 + n_q rows; accept drops `rejected` of them from the lengths
    and kv_seq_len, leaves the buffers as they are and (far from a trigger point) runs nothing."""
    attn = _hook(64, 8, 2)
    k_c, k_w, v_c, v_w, C, L = attn.to_fused(_past(attn, 40))
    k_w.buf[:, :, :40 + n_q] = 1.0
    k_w.len = v_w.len = 40 + n_q          # what decode_multi leaves behind
    before = k_w.buf.clone()
    new = attn.accept((k_c, k_w, v_c, v_w, C, L + n_q), rejected=rejected)
    assert new[1] is k_w and new[3] is v_w and new[0] is None and new[4] == 0
    assert k_w.len == v_w.len == 40 + n_q - rejected and new[5] == 40 + n_q - rejected
    assert torch.equal(k_w.buf.view(torch.int16), before.view(torch.int16))   # (bits: the spare rows are uninitialised)
    again = attn.accept(new, rejected=0, defer_trigger=False)
    assert again[5] == new[5] and again[1].len == k_w.len
