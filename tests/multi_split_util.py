"""Helpers of the several-token segment tests (a plain module of the suite, not a conftest): callers of mustafar_decode_shared_segment_multi
and mustafar_decode_multi_segment, the run shape read off the public workspace sizes, and the float64 models of tests/exact_data.py and
tests/partial_util.py applied to all query tokens of a call at once.

Both entry points take q [.., kv_heads * groups, n_q, D], whose memory is [.., kv_heads, groups * n_q, D]: a call of n_q tokens at `groups`
q heads per kv head is, row for row, a one-token call at G' = groups * n_q q heads per kv head.  Every query token sees the whole of a
frozen segment, so the one-token models and the needle builder of tests/shared_util.py apply as they are with G' for the group count."""
import ctypes
import math

import torch

from tests import exact_data as xd
from tests import partial_util as pu
from tests.hd64_util import DEV, _cache

NAN = float("nan")


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def as_one_token(q):
    """q / out [n, Hkv * groups, n_q, D] -> the same memory as [n, Hkv * groups * n_q, 1, D]; lse [n, H, n_q] -> [n, H * n_q]."""
    if q.dim() == 3:
        return q.reshape(q.shape[0], -1)
    n, H, n_q, Dd = q.shape
    return q.reshape(n, H * n_q, 1, Dd)


def run_shape(ws, heads, R, T, Dd):
    """(slabs, blocks per run, blocks of the last run) from a workspace size of slabs x heads x R x (D + 2) floats."""
    per = heads * R * (Dd + 2) * 4
    assert ws > 0 and ws % per == 0
    slabs, ntb = ws // per, T // 64
    assert 1 <= slabs <= ntb
    bpw = -(-ntb // slabs)
    assert -(-ntb // bpw) == slabs, "the slab count is not ceil(blocks / run length) for any whole run length"
    return slabs, bpw, ntb - (slabs - 1) * bpw


def _view(c):
    from mustafar_amd import _lib
    return _lib.CacheView(c[0].data_ptr(), c[2].data_ptr(), c[1].data_ptr(), c[3].data_ptr(), 0, 0, 0)


class SharedMultiCall:
    """Operands of mustafar_decode_shared_segment_multi over pruned rows Kp / Vp [1, Hkv, T, D] through the package's conversion.  Output
    and LSE rows start as NaN: a row no workgroup writes shows."""

    def __init__(self, pkg, Kp, Vp, groups, n_seqs, n_q):
        L_, comp = pkg
        self.L = L_
        _, Hkv, T, Dd = Kp.shape
        self.Hkv, self.T, self.Dd, self.groups, self.n, self.n_q = Hkv, T, Dd, groups, n_seqs, n_q
        self.kc = _cache(Kp.reshape(Hkv, T, Dd).contiguous(), "key", comp)
        self.vc = _cache(Vp.reshape(Hkv, T, Dd).contiguous(), "value", comp)
        self.kv, self.vv = _view(self.kc), _view(self.vc)
        self.ws_bytes = L_.mustafar_shared_segment_multi_workspace_bytes(T, Hkv, groups, n_seqs, n_q, Dd)
        assert self.ws_bytes > 0
        self.ws = torch.empty((self.ws_bytes,), dtype=torch.uint8, device=DEV)
        self.out = torch.full((n_seqs, Hkv * groups, n_q, Dd), NAN, dtype=torch.float16, device=DEV)
        self.lse = torch.full((n_seqs, Hkv * groups, n_q), NAN, dtype=torch.float32, device=DEV)

    def run_shape(self):
        return run_shape(self.ws_bytes, self.Hkv, self.n * self.groups * self.n_q, self.T, self.Dd)

    def call(self, q, rows=None):
        """rows (s0, s1): the call serves sequences [s0, s1) alone, writing their part of out / lse."""
        s0, s1 = rows or (0, self.n)
        off = s0 * self.Hkv * self.groups * self.n_q
        err = self.L.mustafar_decode_shared_segment_multi(
            torch.cuda.current_stream().cuda_stream, ctypes.byref(self.kv), ctypes.byref(self.vv), self.T, self.Hkv, self.groups, s1 - s0,
            self.n_q, q.data_ptr() + off * self.Dd * 2, self.out.data_ptr() + off * self.Dd * 2, self.lse.data_ptr() + off * 4,
            self.ws.data_ptr(), ctypes.c_float(math.sqrt(self.Dd)), self.Dd)
        assert err == 0
        return self.out, self.lse


class SegmentMultiCall:
    """Operands of mustafar_decode_multi_segment for B' = B x Hkv heads at `groups` q heads per kv head and n_q tokens.  The cache comes
    either as pruned rows Kp / Vp [B, Hkv, T, D] (one view per side, through the package's conversion) or as `views` = what a cache
    object's view_args() returned: (k view, v view, T_base, k table, v table) of T tokens."""

    def __init__(self, pkg, B, Hkv, T, Dd, groups, n_q, Kp=None, Vp=None, views=None):
        L_, comp = pkg
        self.L = L_
        self.B, self.Hkv, self.T, self.Dd, self.groups, self.n_q = B, Hkv, T, Dd, groups, n_q
        if views is None:
            self.kc = _cache(Kp.reshape(B * Hkv, T, Dd).contiguous(), "key", comp)
            self.vc = _cache(Vp.reshape(B * Hkv, T, Dd).contiguous(), "value", comp)
            self.kv, self.vv = _view(self.kc), _view(self.vc)
            views = (ctypes.byref(self.kv), ctypes.byref(self.vv), T, None, None)
        self.views = views
        self.ws_bytes = L_.mustafar_decode_multi_segment_workspace_bytes(T, B * Hkv, groups, n_q, Dd)
        assert self.ws_bytes > 0
        self.ws = torch.empty((self.ws_bytes,), dtype=torch.uint8, device=DEV)
        self.out = torch.full((B, Hkv * groups, n_q, Dd), NAN, dtype=torch.float16, device=DEV)
        self.lse = torch.full((B, Hkv * groups, n_q), NAN, dtype=torch.float32, device=DEV)

    def run_shape(self):
        return run_shape(self.ws_bytes, self.B * self.Hkv, self.groups * self.n_q, self.T, self.Dd)

    def call(self, q, mask=None):
        """mask: None, or fp16 [B, 1, 1 or n_q, T] (any view with unit stride along a row): one plane per sequence."""
        kv, vv, t_base, kt, vt = self.views
        margs = (None, 0, 0, 1, 1)
        if mask is not None:
            assert mask.stride(3) == 1
            margs = (mask.data_ptr(), mask.stride(0), mask.stride(2), mask.shape[2], self.Hkv)
        err = self.L.mustafar_decode_multi_segment(
            torch.cuda.current_stream().cuda_stream, kv, vv, t_base, kt, vt, self.T, self.B * self.Hkv, self.groups, self.n_q, q.data_ptr(),
            self.out.data_ptr(), self.lse.data_ptr(), self.ws.data_ptr(), ctypes.c_float(math.sqrt(self.Dd)), self.Dd, *margs)
        assert err == 0
        return self.out, self.lse


# ---- the models ---------------------------------------------------------------------------------------------------------------------------
def row_mask(mask, Hkv, groups, n_q):
    """An additive mask [B, 1, 1 or n_q, L] -> [B, Hkv * groups * n_q, 1, L]: the row of query token j for each row (kv head, q head, j)."""
    B, _, rows, L = mask.shape
    m = mask[:, 0].expand(B, n_q, L) if rows == 1 else mask[:, 0]
    return m[:, None, None].expand(B, Hkv, groups, n_q, L).reshape(B, Hkv * groups * n_q, 1, L)


def segment_ratios(out, lse, q, Kp, Vp, groups, mask=None):
    """(max |out - hook_model| / bound, max |lse - lse_model| / bound) of a several-token call over a frozen segment Kp / Vp
    [B or 1, Hkv, T, D] (one copy is expanded over the sequences): every query token sees every token of it."""
    n, H, n_q, _ = q.shape
    Hkv = Kp.shape[1]
    Ke, Ve = Kp.expand(n, -1, -1, -1), Vp.expand(n, -1, -1, -1)
    m = None if mask is None else row_mask(mask, Hkv, groups, n_q)
    want, bound = xd.hook_model(as_one_token(q), Ke, Ve, groups * n_q, mask=m)
    r = (as_one_token(out).double() - want).abs() / bound
    r_out = float(r.max()) if torch.isfinite(r).all() else float("inf")
    want_l, bound_l = pu.lse_model(as_one_token(q), Ke, groups * n_q, mask=m)
    return r_out, pu.lse_ratio(as_one_token(lse), want_l, bound_l)


def assert_segment_models(out, lse, q, Kp, Vp, groups, what, mask=None):
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all(), f"{what}: NaN / Inf in the outputs (a row nobody wrote?)"
    r_out, r_lse = segment_ratios(out, lse, q, Kp, Vp, groups, mask)
    print(f"{what}: |out - model| / bound = {r_out:.3f}, |lse - model| / bound = {r_lse:.3f}")
    assert r_out <= 1.0 and r_lse <= 1.0, f"{what}: out {r_out:.3f}, lse {r_lse:.3f}"
