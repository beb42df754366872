"""Helpers of the partial-attention tests (a plain module of the suite, not a conftest): the float64 model of a fused decode call's
log-sum-exp with its derived bound, callers of the two entry points with an LSE (with a window through tests/hd64_util.Step, and
window-less), the float64 model of the merge, and the needle constants both head dims' exact tests rest on."""
import ctypes
import math

import numpy as np
import torch

from tests import exact_data as xd
from tests.hd64_util import DEV, _cache, oracle_prune

NEG = torch.finfo(torch.float16).min


# ---- needle constants: the x a needle's score becomes, as the kernels form it -------------------------------------------------------
def needle_x(Dd, level):
    """x = fp16(fp16(score) * fp32(1 / sqrt d)) of a needle at key level `level` (A1 primary, A2 secondary): score = level * QB * SLOT
    exactly (q is zero outside the slot).  D = 64: 128 and 64; D = 128: 90.5 and 45.25."""
    score = np.float16(level * xd.QB * xd.SLOT)
    inv = np.float32(1.0 / np.float64(np.float32(math.sqrt(Dd))))
    return float(np.float16(np.float32(score) * inv))


def other_x_max(Dd):
    """The largest x of a token that is no needle: |k| <= 1 on the slot, so its score is at most QB * SLOT."""
    return needle_x(Dd, 1.0)


# ---- float64 model of the LSE -----------------------------------------------------------------------------------------------------
def lse_model(q, K, groups, mask=None):
    """(lse, bound), float64 [B, Hq], of a fused decode over pruned-but-dense K [B, Hkv, L, D] (fp16): |kernel - lse| <= bound.

    The candidates for x are formed exactly as tests/exact_data.hook_model forms them: the stored score is fp16(s') for some s' within
    a = 128 * 2^-24 * sum|q k| of the exact s (three candidates), x is the quotient by sqrt(d) or the product with the fp32 reciprocal
    (two each), the mask is added in fp16 and clamped; x_lo / x_hi bracket every x a kernel can form, dx = x_hi - x_lo, and the model's
    own x is the quotient of the nearest rounding.

    lse = m + log l with l = sum_t e_t, e_t = exp(x_t - m).  What separates a kernel's value from the model's:
      * the ambiguity of x: d lse / d x_t = e_t / l, so a token contributes e_t dx_t / l (first order; dx < 2^-5 wherever e counts);
      * e is stored as fp16 by the one-pass forms before it is summed: 2^-11 relative, or the subnormal quantum 2^-25 absolute; a change
        de_t of one e moves log l by de_t / l;
      * the fp32 sums of e (in a workgroup, then over the slabs), the fast exponentials that rescale the slabs, the fp32 log and the final
        addition m + log l: 2^-21 (|lse| + 1) (a few fp32 ulps of the result and of the two terms that form it).
    bound = sum_t (e_t (dx_t + 2^-11) + 2^-25) / l + 2^-21 (|lse| + 1)."""
    B, Hkv, L, Dd = K.shape
    Hq = q.shape[1]
    rs = math.sqrt(Dd)
    inv = torch.tensor(1.0 / rs, dtype=torch.float32, device=K.device)
    lses, bounds = [], []
    for b in range(B):
        qd = q[b].double().reshape(Hkv, groups, Dd)
        Kd = K[b].double()
        s = torch.einsum("kgd,ktd->kgt", qd, Kd)
        acc = 128 * 2.0 ** -24 * torch.einsum("kgd,ktd->kgt", qd.abs(), Kd.abs())
        cands = [(s - acc).half().double(), (s + acc).half().double(), s.half().double()]
        xs = [f(c) for c in cands for f in (lambda c: (c / rs).half().double(), lambda c: (c.float() * inv).half().double())]
        if mask is not None:
            mb = mask[b].to(torch.float16).expand(Hq, 1, L).reshape(Hkv, groups, L)
            xs = [torch.clamp(c.half() + mb, min=NEG).double() for c in xs]
        x = xs[4]
        dx = torch.stack(xs).amax(0) - torch.stack(xs).amin(0)
        m = x.amax(-1, keepdim=True)
        e = torch.exp(x - m)
        l = e.sum(-1, keepdim=True)
        lse = (m + torch.log(l)).squeeze(-1)
        bound = ((e * (dx + 2.0 ** -11) + 2.0 ** -25).sum(-1, keepdim=True) / l).squeeze(-1) + 2.0 ** -21 * (lse.abs() + 1)
        lses.append(lse.reshape(Hq))
        bounds.append(bound.reshape(Hq))
    return torch.stack(lses), torch.stack(bounds)


def lse_ratio(lse, want, bound):
    """max |lse - want| / bound, printed by the callers before they assert (> 1: outside)."""
    r = (lse.double() - want).abs() / bound
    return float(r.max()) if torch.isfinite(r).all() else float("inf")


def pruned_rows(K, V, C, ks=0.7, vs=0.7):
    """K / V with the first C tokens pruned by the oracle's rule: what the cache holds, dense."""
    Kp, Vp = K.clone(), V.clone()
    if C:
        Kp[:, :, :C], Vp[:, :, :C] = oracle_prune(K[:, :, :C], ks), oracle_prune(V[:, :, :C], vs)
    return Kp, Vp


# ---- callers ---------------------------------------------------------------------------------------------------------------------------
def call_lse(st, q, flags=0, lse=True):
    """A tests/hd64_util.Step through mustafar_decode_attention_lse_hd: (out, lse fp32 [B, Hq]) -- lse=False passes NULL."""
    out_lse = torch.full((st.B, st.Hkv * st.groups), float("nan"), dtype=torch.float32, device=DEV)
    fn = lambda *a: st.L.mustafar_decode_attention_lse_hd(*a, st.Dd, out_lse.data_ptr() if lse else None)
    return st.call(q, flags=flags, fn=fn), out_lse


class Segment:
    """A window-less call's operands: pruned rows Kp / Vp [B, Hkv, T, D] through the package's conversion, scratch sized for T alone."""

    def __init__(self, pkg, Kp, Vp, groups):
        L_, comp = pkg
        self.L = L_
        B, Hkv, T, Dd = Kp.shape
        self.B, self.Hkv, self.T, self.Dd, self.groups = B, Hkv, T, Dd, groups
        self.BH = B * Hkv * groups
        self.kc = _cache(Kp.reshape(B * Hkv, T, Dd).contiguous(), "key", comp)
        self.vc = _cache(Vp.reshape(B * Hkv, T, Dd).contiguous(), "value", comp)
        self.ld = (T + 31) // 32 * 32
        self.scores = torch.empty((self.BH, self.ld), dtype=torch.float16, device=DEV)
        self.ws = torch.empty((L_.mustafar_decode_workspace_bytes_hd(T, self.BH, groups, 1, Dd),), dtype=torch.uint8, device=DEV)
        self.out = torch.empty((B, Hkv * groups, 1, Dd), dtype=torch.float16, device=DEV)
        self.lse = torch.full((B, Hkv * groups), float("nan"), dtype=torch.float32, device=DEV)

    def call(self, q, mask=None, flags=0):
        kc, vc = self.kc, self.vc
        p = lambda t: t.data_ptr() if t is not None else None
        err = self.L.mustafar_decode_attention_lse_hd(
            torch.cuda.current_stream().cuda_stream, p(kc[0]), p(kc[2]), p(kc[1]), p(kc[3]), p(vc[0]), p(vc[2]), p(vc[1]), p(vc[3]),
            q.data_ptr(), None, None, None, None, 0, 0, self.scores.data_ptr(), self.ld, self.out.data_ptr(), self.ws.data_ptr(), 1, self.T,
            self.BH, self.groups, ctypes.c_float(math.sqrt(self.Dd)), None, p(mask), mask.shape[-1] if mask is not None else 0,
            self.Hkv * self.groups, flags, self.Dd, self.lse.data_ptr())
        assert err == 0
        return self.out, self.lse


# ---- the merge ---------------------------------------------------------------------------------------------------------------------
def merge_model(outs, lses):
    """float64 merge of parts outs [n, BH, D] (fp16), lses [n, BH] (fp32): (out, lse, bound).  The arithmetic of
    mustafar_merge_attention_states: M = max lse, w = exp(lse - M) (0 for -inf), out = sum w out / sum w, lse = M + log sum w; all parts
    empty: 0 and -inf.  bound = 2^-11 |out| + 2^-25 + 2^-18 sum w |out_i| / sum w: the final fp16 rounding, and the fp32 sums with a fast
    exponential whose arguments are at most ~17 in size where the weight still counts."""
    o, l = outs.double(), lses.double()
    M = l.amax(0)
    w = torch.where(torch.isinf(l) & (l < 0), torch.zeros_like(l), torch.exp(l - torch.where(torch.isinf(M), torch.zeros_like(M), M)))
    ws = w.sum(0)
    safe = torch.where(ws > 0, ws, torch.ones_like(ws))
    out = (w[..., None] * o).sum(0) / safe[..., None]
    lse = torch.where(ws > 0, M + torch.log(safe), torch.full_like(M, float("-inf")))
    bound = 2.0 ** -11 * out.abs() + 2.0 ** -25 + 2.0 ** -18 * (w[..., None] * o.abs()).sum(0) / safe[..., None]
    return out, lse, bound


def call_merge(L_, outs, lses, out_stride=None, lse_stride=None, want_lse=True):
    """mustafar_merge_attention_states over parts laid out `out_stride` halfs / `lse_stride` floats apart (default: packed).
    outs [n, BH, D] fp16, lses [n, BH] fp32 on the device.  Returns (out [BH, D], lse [BH] or None)."""
    n, BH, Dd = outs.shape
    out_stride = out_stride or BH * Dd
    lse_stride = lse_stride or BH
    ob = torch.full((n * out_stride,), float("nan"), dtype=torch.float16, device=DEV)
    lb = torch.full((n * lse_stride,), float("nan"), dtype=torch.float32, device=DEV)
    for i in range(n):
        ob[i * out_stride:i * out_stride + BH * Dd] = outs[i].reshape(-1)
        lb[i * lse_stride:i * lse_stride + BH] = lses[i]
    out = torch.full((BH, Dd), float("nan"), dtype=torch.float16, device=DEV)
    lse = torch.full((BH,), float("nan"), dtype=torch.float32, device=DEV) if want_lse else None
    err = L_.mustafar_merge_attention_states(torch.cuda.current_stream().cuda_stream, ob.data_ptr(), out_stride, lb.data_ptr(), lse_stride,
                                             n, BH, Dd, out.data_ptr(), lse.data_ptr() if want_lse else None)
    assert err == 0
    return out, lse
