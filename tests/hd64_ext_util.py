"""Helpers of the head_dim-64 extent tests: the new trigger driven through the C ABI on window buffers, an ExtentCache64 built from
given tokens (base by the package's conversion of oracle-pruned rows, extents by the new trigger), and the operands of a
mustafar_decode_attention_extents_hd call.  A plain module of the suite (tests/hd64_util.py is reused unchanged)."""
import ctypes
import math

import numpy as np
import torch

from oracle import oracle as orc
from tests.hd64_util import DEV, D, _cache, oracle_prune

SENTINEL = 0x7BCD   # an fp16 bit pattern no test data holds (51 616.0): "this byte was not written"


def kth(s):
    return max(1, int(s * D))


class Trigger:
    """One layer's operands of mustafar_trigger_compress_batch_hd: window buffers [B', cap, 64] with the 256 rows at the front, an
    empty extent per side with regions of `region` halfs filled with SENTINEL, head totals and the flag."""

    def __init__(self, Kw, Vw, cap=320, region=None, k_region=None, v_region=None):
        from mustafar_amd import _lib
        Bp = Kw.shape[0]
        assert Kw.shape == (Bp, 256, D) and Vw.shape == Kw.shape
        self.Bp, self.cap = Bp, cap
        self.kw = torch.zeros((Bp, cap, D), dtype=torch.float16, device=DEV)
        self.vw = torch.zeros_like(self.kw)
        self.kw[:, :256], self.vw[:, :256] = Kw, Vw
        self.reg = {"k": k_region or region or 256 * D, "v": v_region or region or 256 * D}
        self.t = {}
        for s in "kv":
            r = self.reg[s]
            assert r % 8 == 0
            self.t[s] = dict(bmp=torch.full((Bp, 256), -1, dtype=torch.int64, device=DEV),
                             idx=torch.full((Bp, 257), -1, dtype=torch.int32, device=DEV),
                             off=torch.full((Bp,), -1, dtype=torch.int32, device=DEV),
                             nz=torch.full((Bp, r), SENTINEL, dtype=torch.int16, device=DEV),
                             tot=torch.full((Bp,), -1, dtype=torch.int64, device=DEV))
        self.flag = torch.zeros((1,), dtype=torch.int32, device=DEV)
        self.slots = torch.zeros((2, ctypes.sizeof(_lib.CacheView)), dtype=torch.uint8, device=DEV)

    def view(self, s):
        from mustafar_amd import _lib
        t = self.t[s]
        return _lib.CacheView(t["bmp"].data_ptr(), t["nz"].data_ptr(), t["idx"].data_ptr(), t["off"].data_ptr(), 256, 257, self.reg[s] // 8)

    def fill(self, it):
        it.k_window, it.v_window = self.kw.data_ptr(), self.vw.data_ptr()
        it.k_dst, it.v_dst = self.view("k"), self.view("v")
        it.k_table_slot, it.v_table_slot = self.slots[0].data_ptr(), self.slots[1].data_ptr()
        it.k_head_total, it.v_head_total = self.t["k"]["tot"].data_ptr(), self.t["v"]["tot"].data_ptr()
        it.overflow_flag = self.flag.data_ptr()

    def result(self, s):
        """(bmp, idx, totals, nz) as numpy; nz int16 [B', region]."""
        t = self.t[s]
        return t["bmp"].cpu().numpy(), t["idx"].cpu().numpy(), t["tot"].cpu().numpy(), t["nz"].cpu().numpy()


def run_triggers(L_, trigs, kth_k, kth_v, batched=True):
    from mustafar_amd import _lib
    n = len(trigs)
    st = torch.cuda.current_stream().cuda_stream
    items = (_lib.TriggerItem * n)()
    for i, t in enumerate(trigs):
        t.fill(items[i])
    hs = trigs[0].cap * D
    kr, vr = trigs[0].reg["k"], trigs[0].reg["v"]
    if batched:
        assert L_.mustafar_trigger_compress_batch_hd(st, n, items, hs, trigs[0].Bp, 256, D, kth_k, kth_v, kr, vr, None) == 0
    else:
        for i in range(n):
            one = (_lib.TriggerItem * 1)(items[i])
            assert L_.mustafar_trigger_compress_batch_hd(st, 1, one, hs, trigs[0].Bp, 256, D, kth_k, kth_v, kr, vr, None) == 0
    torch.cuda.synchronize()


def oracle_extent(x, s, which, pruned=False):
    """Oracle prune + compress of rows [B', 256, 64] (numpy fp16): (bmp, idx, [streams as uint16])."""
    xp = x if pruned else orc.prune_magnitude(x, s)
    conv = orc.convert_key_batched if which == "k" else orc.convert_value_batched
    bmp, idx, nzs = conv(np.ascontiguousarray(xp))
    return bmp, idx, [np.asarray(z).view(np.uint16) for z in nzs]


def assert_extent_equals_oracle(trig, s, want, skip_stream=()):
    """Bit-exact: bitmaps, offsets, totals, every head's stream (heads in skip_stream: region untouched instead); nothing behind a
    head's stream is written."""
    bmp, idx, tot, nz = trig.result(s)
    obmp, oidx, onz = want
    assert np.array_equal(bmp, obmp), f"{s}: bitmaps"
    assert np.array_equal(idx, oidx), f"{s}: offsets"
    assert np.array_equal(tot, 2 * oidx[:, -1].astype(np.int64)), f"{s}: head totals"
    assert np.array_equal(trig.t[s]["off"].cpu().numpy(), np.arange(trig.Bp) * (trig.reg[s] // 8)), f"{s}: nz_offset"
    u = nz.view(np.uint16)
    for h in range(trig.Bp):
        n = len(onz[h])
        if h in skip_stream:
            assert (u[h] == SENTINEL).all(), f"{s}: head {h} overflowed and must stay untouched"
            continue
        assert np.array_equal(u[h, :n], onz[h]), f"{s}: stream of head {h}"
        assert (u[h, n:] == SENTINEL).all(), f"{s}: head {h} wrote behind its stream"


class ExtCase:
    """K / V [B, Hkv, n, 64] with T_base + 256 n_ext compressed tokens: the base is the oracle-pruned rows through the package's
    conversion, each extent comes from the NEW trigger on the raw rows (through ExtentCache64.append_extents, all of them or `upto`),
    the window holds the rest.  call_ext(): mustafar_decode_attention_extents_hd; call_plain(): mustafar_decode_attention_hd on
    to_reference()."""

    def __init__(self, pkg, K, V, T_base, n_ext, groups, ks, vs, cap=None, cache_cls=None, listed=None, cap_T=None):
        from mustafar_amd.cache64 import ExtentCache64
        from mustafar_amd.hook import FlatStreams
        L_, comp = pkg
        self.L = L_
        B, Hkv, n, _ = K.shape
        Bp = B * Hkv
        self.B, self.Hkv, self.Bp, self.groups, self.T_base, self.n_ext = B, Hkv, Bp, groups, T_base, n_ext
        self.T = T_base + 256 * n_ext
        self.BH = Bp * groups
        cls = cache_cls or ExtentCache64
        self.Kp = torch.cat([oracle_prune(K[:, :, :self.T], ks)], 2)
        self.Vp = torch.cat([oracle_prune(V[:, :, :self.T], vs)], 2)
        caches = []
        for x, which in ((self.Kp, "key"), (self.Vp, "value")):
            bmp, idx, flat, off = _cache(x[:, :, :T_base].reshape(Bp, T_base, D), which, comp)
            ends = (idx.view(Bp, -1)[:, -1].to(torch.int64) * 2).cumsum(0).tolist()
            per_head = [flat[(ends[h - 1] if h else 0):ends[h]] for h in range(Bp)]
            caches.append(cls([bmp, idx, FlatStreams(per_head, flat), off], which, Bp, T_base))
        self.kc, self.vc = caches
        self.K, self.V, self.ks, self.vs = K, V, ks, vs
        for i in range(n_ext if listed is None else listed):
            self.add_extent(i)
        wl = n - self.T
        self.wl = wl
        self.cap = cap or max(64, (wl + 63) // 64 * 64)
        self.kw = torch.zeros((B, Hkv, self.cap, D), dtype=torch.float16, device=DEV)
        self.vw = torch.zeros_like(self.kw)
        self.kw[:, :, :wl - 1] = K[:, :, self.T:n - 1]
        self.vw[:, :, :wl - 1] = V[:, :, self.T:n - 1]
        self.kn, self.vn = K[:, :, n - 1].contiguous(), V[:, :, n - 1].contiguous()
        self.cap_T = cap_T or self.T
        self.ld = (self.cap_T + self.cap + 31) // 32 * 32
        self.scores = torch.empty((self.BH, self.ld), dtype=torch.float16, device=DEV)
        self.ws = torch.empty((L_.mustafar_decode_workspace_bytes_hd(self.cap_T, self.BH, groups, 1, D),), dtype=torch.uint8, device=DEV)
        self.out = torch.empty((B, Hkv * groups, 1, D), dtype=torch.float16, device=DEV)

    def add_extent(self, i):
        from mustafar_amd.cache64 import ExtentCache64
        t0 = self.T_base + 256 * i
        kb = torch.zeros((self.B, self.Hkv, 288, D), dtype=torch.float16, device=DEV)
        vb = torch.zeros_like(kb)
        kb[:, :, :256], vb[:, :, :256] = self.K[:, :, t0:t0 + 256], self.V[:, :, t0:t0 + 256]
        ExtentCache64.append_extents([(self.kc, self.vc)], [(kb, vb)], kth(self.ks), kth(self.vs), 256)

    def _tail(self, q, T, wl, extra, mask, mask_stride):
        p = lambda t: t.data_ptr() if t is not None else None
        return [q.data_ptr(), self.kw.data_ptr(), self.vw.data_ptr(), p(self.kn), p(self.vn), wl, self.cap, self.scores.data_ptr(), self.ld,
                self.out.data_ptr(), self.ws.data_ptr(), 1, T, self.BH, self.groups, ctypes.c_float(math.sqrt(D)), p(extra), p(mask),
                mask_stride, self.Hkv * self.groups, 0]

    def call_ext(self, q, t_device=None, extra=None, mask=None, wl=None, v_table=None):
        st = torch.cuda.current_stream().cuda_stream
        tail = self._tail(q, self.cap_T, self.wl if wl is None else wl, extra, mask, mask.shape[-1] if mask is not None else 0)
        err = self.L.mustafar_decode_attention_extents_hd(st, self.kc.view_ptr(), self.vc.view_ptr(), self.T_base, self.kc.table.data_ptr(),
                                                          (v_table if v_table is not None else self.vc.table).data_ptr(), *tail,
                                                          t_device.data_ptr() if t_device is not None else None, D)
        assert err == 0
        return self.out

    def call_plain(self, q, mask=None):
        kb, ki, kz, ko = self.kc.to_reference()
        vb, vi, vz, vo = self.vc.to_reference()
        self._keep = (kb, ki, kz.flat, ko, vb, vi, vz.flat, vo)
        st = torch.cuda.current_stream().cuda_stream
        tail = self._tail(q, self.T, self.wl, None, mask, mask.shape[-1] if mask is not None else 0)
        err = self.L.mustafar_decode_attention_hd(st, kb.data_ptr(), kz.flat.data_ptr(), ki.data_ptr(), ko.data_ptr(), vb.data_ptr(),
                                                  vz.flat.data_ptr(), vi.data_ptr(), vo.data_ptr(), *tail, D)
        assert err == 0
        return self.out


def same_reference(a, b):
    """Two reference-layout caches [bitmaps, idxs, streams, nz_offset] hold the same bits."""
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3]) and len(a[2]) == len(b[2]) and \
        all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(a[2], b[2]))
