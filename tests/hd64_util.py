"""Helpers of the head_dim-64 GPU tests (a plain module of the suite, not a conftest): the operands of one
mustafar_decode_attention_hd call, random and needle data at D = 64, mask buffers of any row geometry, and the run shape
(compressed slabs S1, blocks per workgroup bpw) a launch gets, read off the public workspace size."""
import ctypes
import math

import numpy as np
import torch

from oracle import oracle as orc

DEV = torch.device("cuda:0")
D = 64
S = 0.7
NEG = torch.finfo(torch.float16).min
# name -> (B' = batch x kv heads, T, bpw, S1, blocks of the last run): the run shapes the multi-block tests need (each asserts its own
# before it launches; tests/test_headdim64_host.py checks the table without a GPU).  bpw2_full / bpw8: DESIGN.md 4.7's 8k / 32k bench shapes.
RUN_SHAPES = {
    "bpw2_full": (64, 7936, 2, 62, 2),
    "bpw2": (64, 8000, 2, 63, 1),
    "bpw3": (64, 10240, 3, 54, 1),
    "bpw8": (64, 32512, 8, 64, 4),
    "cap": (1, 64512, 1, 1008, 1),      # the slab limit: 1008 compressed slabs + 16 of a 1024-row window
    "cap+1": (1, 64576, 2, 505, 1),     # the first T behind the cap
    "64k": (1, 65536, 2, 512, 2),
}
WINDOW_SLABS = 16     # slabs the workspace reserves for the window: capacity 1024 / 64 rows per window workgroup


def run_shape(L_, T, BH, groups):
    """(S1, bpw) of a D = 64 decode over T compressed tokens: S1 = compressed slabs per row, from the public workspace size
    ((S1 + 16) slabs of 66 floats per row), bpw = ceil(ntb / S1) 64-token blocks per one-wave workgroup."""
    ws = L_.mustafar_decode_workspace_bytes_hd(T, BH, groups, 1, D)
    assert ws > 0 and ws % (BH * 66 * 4) == 0
    S1 = ws // (BH * 66 * 4) - WINDOW_SLABS
    ntb = T // 64
    if ntb == 0:
        assert S1 == 0
        return 0, 1
    assert 1 <= S1 <= ntb
    bpw = -(-ntb // S1)
    assert -(-ntb // bpw) == S1, "the slab count is not ceil(ntb / bpw) for any whole bpw"
    return S1, bpw


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cache(x, which, comp):
    from mustafar_amd.hook import nz_offset_from_idxs
    conv = comp.convert_key_batched if which == "key" else comp.convert_value_batched
    bmp, idx, nzs = conv(x)
    return bmp, idx, torch.cat(nzs), nz_offset_from_idxs(idx, x.shape[0])


def oracle_prune(x, sparsity, threads=8):
    """The oracle's magnitude prune of a tensor [..., D].  The rule is per row, so large inputs go through the oracle in slices of rows
    on a few threads (the C call releases the interpreter lock): the same bits as one call."""
    h = np.ascontiguousarray(x.cpu().numpy())
    rows = h.reshape(-1, h.shape[-1])
    if rows.shape[0] < (1 << 16):
        return torch.from_numpy(orc.prune_magnitude(h, sparsity)).to(x.device)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda r: orc.prune_magnitude(r, sparsity), np.array_split(rows, 4 * threads)))
    return torch.from_numpy(np.concatenate(parts).reshape(h.shape)).to(x.device)


class Step:
    """Operands of one mustafar_decode_attention_hd call for K / V [B, Hkv, L, D] (the step's new row last), C of them compressed:
    the compressed part is the oracle-pruned rows (K at `ks`, V at `vs`) through the package's conversion, the window holds rows
    [C, L - 1).  stored_new: the newest row is already in the windows and k_new = v_new = NULL are passed.  mask: an fp16 tensor whose
    last dimension is a row's columns; its base is mask.data_ptr(), `mask_stride` (default: the column count) and `mask_heads` (default:
    the q heads) are passed as given.  pruned: (Kp, Vp) = the first C rows already pruned by the oracle (large shapes prune once)."""

    def __init__(self, pkg, K, V, C, groups, cap=None, mask=None, extra=None, ks=S, vs=S, stored_new=False, mask_stride=None,
                 mask_heads=None, pruned=None):
        L_, comp = pkg
        self.L = L_
        B, Hkv, n, Dd = K.shape
        self.B, self.Hkv, self.groups, self.C, self.Dd = B, Hkv, groups, C, Dd
        self.BH = B * Hkv * groups
        wl = n - C
        self.cap = cap or max(64, (wl + 63) // 64 * 64)
        self.Kp, self.Vp = pruned if pruned is not None else (oracle_prune(K[:, :, :C], ks), oracle_prune(V[:, :, :C], vs))
        self.kc = _cache(self.Kp.reshape(B * Hkv, C, Dd), "key", comp) if C else None
        self.vc = _cache(self.Vp.reshape(B * Hkv, C, Dd), "value", comp) if C else None
        self.kw = torch.zeros((B, Hkv, self.cap, Dd), dtype=torch.float16, device=DEV)
        self.vw = torch.zeros_like(self.kw)
        stored = wl if stored_new else wl - 1
        self.kw[:, :, :stored] = K[:, :, C:C + stored]
        self.vw[:, :, :stored] = V[:, :, C:C + stored]
        self.kn = None if stored_new else K[:, :, n - 1].contiguous()
        self.vn = None if stored_new else V[:, :, n - 1].contiguous()
        self.wl = wl
        self.ld = (C + self.cap + 31) // 32 * 32
        self.scores = torch.empty((self.BH, self.ld), dtype=torch.float16, device=DEV)
        self.ws = torch.empty((L_.mustafar_decode_workspace_bytes_hd(C, self.BH, groups, 1, Dd),), dtype=torch.uint8, device=DEV)
        self.out = torch.empty((B, Hkv * groups, 1, Dd), dtype=torch.float16, device=DEV)
        self.mask, self.extra = mask, extra
        self.mask_stride = (mask_stride if mask_stride is not None else mask.shape[-1]) if mask is not None else 0
        self.mask_heads = mask_heads if mask_heads is not None else Hkv * groups

    def call(self, q, flags=0, head_dim=None, fn=None):
        p = lambda t: t.data_ptr() if t is not None else None
        kc, vc = self.kc or (None,) * 4, self.vc or (None,) * 4
        args = [torch.cuda.current_stream().cuda_stream, p(kc[0]), p(kc[2]), p(kc[1]), p(kc[3]), p(vc[0]), p(vc[2]), p(vc[1]), p(vc[3]),
                q.data_ptr(), self.kw.data_ptr(), self.vw.data_ptr(), p(self.kn), p(self.vn), self.wl, self.cap,
                self.scores.data_ptr(), self.ld, self.out.data_ptr(), self.ws.data_ptr(), 1, self.C, self.BH, self.groups,
                ctypes.c_float(math.sqrt(self.Dd)), p(self.extra), p(self.mask), self.mask_stride, self.mask_heads, flags]
        if fn is None:
            err = self.L.mustafar_decode_attention_hd(*args, head_dim or self.Dd)
        else:
            err = fn(*args)
        assert err == 0
        return self.out


def _rand(B, Hkv, n, groups, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    K = torch.randn((B, Hkv, n, D), generator=g, device=DEV).half()
    V = torch.randn((B, Hkv, n, D), generator=g, device=DEV).half()
    q = torch.randn((B, Hkv * groups, 1, D), generator=g, device=DEV).half()
    return K, V, q


def _left_pad_mask(B, cols, pads):
    m = torch.zeros((B, 1, 1, cols), dtype=torch.float16, device=DEV)
    for b, p in enumerate(pads):
        m[b, ..., :p] = NEG
    return m


def mask_rows(rows, cols, stride=None, offset=0):
    """[rows, cols] fp16 zeros, a view into a flat buffer: rows `stride` halfs apart (default cols), the first `offset` halfs behind
    the allocation's (256-byte aligned) base -- offset 1 gives a base that is 2-byte aligned only.  The buffer ends with the last
    row's last column: a read beyond a row's columns in the last row leaves the allocation."""
    stride = cols if stride is None else stride
    assert stride >= cols or rows == 1
    flat = torch.zeros((offset + (rows - 1) * stride + cols,), dtype=torch.float16, device=DEV)
    view = flat.as_strided((rows, cols), (stride, 1), offset)
    assert view.data_ptr() == flat.data_ptr() + 2 * offset
    return view


# ---- needles: exactly checkable outputs ----------------------------------------------------------------------------------------------
SLOT, A1, A2, QB = 8, 16.0, 8.0, 8.0


def needle_data_64(B, Hq, Hkv, n, pos, seed, device=None, pos2=None):
    """K, V [B, Hkv, n, 64], q [B, Hq, 1, 64]: q head h attends to token pos[b, h] only (the D = 64 version of tests/exact_data.py).
    Key noise multiples of 1/4 in [-1, 1]; the needle row holds A1 = 16 on the head's slot of 8 channels (8 disjoint slots per kv head),
    q holds QB = 8 there.  Scores: needle 1024 (x = 128), any other <= 64 (x <= 8): exp(-120) is 0 in fp16 and in fp32, so the output is
    the needle's V row (pruned when the token is compressed) exactly; V holds multiples of 2^-5.

    pos [B, Hq] or [B, Hq, k]: k needles of equal score on distinct tokens (k a power of two: the output is the exact mean of their V
    rows).  pos2 [B, Hq] (-1: none): a secondary needle at A2 = 8 (score 512, x = 64: still 56 above every other row), the winner once
    the primary ones are masked.  The eight slot channels tie at the row's top magnitude, and the prune keeps every value at or above
    its threshold, so they survive at every sparsity (at most 63 of 64 pruned); tests/test_headdim64_host.py checks both claims."""
    device = DEV if device is None else device
    g = Hq // Hkv
    assert g <= D // SLOT
    pos = np.asarray(pos, np.int64)
    if pos.ndim == 2:
        pos = pos[..., None]
    k = pos.shape[-1]
    assert pos.shape[:2] == (B, Hq) and k & (k - 1) == 0 and (pos >= 0).all() and (pos < n).all()
    gen = torch.Generator(device=device).manual_seed(seed)
    K = torch.randint(-4, 5, (B, Hkv, n, D), generator=gen, device=device).half() * 0.25
    V = torch.randint(-64, 65, (B, Hkv, n, D), generator=gen, device=device).half() * 2.0 ** -5
    q = torch.zeros((B, Hq, 1, D), dtype=torch.float16, device=device)
    for b in range(B):
        for h in range(Hq):
            ch = slice((h % g) * SLOT, (h % g + 1) * SLOT)
            assert len(set(pos[b, h].tolist())) == k, "a row's equal needles must sit on distinct tokens"
            for t in pos[b, h]:
                K[b, h // g, int(t), ch] = A1
            if pos2 is not None and pos2[b, h] >= 0:
                assert int(pos2[b, h]) not in pos[b, h].tolist()
                K[b, h // g, int(pos2[b, h]), ch] = A2
            q[b, h, 0, ch] = QB
    return K, V, q


def needle_expect_64(V, pos, C, groups, vs=S, pos2=None, masked=None):
    """The exact output [B, Hq, 1, 64] fp16: the (mean of the) V row(s) of each head's winning needle(s), pruned by the oracle's rule
    at `vs` where the token is one of the first C.  masked [B, Hq, n] bool (or None): tokens the mask removes for that head; a head
    whose primary needles are all masked falls to its secondary one.  Computed from V and the oracle's prune alone."""
    B, Hkv, n, _ = V.shape
    pos = np.asarray(pos, np.int64)
    if pos.ndim == 2:
        pos = pos[..., None]
    Vh = V.cpu().numpy()
    want = np.zeros((B, Hkv * groups, 1, D), np.float16)
    for b in range(B):
        for h in range(Hkv * groups):
            win = [int(t) for t in pos[b, h] if masked is None or not masked[b, h, t]]
            if not win:
                assert pos2 is not None and pos2[b, h] >= 0 and not masked[b, h, pos2[b, h]], "no unmasked needle left"
                win = [int(pos2[b, h])]
            assert len(win) & (len(win) - 1) == 0, "a mean over a non-power-of-two count is not exact"
            rows = np.stack([orc.prune_magnitude(Vh[b, h // groups, t][None], vs)[0] if t < C else Vh[b, h // groups, t] for t in win])
            mean = rows.astype(np.float64).mean(0)
            want[b, h, 0] = mean.astype(np.float16)
            assert np.array_equal(want[b, h, 0].astype(np.float64), mean), "the expected mean is not an fp16 number"
    return torch.from_numpy(want).to(V.device)
