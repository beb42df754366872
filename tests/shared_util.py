"""Helpers of the shared-segment tests (a plain module of the suite, not a conftest): needle data with slots narrow enough that every
row of a kv head has one of its own, a caller of mustafar_decode_shared_segment, the run shape read off the public workspace size, and
the split bound of DESIGN.md 4.9 restated.

A shared call with R = n_seqs x groups rows per kv head is the arithmetic of a batch-1 call with group count R and permuted query rows:
local row r = s * groups + g of kv head k is query row (s, k * groups + g)."""
import ctypes
import math

import numpy as np
import torch

from oracle import oracle as orc
from tests.hd64_util import DEV, _cache

QB = 8.0


# ---- needle constants ----------------------------------------------------------------------------------------------------------------
def slot_width(Dd, R):
    """Channels of a row's slot: the widest power of two, at most 8, that gives each of the R rows (padded to a power of two) its own."""
    rows = 1
    while rows < R:
        rows *= 2
    w = min(8, Dd // rows)
    assert w >= 1, f"{R} rows do not fit {Dd} channels"
    return w


def level(w):
    """Key level of a needle on a slot of w channels: 16 down to 4 channels, 32 on 2, 64 on 1 -- the needle's score stays 512 or 1024."""
    return max(16.0, 64.0 / w)


def needle_x(Dd, w, boost=1):
    """x = fp16(fp16(score) * fp32(1 / sqrt d)), score = boost * level * QB * w exactly (q is zero outside the slot)."""
    inv = np.float32(1.0 / np.float64(np.float32(math.sqrt(Dd))))
    assert boost * level(w) * QB * w <= 2048
    return float(np.float16(np.float32(np.float16(boost * level(w) * QB * w)) * inv))


def other_x_max(Dd, w):
    """|k| <= 1 on the slot of a token that is no needle of the row: its score is at most QB * w."""
    inv = np.float32(1.0 / np.float64(np.float32(math.sqrt(Dd))))
    return float(np.float16(np.float32(np.float16(QB * w)) * inv))


def row_of(s, h, groups):
    """Local row of query row (s, h) among the rows of its kv head."""
    return s * groups + h % groups


def edge_positions(T):
    """Token 0, the first and last token of every 64-token block, T - 1."""
    pos = {0, T - 1}
    for b in range(0, T, 64):
        pos.update((b, b + 63))
    return sorted(pos)


def assign_rows(positions, n_seqs, H, rng, T):
    """Spread `positions` over the n_seqs x H rows of one or more calls ([n_seqs, H] int64 each); rows left over get random tokens."""
    rows = n_seqs * H
    calls = []
    for i in range(0, max(len(positions), 1), rows):
        chunk = np.asarray(positions[i:i + rows], np.int64)
        calls.append(np.concatenate([chunk, rng.integers(0, T, size=rows - len(chunk))]).reshape(n_seqs, H))
    return calls


def needle_data(Dd, n_seqs, groups, Hkv, T, pos, seed, k_sparsity=0.7, device="cpu", boost=1):
    """K, V [1, Hkv, T, Dd] (ONE copy) and q [n_seqs, Hkv * groups, 1, Dd]: query row (s, h) attends to token pos[s, h] of kv head
    h // groups only.  Key noise: multiples of 1/4 in [-1, 1]; V: multiples of 2^-5 in [-2, 2].  Row r of a kv head owns channels
    [r w, (r + 1) w).  Asserts the gap (> 39: every other e is 0 in fp16, every other weight is absorbed in fp32) and that the oracle's
    prune keeps each needle's slot.  boost: a power of two the needles' level is multiplied by -- at 2, on slots of 8 channels, every needle's x stands
    more than 88 above every other x, so exp(x - a maximum that missed the needle) overflows fp32.  Returns K, V, q, w."""
    H, R = Hkv * groups, n_seqs * groups
    w = slot_width(Dd, R)
    lv = boost * level(w)
    assert needle_x(Dd, w, boost) - other_x_max(Dd, w) > 39
    pos = np.asarray(pos, np.int64)
    assert pos.shape == (n_seqs, H) and (pos >= 0).all() and (pos < T).all()
    gen = torch.Generator(device=device).manual_seed(seed)
    K = torch.randint(-4, 5, (1, Hkv, T, Dd), generator=gen, device=device).half() * 0.25
    V = torch.randint(-64, 65, (1, Hkv, T, Dd), generator=gen, device=device).half() * 2.0 ** -5
    q = torch.zeros((n_seqs, H, 1, Dd), dtype=torch.float16, device=device)
    for s in range(n_seqs):
        for h in range(H):
            r = row_of(s, h, groups)
            K[0, h // groups, int(pos[s, h]), r * w:(r + 1) * w] = lv
            q[s, h, 0, r * w:(r + 1) * w] = QB
    for s in range(n_seqs):
        for h in range(H):
            r = row_of(s, h, groups)
            kept = orc.prune_magnitude(K[0, h // groups, int(pos[s, h])][None].cpu().numpy(), k_sparsity)[0]
            assert (kept[r * w:(r + 1) * w] == lv).all(), "a needle slot does not survive the prune"
    return K, V, q, w


def needle_expect(V, pos, groups, v_sparsity=0.7):
    """[n_seqs, H, 1, Dd] fp16: the needle's V row, pruned by the oracle's rule."""
    n_seqs, H = pos.shape
    Vh = V.cpu().numpy()
    want = np.stack([np.stack([orc.prune_magnitude(Vh[0, h // groups, int(pos[s, h])][None], v_sparsity)[0] for h in range(H)])
                     for s in range(n_seqs)])
    return torch.from_numpy(want[:, :, None]).to(V.device)


# ---- the call --------------------------------------------------------------------------------------------------------------------------
def run_shape(L_, T, Hkv, groups, n_seqs, Dd):
    """(slabs, blocks per run, blocks of the last run) of a shared call, from the public workspace size: slabs x Hkv x R x (D + 2) floats."""
    R = n_seqs * groups
    ws = L_.mustafar_shared_segment_workspace_bytes(T, Hkv, groups, n_seqs, Dd)
    assert ws > 0 and ws % (Hkv * R * (Dd + 2) * 4) == 0
    slabs = ws // (Hkv * R * (Dd + 2) * 4)
    ntb = T // 64
    assert 1 <= slabs <= ntb
    bpw = -(-ntb // slabs)
    assert -(-ntb // bpw) == slabs, "the slab count is not ceil(blocks / run length) for any whole run length"
    return slabs, bpw, ntb - (slabs - 1) * bpw


class SharedCall:
    """Operands of mustafar_decode_shared_segment over pruned rows Kp / Vp [1, Hkv, T, D] through the package's conversion."""

    def __init__(self, pkg, Kp, Vp, groups, n_seqs):
        from mustafar_amd import _lib
        L_, comp = pkg
        self.L = L_
        _, Hkv, T, Dd = Kp.shape
        self.Hkv, self.T, self.Dd, self.groups, self.n = Hkv, T, Dd, groups, n_seqs
        self.kc = _cache(Kp.reshape(Hkv, T, Dd).contiguous(), "key", comp)
        self.vc = _cache(Vp.reshape(Hkv, T, Dd).contiguous(), "value", comp)
        self.kv = _lib.CacheView(self.kc[0].data_ptr(), self.kc[2].data_ptr(), self.kc[1].data_ptr(), self.kc[3].data_ptr(), 0, 0, 0)
        self.vv = _lib.CacheView(self.vc[0].data_ptr(), self.vc[2].data_ptr(), self.vc[1].data_ptr(), self.vc[3].data_ptr(), 0, 0, 0)
        self.ws = torch.empty((L_.mustafar_shared_segment_workspace_bytes(T, Hkv, groups, n_seqs, Dd),), dtype=torch.uint8, device=DEV)
        self.out = torch.full((n_seqs, Hkv * groups, 1, Dd), float("nan"), dtype=torch.float16, device=DEV)
        self.lse = torch.full((n_seqs, Hkv * groups), float("nan"), dtype=torch.float32, device=DEV)

    def call(self, q):
        err = self.L.mustafar_decode_shared_segment(torch.cuda.current_stream().cuda_stream, ctypes.byref(self.kv), ctypes.byref(self.vv),
                                                    self.T, self.Hkv, self.groups, self.n, q.data_ptr(), self.out.data_ptr(),
                                                    self.lse.data_ptr(), self.ws.data_ptr(), ctypes.c_float(math.sqrt(self.Dd)), self.Dd)
        assert err == 0
        return self.out, self.lse


# ---- the split bound of DESIGN.md 4.9 ---------------------------------------------------------------------------------------------------
def split_bound(parts, lse_bounds, out_all, bound_all):
    """The model's bound of the whole + the parts' own roundings and LSE errors carried through the merge: parts = [(out_i fp64, W_i)],
    W_i the part's share of the whole's denominator.  bound = bound_all + sum_i W_i (2^-11 |out_i| + 2^-25)
    + 2 max_j bound_lse_j * sum_i W_i |out_i - out|."""
    extra = sum(W[..., None, None] * (2.0 ** -11 * o.abs() + 2.0 ** -25) for o, W in parts)
    worst = torch.stack(lse_bounds).amax(0)
    spread = sum(W[..., None, None] * (o - out_all).abs() for o, W in parts)
    return bound_all + extra + 2 * worst[..., None, None] * spread
