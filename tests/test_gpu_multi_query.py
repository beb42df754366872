"""GPU: several query tokens of every sequence per fused decode call (ABI 112: mustafar_decode_multi_query, MustafarAttention.decode_multi
and accept).

The reference has no such path (its q_len > 1 is the dense prefill), so the comparators are the suite's own: the float64 models of
tests/exact_data.py and tests/partial_util.py with their derived bounds -- for query token j evaluated on the K / V that token may see,
the first C rows oracle-pruned --, needles on slots narrow enough for every row of a kv head (tests/shared_util.py: output = the
needle's V row bit for bit, LSE = the needle's x exactly), and the existing one-token call.  kv heads <= 2, batch <= 2."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import exact_data as xd
from tests import partial_util as pu
from tests import shared_util as su
from tests.hd64_util import DEV, S, _cache, oracle_prune

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def pkg():
    from mustafar_amd import _lib, compression
    return _lib.load(), compression


def _hook(Dd, Hq, Hkv, ks=S, vs=S, **kw):
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    return MustafarAttention(MustafarConfig(num_attention_heads=Hq, num_key_value_heads=Hkv, head_dim=Dd, k_sparsity=ks, v_sparsity=vs,
                                            api="fused", **kw))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


# ---- one call of the C entry point over raw rows ------------------------------------------------------------------------------------------
class Call:
    """Operands of one mustafar_decode_multi_query call for K / V [B, Hkv, Ltot, D]: the first C rows compressed (oracle-pruned, through the
    package's conversion, one view per side), rows [C, Ltot - n_q) in the windows, the last n_q rows the call's new rows.  Every window
    row that holds nothing is NaN: a kernel that lets one into an image poisons its output.  stored: the new rows are in the windows
    already and k_new = v_new = NULL."""

    def __init__(self, pkg, K, V, C, n_q, groups, cap=None, ks=S, vs=S, stored=False):
        from mustafar_amd import _lib
        L_, comp = pkg
        self.L = L_
        B, Hkv, Ltot, Dd = K.shape
        self.B, self.Hkv, self.Dd, self.C, self.n_q, self.groups = B, Hkv, Dd, C, n_q, groups
        self.w_len = Ltot - C
        w0 = self.w_len - n_q
        assert w0 >= 0
        self.cap = cap or max(64, (self.w_len + 63) // 64 * 64)
        self.Kp, self.Vp = K.clone(), V.clone()
        if C:
            self.Kp[:, :, :C], self.Vp[:, :, :C] = oracle_prune(K[:, :, :C], ks), oracle_prune(V[:, :, :C], vs)
            self.kc = _cache(self.Kp[:, :, :C].reshape(B * Hkv, C, Dd).contiguous(), "key", comp)
            self.vc = _cache(self.Vp[:, :, :C].reshape(B * Hkv, C, Dd).contiguous(), "value", comp)
            self.kv = _lib.CacheView(self.kc[0].data_ptr(), self.kc[2].data_ptr(), self.kc[1].data_ptr(), self.kc[3].data_ptr(), 0, 0, 0)
            self.vv = _lib.CacheView(self.vc[0].data_ptr(), self.vc[2].data_ptr(), self.vc[1].data_ptr(), self.vc[3].data_ptr(), 0, 0, 0)
        self.kw = torch.full((B, Hkv, self.cap, Dd), NAN, dtype=torch.float16, device=DEV)
        self.vw = torch.full_like(self.kw, NAN)
        kept = self.w_len if stored else w0
        self.kw[:, :, :kept], self.vw[:, :, :kept] = K[:, :, C:C + kept], V[:, :, C:C + kept]
        self.kn = None if stored else K[:, :, Ltot - n_q:].contiguous()
        self.vn = None if stored else V[:, :, Ltot - n_q:].contiguous()
        self.ws_bytes = L_.mustafar_decode_multi_query_workspace_bytes(C, self.cap, B * Hkv, groups, n_q, Dd)
        assert self.ws_bytes > 0
        self.ws = torch.empty((self.ws_bytes,), dtype=torch.uint8, device=DEV)
        self.out = torch.full((B, Hkv * groups, n_q, Dd), NAN, dtype=torch.float16, device=DEV)
        self.lse = torch.full((B, Hkv * groups, n_q), NAN, dtype=torch.float32, device=DEV)

    def runs(self):
        """(compressed runs, blocks per run) read off the public workspace size."""
        slabs = self.ws_bytes // (self.B * self.Hkv * self.n_q * self.groups * (self.Dd + 2) * 4)
        assert slabs * self.B * self.Hkv * self.n_q * self.groups * (self.Dd + 2) * 4 == self.ws_bytes
        runs = slabs - (self.cap + 63) // 64
        return runs, (-(-(self.C // 64) // runs) if runs else 0)

    def call(self, q):
        p = lambda t: t.data_ptr() if t is not None else None
        kv, vv = (ctypes.byref(self.kv), ctypes.byref(self.vv)) if self.C else (None, None)
        err = self.L.mustafar_decode_multi_query(torch.cuda.current_stream().cuda_stream, kv, vv, self.C, None, None, self.C, self.B * self.Hkv,
                                                 self.groups, self.n_q, q.data_ptr(), self.kw.data_ptr(), self.vw.data_ptr(), p(self.kn),
                                                 p(self.vn), self.w_len, self.cap, self.out.data_ptr(), self.lse.data_ptr(),
                                                 self.ws.data_ptr(), ctypes.c_float(math.sqrt(self.Dd)), self.Dd)
        assert err == 0
        return self.out, self.lse


def _run_spans(L_, C, cap, Bkv, groups, n_q, Dd):
    """[(first block, one past the last block)] of every compressed run of a call, from the public workspace size alone.  The run length
    depends on R and D only, so it is the largest block count that the same (cap, Bkv, groups, n_q, D) still serves as ONE run; the slab
    count at C must then be the runs of that length plus the window chunks."""
    per, chunks = Bkv * n_q * groups * (Dd + 2) * 4, (cap + 63) // 64

    def runs(T):
        ws = L_.mustafar_decode_multi_query_workspace_bytes(T, cap, Bkv, groups, n_q, Dd)
        assert ws > 0 and ws % per == 0
        return ws // per - chunks

    assert runs(0) == 0 and runs(64) == 1
    bpw = 1
    while runs(64 * (bpw + 1)) == 1:
        bpw += 1
    ntb = C // 64
    assert runs(C) == -(-ntb // bpw)
    return [(b, min(ntb, b + bpw)) for b in range(0, ntb, bpw)]


def _rule(R, Dd):
    """Blocks per run, DESIGN.md 4.10 restated: the smallest count whose stream bytes (about 88 D a block) reach the slab bytes 8 R (D + 2)."""
    return -(-8 * R * (Dd + 2) // (88 * Dd))


def _model_ratios(out, lse, q, Kp, Vp, first, groups):
    """max |out - hook_model| / bound and |lse - lse_model| / bound over the tokens of a call: token j sees rows [0, first + j + 1) of
    Kp / Vp (pruned where compressed)."""
    r_out = r_lse = 0.0
    for j in range(q.shape[2]):
        Lj = first + j + 1
        want, bound = xd.hook_model(q[:, :, j:j + 1], Kp[:, :, :Lj], Vp[:, :, :Lj], groups)
        r = (out[:, :, j:j + 1].double() - want).abs() / bound
        r_out = max(r_out, float(r.max()) if torch.isfinite(r).all() else float("inf"))
        want_l, bound_l = pu.lse_model(q[:, :, j:j + 1], Kp[:, :, :Lj], groups)
        r_lse = max(r_lse, pu.lse_ratio(lse[:, :, j], want_l, bound_l))
    return r_out, r_lse


def _assert_models(out, lse, q, Kp, Vp, first, groups, what):
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all(), f"{what}: NaN / Inf in the outputs"
    r_out, r_lse = _model_ratios(out, lse, q, Kp, Vp, first, groups)
    print(f"{what}: |out - model| / bound = {r_out:.3f}, |lse - model| / bound = {r_lse:.3f}")
    assert r_out <= 1.0 and r_lse <= 1.0, f"{what}: out {r_out:.3f}, lse {r_lse:.3f}"


def _rand(B, Hkv, Ltot, groups, n_q, Dd, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    K = torch.randn((B, Hkv, Ltot, Dd), generator=g, device=DEV).half()
    V = torch.randn((B, Hkv, Ltot, Dd), generator=g, device=DEV).half()
    q = torch.randn((B, Hkv * groups, n_q, Dd), generator=g, device=DEV).half()
    return K, V, q


# ---- needles: row (b, h, j) attends to ONE token --------------------------------------------------------------------------------------------
def needle_data(Dd, B, Hkv, groups, n_q, Ltot, pos, C, seed, ks=S, twice=None, boost=1):
    """K, V [B, Hkv, Ltot, Dd], q [B, H, n_q, Dd]: the row of q head h and query token j attends to token pos[b, h, j] of its kv head.
    The R = n_q x groups rows of a kv head own a slot each (tests/shared_util.py: width, level, key noise |k| <= 1, V multiples of 2^-5).
    twice [B, H, n_q] (-1: none): a needle of twice the level in the same slot -- the winner wherever the row can see it.  Needles among
    the first C tokens must survive the oracle's prune.  boost: see tests/shared_util.py.  Returns K, V, q, slot width."""
    H, R = Hkv * groups, n_q * groups
    w = su.slot_width(Dd, R)
    lv = boost * su.level(w)
    assert su.needle_x(Dd, w, boost) - su.other_x_max(Dd, w) > 39
    gen = torch.Generator(device="cpu").manual_seed(seed)
    K = torch.randint(-4, 5, (B, Hkv, Ltot, Dd), generator=gen).half() * 0.25
    V = torch.randint(-64, 65, (B, Hkv, Ltot, Dd), generator=gen).half() * 2.0 ** -5
    q = torch.zeros((B, H, n_q, Dd), dtype=torch.float16)
    for b in range(B):
        for h in range(H):
            for j in range(n_q):
                r = j * groups + h % groups
                sl = slice(r * w, (r + 1) * w)
                p = int(pos[b, h, j])
                assert 0 <= p < Ltot
                K[b, h // groups, p, sl] = lv
                if twice is not None and twice[b, h, j] >= 0:
                    K[b, h // groups, int(twice[b, h, j]), sl] = 2 * lv
                q[b, h, j, sl] = su.QB
                if p < C:
                    kept = orc.prune_magnitude(K[b, h // groups, p][None].numpy(), ks)[0]
                    assert (kept[sl] == lv).all(), "a needle slot does not survive the prune"
    return K.to(DEV), V.to(DEV), q.to(DEV), w


def needle_want(V, pos, C, groups, vs=S):
    """[B, H, n_q, Dd] fp16: each row's needle's V row, pruned by the oracle's rule where the token is compressed."""
    B, H, n_q = pos.shape
    Vh = V.cpu().numpy()
    want = np.zeros((B, H, n_q, V.shape[3]), np.float16)
    for b in range(B):
        for h in range(H):
            for j in range(n_q):
                p = int(pos[b, h, j])
                row = Vh[b, h // groups, p]
                want[b, h, j] = orc.prune_magnitude(row[None], vs)[0] if p < C else row
    return torch.from_numpy(want).to(V.device)


def _assert_needles(out, lse, V, pos, C, groups, Dd, w, what, boost=1):
    want = needle_want(V, pos, C, groups)
    miss = (out.float() != want.float()).any(-1)
    assert not miss.any(), f"{what}: rows {miss.nonzero().tolist()} differ from their needle's V row"
    assert torch.equal(lse, torch.full_like(lse, su.needle_x(Dd, w, boost))), f"{what}: an LSE is not the needle's x"


# ---- 1. exact needles in the compressed part and the window -------------------------------------------------------------------------------
# R = 35, 42, 48, 34: three row tiles (odd n_q with padded rows, a tile exactly full, groups = 2); R = 49: one row into the fourth tile
NEEDLE_ROWS = [(1, 4), (3, 3), (4, 4), (8, 4), (16, 4), (8, 8), (2, 1), (7, 5), (6, 7), (8, 6), (17, 2), (7, 7)]


@pytest.mark.parametrize("n_q,groups", NEEDLE_ROWS)
@pytest.mark.parametrize("T", [0, 64, 320])
@pytest.mark.parametrize("Dd", [64, 128])
def test_exact_on_needles(pkg, Dd, T, n_q, groups):
    """Needles on token 0, every block edge, T - 1, window row 0, the last old window row and each token's own new row, spread over
    the rows of as many calls as it takes.  (needle_data asserts the slot width and the gap: one channel at D = 64 from R = 33 on.)"""
    B, Hkv, w0 = 1, 2, 5
    H, Ltot = Hkv * groups, T + w0 + n_q
    targets = (su.edge_positions(T) if T else []) + [T, T + w0 - 1]
    k, c = 0, 0
    while k < len(targets):
        pos = np.zeros((B, H, n_q), np.int64)
        for b, h, j in np.ndindex(B, H, n_q):
            if (h + j) % 2 == 0:      # the row's own new row: every token has such a row among its heads
                pos[b, h, j] = T + w0 + j
            else:
                pos[b, h, j] = targets[k % len(targets)]
                k += 1
        K, V, q, w = needle_data(Dd, B, Hkv, groups, n_q, Ltot, pos, T, seed=Dd + T + n_q * groups + c)
        out, lse = Call(pkg, K, V, T, n_q, groups).call(q)
        _assert_needles(out, lse, V, pos, T, groups, Dd, w, f"call {c}")
        c += 1


# ---- 2. the causal limit, exact ------------------------------------------------------------------------------------------------------------
#   (the largest window: w0 = 1000 at n_q = 8 gives a capacity of 1024, sixteen chunks, and the spare row behind window_len still exists)
CAUSAL = [(Dd, n_q, groups, w0) for Dd, n_q, groups in [(64, 4, 4), (128, 8, 4), (128, 3, 3), (64, 7, 5), (128, 6, 7), (128, 12, 4)]
          for w0 in [0, 1, 62, 63, 64, 250]] + [(128, 8, 4, 1000)]


@pytest.mark.parametrize("Dd,n_q,groups,w0", CAUSAL)
def test_the_causal_limit_is_exact(pkg, Dd, n_q, groups, w0):
    """Every row of query token j has its needle on window row w0 + j, its own new row and the last it may see; a needle of twice the level
    sits in the same slot one row later, which it must not see (for the last token: in the spare row behind the window).  One row too few
    loses the needle, one too many finds the stronger one."""
    B, Hkv, T = 1, 2, 64
    H = Hkv * groups
    Ltot = T + w0 + n_q
    pos = np.zeros((B, H, n_q), np.int64)
    pos[:] = T + w0 + np.arange(n_q)
    K, V, q, w = needle_data(Dd, B, Hkv, groups, n_q, Ltot + 1, pos, T, seed=Dd + w0, twice=pos + 1)
    c = Call(pkg, K[:, :, :Ltot], V[:, :, :Ltot], T, n_q, groups, cap=(w0 + n_q + 1 + 63) // 64 * 64)
    assert c.cap > w0 + n_q and (w0 != 1000 or c.cap == 1024)
    c.kw[:, :, w0 + n_q], c.vw[:, :, w0 + n_q] = K[:, :, Ltot], V[:, :, Ltot]   # the spare row behind window_len: visible to nobody
    out, lse = c.call(q)
    _assert_needles(out, lse, V, pos, T, groups, Dd, w, f"w0 {w0}")


# ---- 3. a row that sees nothing in a chunk --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w0,n_q,cap", [(60, 8, 128), (56, 8, 128), (60, 8, 192)])
@pytest.mark.parametrize("Dd", [64, 128])
def test_a_row_that_sees_no_column_of_a_chunk(pkg, Dd, w0, n_q, cap):
    """w0 = 60, n_q = 8: tokens 0 .. 3 see no column of the second chunk; w0 + n_q = 64 with capacity 128 (and 192): whole chunks beyond the
    window.  The spare rows of the windows hold NaN.  No NaN / Inf anywhere, the models hold, needles on the own rows are exact."""
    B, Hkv, groups, T = 1, 2, 4, 64
    K, V, q = _rand(B, Hkv, T + w0 + n_q, groups, n_q, Dd, seed=Dd + w0)
    c = Call(pkg, K, V, T, n_q, groups, cap=cap)
    out, lse = c.call(q)
    _assert_models(out, lse, q, c.Kp, c.Vp, T + w0, groups, f"D={Dd} w0={w0} cap={cap}")
    pos = np.zeros((B, Hkv * groups, n_q), np.int64)
    pos[:] = T + w0 + np.arange(n_q)
    K, V, q, w = needle_data(Dd, B, Hkv, groups, n_q, T + w0 + n_q, pos, T, seed=Dd)
    out, lse = Call(pkg, K, V, T, n_q, groups, cap=cap).call(q)
    _assert_needles(out, lse, V, pos, T, groups, Dd, w, f"w0 {w0} cap {cap}")
    # nothing compressed at all: the window alone
    K, V, q = _rand(B, Hkv, w0 + n_q, groups, n_q, Dd, seed=Dd + 1)
    c = Call(pkg, K, V, 0, n_q, groups, cap=cap)
    out, lse = c.call(q)
    _assert_models(out, lse, q, c.Kp, c.Vp, w0, groups, f"D={Dd} T=0 w0={w0} cap={cap}")


# ---- 4. random data against the models -----------------------------------------------------------------------------------------------------
#         n_q, groups, T, window_len, capacity, (runs, blocks per run) the public workspace size must show
SHAPES = [(1, 4, 64, 1, 64, (1, 1)),          # the window at one row
          (3, 3, 192, 63, 64, (3, 1)),        # R = 9: one block per run
          (3, 3, 128, 64, 64, (2, 1)),        # the window at its capacity
          (3, 3, 64, 65, 128, (1, 1)),
          (5, 4, 192, 128, 128, (2, 2)),      # R = 20: two blocks per run and a shorter last run; the window at its capacity
          (8, 4, 320, 65, 128, (2, 3)),       # R = 32: three blocks per run, a last run of two
          (16, 4, 704, 40, 64, (2, 6))]       # R = 64: six blocks per run, a last run of five
# Row tiles and group counts the rows above leave out.  T and the shape follow from the run-length rule at the head dim (_rule): two runs
# with a shorter last one, T = 64 (2 bpw - 1), or three one-block runs; a window of 65 .. 70 rows in a capacity of 128: the first tokens
# see nothing in the second chunk.
SHAPES += [(n_q, groups, None, 65 + n_q * groups % 6, 128, None)
           for n_q, groups in [(7, 5), (6, 7), (8, 6), (17, 2), (11, 3), (17, 1), (7, 7)]]


@pytest.mark.parametrize("ks,vs", [(0.5, 0.7), (0.7, 0.9)])
@pytest.mark.parametrize("n_q,groups,T,w_len,cap,shape", SHAPES)
@pytest.mark.parametrize("Dd", [64, 128])
def test_random_data_against_the_models(pkg, Dd, n_q, groups, T, w_len, cap, shape, ks, vs):
    B, Hkv = 2, 2
    if shape is None:
        bpw = _rule(n_q * groups, Dd)
        T, shape = (192, (3, 1)) if bpw == 1 else (64 * (2 * bpw - 1), (2, bpw))
        assert 65 <= w_len <= 70 and w_len - n_q < 64   # token 0 sees no column of the second chunk
    K, V, q = _rand(B, Hkv, T + w_len, groups, n_q, Dd, seed=T + Dd + n_q * groups)
    c = Call(pkg, K, V, T, n_q, groups, cap=cap, ks=ks, vs=vs)
    assert c.runs() == shape and (T // 64) % shape[1] == (0 if shape[1] == 1 else shape[1] - 1)
    out, lse = c.call(q)
    _assert_models(out, lse, q, c.Kp, c.Vp, T + w_len - n_q, groups, f"D={Dd} R={n_q * groups} T={T} w={w_len} K{ks}/V{vs}")


# ---- the hook: pasts of every cache kind ---------------------------------------------------------------------------------------------------
#   (inplace: the arena whose trigger appends in place instead of listing an extent)
KINDS = {"list": dict(), "arena": dict(arena=True), "inplace": dict(arena=True, extents=False), "ext64": dict(hd64_extents=True)}


def _attn(kind, groups=4, Hkv=2, **kw):
    Dd = kw.pop("Dd", 128)
    Dd = 64 if kind == "ext64" else Dd
    return _hook(Dd, Hkv * groups, Hkv, **KINDS[kind], **kw)


def _past(attn, K, V, L0):
    return attn.to_fused(attn.build_cache(K[:, :, :L0].contiguous(), V[:, :, :L0].contiguous()))


def _grow(attn, K, V, q1, extents):
    """A past over K / V [B, Hkv, >= 288 + 256 extents, D] whose cache has been through `extents` triggers, one decode_fused step each: the
    window is refilled with the 255 rows in front of the next trigger point.  Returns (past, tokens it holds)."""
    from mustafar_amd.hook import Window
    past = _past(attn, K, V, 256 + 32 + 255)
    n = 256 + 32 + 255
    for e in range(extents):
        k_c, k_w, v_c, v_w, C, L = past
        if e:   # rows [C, C + 287) into the windows: one step short of the trigger
            n = C + 287
            past = (k_c, Window(K[:, :, C:n].contiguous(), 288), v_c, Window(V[:, :, C:n].contiguous(), 288), C, n)
        _, past = attn.decode_fused(q1, K[:, :, n:n + 1], V[:, :, n:n + 1], past)
        n += 1
        assert past[4] == 256 * (e + 2) and past[1].len == 32 and past[5] == n
    return past, n


def _reference(c):
    c = c.to_reference() if hasattr(c, "to_reference") else c
    nz = c[2]
    return [c[0].reshape(-1), c[1].reshape(-1), nz if isinstance(nz, torch.Tensor) else torch.cat(list(nz)), c[3].reshape(-1)]


def _same_cache(a, b):
    return all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(_reference(a), _reference(b)))


def _hook_models(attn, out, lse, q, K, V, past_before, what):
    """The models over what a decode_multi call on `past_before` (C compressed tokens, kv_seq_len rows) saw."""
    C, L = past_before
    Kp, Vp = K.clone(), V.clone()
    Kp[:, :, :C], Vp[:, :, :C] = oracle_prune(K[:, :, :C], attn.cfg.k_sparsity), oracle_prune(V[:, :, :C], attn.cfg.v_sparsity)
    _assert_models(out, lse, q, Kp, Vp, L, attn.num_key_value_groups, what)
    return Kp, Vp


# ---- 5. extents --------------------------------------------------------------------------------------------------------------------------
def _crossings(spans, ntb_base=4, per_extent=4):
    """What each run of `spans` crosses: (run, "base->extent") / (run, "extent->extent"), the base being blocks [0, ntb_base) and extent e
    blocks [ntb_base + per_extent e, + per_extent)."""
    region = lambda b: -1 if b < ntb_base else (b - ntb_base) // per_extent
    out = []
    for i, (b0, b1) in enumerate(spans):
        for b in range(b0 + 1, b1):
            if region(b) != region(b - 1):
                out.append((i, "base->extent" if region(b - 1) < 0 else "extent->extent"))
    return out


@pytest.mark.parametrize("n_q", [3, 8, 11, 13])
@pytest.mark.parametrize("extents", [1, 2])
@pytest.mark.parametrize("kind", ["arena", "ext64"])
def test_extents(pkg, kind, extents, n_q):
    """T_base = 256 and one or two extents at R = 12, 32, 44 and 52: one to four row tiles of the EXT instantiations (groups = 4: the
    decode_fused steps that grow an arena by extents need it).  R = 12: two blocks per run, no run crosses a boundary (per-block resolution
    alone); R = 32: three blocks per run, run 1 crosses base -> extent; R = 44 and 52: five blocks per run, run 0 crosses base -> extent
    and, with two extents, run 1 extent -> extent -- all read off the workspace size.  Random data against the models; needles on the
    first and last token of the base and of each extent; the same tokens consolidated into one view: the same bits."""
    B, Hkv, groups = 1, 2, 4
    attn = _attn(kind)
    Dd = attn.head_dim
    total = 256 * (extents + 1) + 32 + n_q
    K, V, q = _rand(B, Hkv, total, groups, n_q, Dd, seed=extents + Dd)
    past, n = _grow(attn, K, V, q[:, :, :1].contiguous(), extents)
    assert n + n_q == total and len(past[0].extents) == extents and past[0].tokens == 256
    spans = _run_spans(pkg[0], past[4], past[1].cap, B * Hkv, groups, n_q, Dd)
    crossed = _crossings(spans)
    print(f"{kind} R={n_q * groups} {extents} extents: runs {spans}, crossings {crossed}")
    if n_q == 3:
        assert spans[0] == (0, 2) and not crossed
    elif n_q == 8:
        assert spans[0] == (0, 3) and (1, "base->extent") in crossed
    else:
        assert spans[0] == (0, 5) and (0, "base->extent") in crossed and (extents == 1 or (1, "extent->extent") in crossed)
    out, lse, new = attn.decode_multi(q, K[:, :, n:], V[:, :, n:], past, return_lse=True)
    assert new[5] == total and new[1].len == 32 + n_q
    _hook_models(attn, out, lse, q, K, V, (past[4], n), f"{kind} {extents} extents")
    # one view per side: the run shape is the same (it depends on R and D alone), so the sums are the same sums
    k1, v1 = past[0].consolidate(), past[2].consolidate()
    assert not k1.extents and k1.tokens == 256 * (extents + 1)
    w = new[1].clone(), new[3].clone()
    w[0].len = w[1].len = 32
    out1, lse1, _ = attn.decode_multi(q, K[:, :, n:], V[:, :, n:], (k1, w[0], v1, w[1], past[4], n), return_lse=True)
    assert torch.equal(_bits(out), _bits(out1)) and torch.equal(_bits(lse), _bits(lse1))
    # needles on the first and last token of the base and of each extent
    edges = [t for e in range(extents + 1) for t in (256 * e, 256 * e + 255)]
    pos = np.zeros((B, Hkv * groups, n_q), np.int64)
    for i, idx in enumerate(np.ndindex(B, Hkv * groups, n_q)):
        pos[idx] = edges[i % len(edges)]
    C = 256 * (extents + 1)
    K, V, q, w = needle_data(Dd, B, Hkv, groups, n_q, total, pos, C, seed=7 + extents)
    past, n = _grow(attn, K, V, q[:, :, :1].contiguous(), extents)
    out, lse, _ = attn.decode_multi(q, K[:, :, n:], V[:, :, n:], past, return_lse=True)
    _assert_needles(out, lse, V, pos, C, groups, Dd, w, f"{kind} {extents} extents")


# ---- 6. one token against the existing call -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,Dd", [("list", 64), ("list", 128), ("arena", 128), ("inplace", 128), ("ext64", 64)])
def test_one_token_against_decode_fused(kind, Dd):
    B, Hkv, groups, L0 = 2, 2, 4, 256 + 70
    attn = _attn(kind, Dd=Dd)
    K, V, q = _rand(B, Hkv, L0 + 1, groups, 1, attn.head_dim, seed=Dd)
    pa, pb = _past(attn, K, V, L0), _past(attn, K, V, L0)
    a, la, na = attn.decode_multi(q, K[:, :, L0:], V[:, :, L0:], pa, return_lse=True)
    b, nb = attn.decode_fused(q, K[:, :, L0:], V[:, :, L0:], pb)
    Kp, Vp = _hook_models(attn, a, la, q, K, V, (256, L0), f"{kind} D={Dd}")
    _, bound = xd.hook_model(q, Kp, Vp, groups)
    assert float(((a.double() - b.double()).abs() / (2 * bound)).max()) <= 1.0
    assert na[1].len == nb[1].len == 71 and na[5] == nb[5] == L0 + 1
    assert torch.equal(_bits(na[1].view()), _bits(nb[1].view())) and torch.equal(_bits(na[3].view()), _bits(nb[3].view()))


# ---- 7. several tokens against several steps, through a trigger ------------------------------------------------------------------------------
def _steps(attn, q, K, V, past, n0, count):
    outs = []
    for j in range(count):
        o, past = attn.decode_fused(q[:, :, j:j + 1].contiguous(), K[:, :, n0 + j:n0 + j + 1], V[:, :, n0 + j:n0 + j + 1], past)
        outs.append(o)
    return torch.cat(outs, dim=2), past


def _within_twice_the_bound(a, b, q, Kp, Vp, first, groups):
    for j in range(a.shape[2]):
        _, bound = xd.hook_model(q[:, :, j:j + 1], Kp[:, :, :first + j + 1], Vp[:, :, :first + j + 1], groups)
        r = float(((a[:, :, j:j + 1].double() - b[:, :, j:j + 1].double()).abs() / (2 * bound)).max())
        assert r <= 1.0, f"token {j}: |multi - stepwise| / (2 bound) = {r:.3f}"


@pytest.mark.parametrize("kind", ["list", "arena", "inplace", "ext64"])
def test_six_tokens_against_six_steps_through_a_trigger(kind):
    """The prefill leaves 256 compressed tokens and a window of 282 rows: the sixth row brings it to residual_length + 256 and the trigger
    runs inside accept, as it runs inside the sixth decode_fused step."""
    B, Hkv, groups, n_q, L0 = 2, 2, 4, 6, 256 + 282
    attn = _attn(kind)
    K, V, q = _rand(B, Hkv, L0 + n_q, groups, n_q, attn.head_dim, seed=11)
    pa, pb = _past(attn, K, V, L0), _past(attn, K, V, L0)
    a, la, na = attn.decode_multi(q, K[:, :, L0:], V[:, :, L0:], pa, return_lse=True)
    assert na[4] == 256 and na[1].len == 288 and attn.trigger_due(na)
    Kp, Vp = _hook_models(attn, a, la, q, K, V, (256, L0), kind)
    na = attn.accept(na)
    b, nb = _steps(attn, q, K, V, pb, L0, n_q)
    _within_twice_the_bound(a, b, q, Kp, Vp, L0, groups)
    assert na[4] == nb[4] == 512 and na[5] == nb[5] == L0 + n_q and na[1].len == nb[1].len == 32 and na[3].len == nb[3].len == 32
    assert torch.equal(_bits(na[1].view()), _bits(nb[1].view())) and torch.equal(_bits(na[3].view()), _bits(nb[3].view()))
    assert _same_cache(na[0], nb[0]) and _same_cache(na[2], nb[2])


# ---- 8. rejection ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,Dd", [("list", 128), ("ext64", 64)])
def test_rejected_rows_leave_no_trace(kind, Dd):
    """decode_multi(6), accept(rejected=2), one decode_fused step == decode_multi(4), accept(), that step.  At the trigger shape of the
    test above a single rejected row keeps the trigger from firing."""
    B, Hkv, groups, L0 = 2, 2, 4, 256 + 90
    attn = _attn(kind, Dd=Dd)
    K, V, q = _rand(B, Hkv, L0 + 6, groups, 6, attn.head_dim, seed=13)
    nxt = (q[:, :, 5:6].contiguous(), K[:, :, L0 + 5:L0 + 6], V[:, :, L0 + 5:L0 + 6])   # the step behind the four accepted tokens
    a, pa = attn.decode_multi(q, K[:, :, L0:], V[:, :, L0:], _past(attn, K, V, L0))
    pa = attn.accept(pa, rejected=2)
    assert pa[1].len == 94 and pa[5] == L0 + 4
    sa, pa = attn.decode_fused(*nxt, pa)
    b, pb = attn.decode_multi(q[:, :, :4], K[:, :, L0:L0 + 4], V[:, :, L0:L0 + 4], _past(attn, K, V, L0))
    pb = attn.accept(pb)
    sb, pb = attn.decode_fused(*nxt, pb)
    Kr, Vr = torch.cat([K[:, :, :L0 + 4], nxt[1]], 2), torch.cat([V[:, :, :L0 + 4], nxt[2]], 2)
    Kp, Vp = Kr.clone(), Vr.clone()
    Kp[:, :, :256], Vp[:, :, :256] = oracle_prune(K[:, :, :256], S), oracle_prune(V[:, :, :256], S)
    _within_twice_the_bound(a[:, :, :4], b, q, Kp, Vp, L0, groups)
    _within_twice_the_bound(sa, sb, nxt[0], Kp, Vp, L0 + 4, groups)
    assert pa[1].len == pb[1].len == 95 and pa[5] == pb[5] == L0 + 5
    assert torch.equal(_bits(pa[1].view()), _bits(pb[1].view())) and torch.equal(_bits(pa[3].view()), _bits(pb[3].view()))
    # one row short of the trigger: nothing fires
    L1 = 256 + 282
    K, V, q = _rand(B, Hkv, L1 + 6, groups, 6, attn.head_dim, seed=14)
    _, p = attn.decode_multi(q, K[:, :, L1:], V[:, :, L1:], _past(attn, K, V, L1))
    p = attn.accept(p, rejected=1)
    assert p[4] == 256 and p[1].len == 287 and p[5] == L1 + 5 and not attn.trigger_due(p)


# ---- 9. chunking -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dd", [64, 128])
def test_twenty_tokens_run_as_two_calls(Dd):
    """n_q = 20 at G = 4 is 80 rows per kv head: two calls of 16 + 4 tokens, the second over the rows the first appended."""
    B, Hkv, groups, n_q, L0 = 1, 2, 4, 20, 256 + 40
    attn = _attn("list", Dd=Dd)
    K, V, q = _rand(B, Hkv, L0 + n_q, groups, n_q, Dd, seed=Dd)
    out, lse, new = attn.decode_multi(q, K[:, :, L0:], V[:, :, L0:], _past(attn, K, V, L0), return_lse=True)
    assert out.shape == (B, Hkv * groups, n_q, Dd) and lse.shape == (B, Hkv * groups, n_q) and new[1].len == 60 and new[5] == L0 + n_q
    _hook_models(attn, out, lse, q, K, V, (256, L0), f"D={Dd} n_q=20")


# ---- 10. graph ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dd", [64, 128])
def test_a_captured_call_is_replayed_with_new_queries(pkg, Dd):
    """One call at fixed lengths, the rows stored ahead and k_new == NULL, captured in a graph and replayed twice with alternating queries."""
    B, Hkv, groups, n_q, T, w0 = 2, 2, 4, 4, 192, 70
    K, V, qa = _rand(B, Hkv, T + w0 + n_q, groups, n_q, Dd, seed=Dd)
    qb = torch.randn(qa.shape, generator=torch.Generator(device=DEV).manual_seed(Dd + 1), device=DEV).half()
    c = Call(pkg, K, V, T, n_q, groups, cap=128, stored=True)
    q = qa.clone()
    c.call(q)   # (warm: module load outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c.call(q)
    for which, src in (("a", qa), ("b", qb), ("a", qa)):
        q.copy_(src)
        c.out.fill_(NAN)
        c.lse.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        _assert_models(c.out, c.lse, src, c.Kp, c.Vp, T + w0, groups, f"D={Dd} replay {which}")


# ---- 11. layout ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,Dd", [("list", 64), ("arena", 128), ("inplace", 128)])
def test_each_sequence_and_head_reads_its_own_cache(kind, Dd):
    """batch 2, kv heads 2, a query that is not contiguous: needles that differ per sequence and head, half of them in the compressed part."""
    B, Hkv, groups, n_q, L0 = 2, 2, 4, 4, 256 + 40
    attn = _attn(kind, Dd=Dd)
    H = Hkv * groups
    rng = np.random.default_rng(Dd)
    pos = np.zeros((B, H, n_q), np.int64)
    for i, idx in enumerate(np.ndindex(B, H, n_q)):
        pos[idx] = rng.integers(0, 256) if i % 2 else rng.integers(256, L0 + idx[2] + 1)
    assert len({tuple(pos[0].ravel()), tuple(pos[1].ravel())}) == 2
    K, V, q, w = needle_data(Dd, B, Hkv, groups, n_q, L0 + n_q, pos, 256, seed=Dd)
    q_nc = q.permute(2, 0, 1, 3).contiguous().permute(1, 2, 0, 3)
    assert not q_nc.is_contiguous() and torch.equal(q_nc, q)
    out, lse, _ = attn.decode_multi(q_nc, K[:, :, L0:], V[:, :, L0:], _past(attn, K, V, L0), return_lse=True)
    assert out.is_contiguous()
    _assert_needles(out, lse, V, pos, 256, groups, Dd, w, kind)


# ---- 12. from an empty cache, through the first trigger -------------------------------------------------------------------------------------
def _pruned(attn, K, V, C):
    Kp, Vp = K.clone(), V.clone()
    Kp[:, :, :C], Vp[:, :, :C] = oracle_prune(K[:, :, :C], attn.cfg.k_sparsity), oracle_prune(V[:, :, :C], attn.cfg.v_sparsity)
    return Kp, Vp


@pytest.mark.parametrize("kind,Dd", [("list", 64), ("list", 128), ("arena", 128), ("inplace", 128), ("ext64", 64)])
def test_from_an_empty_cache_through_the_first_trigger(kind, Dd):
    """A prefill of 250 rows compresses nothing (C = 0, no cache object).  decode_multi serves the window alone (at D = 128 too, with an
    LSE: decode_fused(return_lse=True) refuses that call); further calls are sized by _fits_before_trigger until the last row of one is
    the trigger point at 288 rows, and accept() runs the FIRST trigger of the kind: the compressed front of a list, an arena from the raw
    rows, an extent cache's base.  A twin takes the same rows through decode_fused steps.  Then one more call over the new cache."""
    B, Hkv, groups, L0 = 2, 2, 4, 250
    attn = _attn(kind, Dd=Dd)
    Dd = attn.head_dim
    total = 288 + 5
    K, V, q = _rand(B, Hkv, total, groups, total - L0, Dd, seed=Dd + 17)   # q[:, :, i]: the query of token L0 + i
    pa, pb = _past(attn, K, V, L0), _past(attn, K, V, L0)
    assert pa[4] == 0 and pa[0] is None and pa[2] is None and pa[1].len == L0
    Kp, Vp = K, V   # nothing is pruned before the trigger
    n, fired, capped = L0, False, False
    for want in (6, 12, 12, 12):
        fit = attn._fits_before_trigger(pa, want)
        capped |= fit < want
        qs = q[:, :, n - L0:n - L0 + fit].contiguous()
        a, la, pa = attn.decode_multi(qs, K[:, :, n:n + fit], V[:, :, n:n + fit], pa, return_lse=True)
        _assert_models(a, la, qs, Kp, Vp, n, groups, f"{kind} D={Dd} C=0 tokens [{n}, {n + fit})")
        b, pb = _steps(attn, qs, K, V, pb, n, fit)
        _within_twice_the_bound(a, b, qs, Kp, Vp, n, groups)
        n += fit
        assert pa[5] == n and pa[1].len == n and pa[4] == 0
        fired = attn.trigger_due(pa)
        pa = attn.accept(pa)
        if fired:
            break
        assert pa[4] == 0 and pa[0] is None
    assert fired and capped and n == 288, "no call ended on the trigger point"
    assert pa[4] == pb[4] == 256 and pa[5] == pb[5] == 288 and pa[1].len == pb[1].len == 32 and pa[3].len == pb[3].len == 32
    assert type(pa[0]) is type(pb[0]) and pa[0] is not None
    assert torch.equal(_bits(pa[1].view()), _bits(pb[1].view())) and torch.equal(_bits(pa[3].view()), _bits(pb[3].view()))
    assert _same_cache(pa[0], pb[0]) and _same_cache(pa[2], pb[2])
    # one more call, over the cache the first trigger made
    qs = q[:, :, n - L0:].contiguous()
    assert qs.shape[2] == 5
    a, la, pa = attn.decode_multi(qs, K[:, :, n:], V[:, :, n:], pa, return_lse=True)
    _hook_models(attn, a, la, qs, K, V, (256, n), f"{kind} D={Dd} after the first trigger")
    assert pa[4] == 256 and pa[5] == total and pa[1].len == 37


# ---- 13. a speculative loop with rejections, across a trigger, the spare rows poisoned ------------------------------------------------------
#          (tokens asked for, drafts rejected): capped by _fits_before_trigger.  Round 2 ends on the trigger point and its rejection takes the
#          window back off it; round 3 is capped to the four rows that reach it again, nothing rejected: the trigger fires; three rounds follow.
ROUNDS = [(8, 3), (8, 0), (5, 4), (12, 0), (12, 7), (3, 2), (16, 0)]


@pytest.mark.parametrize("kind,Dd", [("list", 64), ("arena", 128)])
def test_a_speculative_loop_with_rejections_across_a_trigger(kind, Dd):
    """Rounds of decode_multi + accept(rejected) against a twin that takes the accepted tokens alone through decode_fused steps.  On the
    multi side the rows [len, cap) of both window buffers are NaN after every accept: they are spare by contract (the rejected rows
    among them), so a stale read shows as NaN in out or lse.  A rejected draft's rows differ from the token accepted in its place."""
    B, Hkv, groups, L0 = 2, 2, 4, 256 + 270
    attn = _attn(kind, Dd=Dd)
    accepted = sum(a - r for a, r in ROUNDS)   # (an upper limit: capped rounds accept fewer)
    K, V, q = _rand(B, Hkv, L0 + accepted, groups, accepted, Dd, seed=Dd + 23)            # the accepted stream; q[:, :, i]: token L0 + i
    Kd, Vd, qd = _rand(B, Hkv, 16, groups, 16, Dd, seed=Dd + 24)                          # drafts that get rejected
    pruned = {C: _pruned(attn, K, V, C) for C in (256, 512)}
    pa, pb = _past(attn, K, V, L0), _past(attn, K, V, L0)
    n, fired_at, held_back = L0, None, False
    for i, (want, rej) in enumerate(ROUNDS):
        fit = attn._fits_before_trigger(pa, want)
        assert rej < fit
        keep = fit - rej
        sl = slice(n - L0, n - L0 + keep)
        qs = torch.cat([q[:, :, sl], qd[:, :, :rej]], 2).contiguous()
        ks = torch.cat([K[:, :, n:n + keep], Kd[:, :, :rej]], 2)
        vs = torch.cat([V[:, :, n:n + keep], Vd[:, :, :rej]], 2)
        C = pa[4]
        a, la, pa = attn.decode_multi(qs, ks, vs, pa, return_lse=True)
        assert torch.isfinite(a.float()).all() and torch.isfinite(la).all(), f"round {i}: NaN / Inf in out or lse"
        due = attn.trigger_due(pa)
        pa = attn.accept(pa, rejected=rej)
        for w in (pa[1], pa[3]):
            w.buf[:, :, w.len:] = NAN
        b, pb = _steps(attn, qs, K, V, pb, n, keep)
        _within_twice_the_bound(a[:, :, :keep], b, qs, *pruned[C], n, groups)
        n += keep
        if due and rej:      # the window reached the trigger point, the rejection took it back: nothing fires
            held_back = True
            assert not attn.trigger_due(pa) and pa[4] == C and pa[1].len == 288 - rej
        if due and not rej:
            assert fired_at is None and held_back and fit < want and pa[4] == C + 256 and pa[1].len == 32
            fired_at = i
        assert pa[4] == pb[4] and pa[5] == pb[5] == n and pa[1].len == pb[1].len == pa[3].len == pb[3].len == n - pa[4]
    assert held_back and fired_at is not None and len(ROUNDS) - 1 - fired_at >= 3
    assert pa[4] == pb[4] == 512 and pa[5] == pb[5] == n
    assert torch.equal(_bits(pa[1].view()), _bits(pb[1].view())) and torch.equal(_bits(pa[3].view()), _bits(pb[3].view()))
    assert _same_cache(pa[0], pb[0]) and _same_cache(pa[2], pb[2])


# ---- 14. many slabs through the merge; the largest window -----------------------------------------------------------------------------------
@pytest.mark.parametrize("Dd", [64, 128])
def test_more_than_64_slabs_through_the_merge(pkg, Dd):
    """R = 8 is one block per run: 4608 tokens are 72 runs, with the window chunks more than the 64 lanes of the merge's max loop and
    several trips of its phase loop, in the (B', R, R) addressing of this entry point."""
    B, Hkv, groups, n_q, T, w_len = 2, 2, 4, 2, 4608, 70
    K, V, q = _rand(B, Hkv, T + w_len, groups, n_q, Dd, seed=Dd + 31)
    c = Call(pkg, K, V, T, n_q, groups, cap=128)
    runs, bpw = c.runs()
    assert (runs, bpw) == (72, 1) and runs + (c.cap + 63) // 64 > 64
    out, lse = c.call(q)
    _assert_models(out, lse, q, c.Kp, c.Vp, T + w_len - n_q, groups, f"D={Dd} {runs} runs + 2 chunks")
    # On random data every slab's maximum is much the same, and the fold is the same sum under any maximum that does not overflow.  So:
    # needles of twice the level on the first and last token of runs 64 .. 71.  Their x stands more than 88 above everything in the
    # first 64 slabs: a maximum taken over those alone makes exp() overflow.
    pos = np.zeros((B, Hkv * groups, n_q), np.int64)
    late = [t for b in range(64, 72) for t in (64 * b, 64 * b + 63)]
    for i, idx in enumerate(np.ndindex(*pos.shape)):
        pos[idx] = late[i % len(late)]
    K, V, q, w = needle_data(Dd, B, Hkv, groups, n_q, T + w_len, pos, T, seed=Dd + 32, boost=2)
    assert su.needle_x(Dd, w, 2) - su.other_x_max(Dd, w) > 88.8   # (exp(88.73) is the first fp32 infinity)
    out, lse = Call(pkg, K, V, T, n_q, groups, cap=128).call(q)
    _assert_needles(out, lse, V, pos, T, groups, Dd, w, f"D={Dd} needles in runs 64 .. 71", boost=2)


@pytest.mark.parametrize("Dd", [64, 128])
def test_the_largest_window(pkg, Dd):
    """window_len = capacity = 1024, the library's limit: sixteen chunks, every one of them full."""
    B, Hkv, groups, n_q, T, w_len = 2, 2, 4, 8, 64, 1024
    K, V, q = _rand(B, Hkv, T + w_len, groups, n_q, Dd, seed=Dd + 37)
    c = Call(pkg, K, V, T, n_q, groups, cap=1024)
    assert c.w_len == c.cap == 1024 and c.runs() == (1, 1)
    assert pkg[0].mustafar_decode_multi_query_workspace_bytes(T, 1025, B * Hkv, groups, n_q, Dd) == 0   # (1024 is the limit)
    out, lse = c.call(q)
    _assert_models(out, lse, q, c.Kp, c.Vp, T + w_len - n_q, groups, f"D={Dd} window 1024")
