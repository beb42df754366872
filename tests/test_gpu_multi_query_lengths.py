"""GPU: device-side lengths in the several-token decode call (ABI 115: mustafar_decode_multi_query_lengths,
MustafarAttention.decode_multi(step_counter=, t_device=, t_capacity=)): one graph of the call replayed while the window and the compressed
cache grow.

Comparators as in tests/test_gpu_multi_query.py: needles (exact), the float64 models of tests/exact_data.py and tests/partial_util.py with
their derived bounds, and the eager call (bit for bit where the same instantiation-independent work is done: the window buffers, and the
outputs at *T_device == T; within twice the model's bound elsewhere).  Batch 2, 2 kv heads.

The C-level cases come first and build their own extent tables: every entry points at valid memory, and the entries at or beyond
*T_device point at a DECOY extent whose keys would win every softmax, so a read past the limit shows as a wrong needle, not as a fault.
The Python-route cases, whose unlisted table entries are zero, follow."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import multi_mask_util as mm
from tests import test_gpu_multi_query as mq
from tests.hd64_util import DEV, S, _cache, oracle_prune

pytestmark = pytest.mark.gpu
NAN = float("nan")
T_BASE, T_CAP = 256, 768
B, HKV, GROUPS = 2, 2, 4
GUARD = 64          # rows behind the last head's window, which no call may touch
SENTINEL = 3.0


@pytest.fixture(scope="module")
def pkg():
    from mustafar_amd import _lib, compression
    return _lib.load(), compression


def _view(c):
    from mustafar_amd import _lib
    return _lib.CacheView(c[0].data_ptr(), c[2].data_ptr(), c[1].data_ptr(), c[3].data_ptr(), 0, 0, 0)


def _table(caches):
    """A device table of mustafar_cache_view, one entry per cache (offsets relative to the extent, strides 0: exactly 4 blocks' tiles)."""
    from mustafar_amd import _lib
    n = ctypes.sizeof(_lib.CacheView)
    raw = b"".join(ctypes.string_at(ctypes.byref(_view(c)), n) for c in caches)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)


_DECOYS = {}


def _decoy(pkg, Dd):
    """An extent of 256 tokens per head whose every key channel is 256 and every value 1.5: against a needle query (8 on a slot of w
    channels) its x is 2048 w / sqrt(D), at least twice any needle's; finite everywhere."""
    if Dd not in _DECOYS:
        k = torch.full((B * HKV, 256, Dd), 256.0, dtype=torch.float16, device=DEV)
        _DECOYS[Dd] = (_cache(k, "key", pkg[1]), _cache(torch.full_like(k, 1.5), "value", pkg[1]))
    return _DECOYS[Dd]


class LenCall:
    """Operands of one mustafar_decode_multi_query_lengths call over K / V [B, Hkv, t_used + w_len, D]: rows [0, 256) are the base view,
    rows [256, t_used) real extents of 256 tokens, the table entries from t_used up to the capacity of 768 tokens decoys; the window rows
    and the new rows as in mq.Call, the windows in ONE allocation with GUARD rows of SENTINEL behind the last head's window."""

    def __init__(self, pkg, K, V, t_used, n_q, cap, ks=S, vs=S):
        self.L = pkg[0]
        Dd = K.shape[3]
        assert t_used in (256, 512, 768) and K.shape[:2] == (B, HKV)
        self.t_used, self.n_q, self.Dd = t_used, n_q, Dd
        cut = lambda x: torch.cat([x[:, :, :T_BASE], x[:, :, t_used:]], 2)
        self.c = c = mq.Call(pkg, cut(K), cut(V), T_BASE, n_q, GROUPS, cap=cap, ks=ks, vs=vs)
        self.w_len, self.cap = c.w_len, c.cap
        Kx, Vx = oracle_prune(K[:, :, T_BASE:t_used], ks), oracle_prune(V[:, :, T_BASE:t_used], vs)
        self.Kp = torch.cat([c.Kp[:, :, :T_BASE], Kx, K[:, :, t_used:]], 2)
        self.Vp = torch.cat([c.Vp[:, :, :T_BASE], Vx, V[:, :, t_used:]], 2)
        dk, dv = _decoy(pkg, Dd)
        self.keep, ks_, vs_ = [], [], []
        for i in range((T_CAP - T_BASE) // 256):
            if T_BASE + 256 * i < t_used:
                sl = slice(256 * i, 256 * (i + 1))
                ks_.append(_cache(Kx[:, :, sl].reshape(B * HKV, 256, Dd).contiguous(), "key", pkg[1]))
                vs_.append(_cache(Vx[:, :, sl].reshape(B * HKV, 256, Dd).contiguous(), "value", pkg[1]))
            else:
                ks_.append(dk)
                vs_.append(dv)
        self.keep = (ks_, vs_)
        self.kt, self.vt = _table(ks_), _table(vs_)
        rows = B * HKV * self.cap
        self.k_all = torch.full((rows + GUARD, Dd), SENTINEL, dtype=torch.float16, device=DEV)
        self.v_all = torch.full_like(self.k_all, SENTINEL)
        self.kw, self.vw = self.k_all[:rows].view(B, HKV, self.cap, Dd), self.v_all[:rows].view(B, HKV, self.cap, Dd)
        self.kw.copy_(c.kw)
        self.vw.copy_(c.vw)
        self.ws_bytes = self.L.mustafar_decode_multi_query_workspace_bytes(T_CAP, self.cap, B * HKV, GROUPS, n_q, Dd)
        self.ws = torch.full((self.ws_bytes // 4,), NAN, dtype=torch.float32, device=DEV)
        self.t_dev = torch.tensor([t_used], dtype=torch.int32, device=DEV)
        self.extra = torch.zeros(1, dtype=torch.int32, device=DEV)

    def spans(self):
        return mq._run_spans(self.L, T_CAP, self.cap, B * HKV, GROUPS, self.n_q, self.Dd)

    def slabs(self):
        """(o [slabs, B', R, D], ml [slabs, B', R, 2]) of the workspace."""
        R, n = self.n_q * GROUPS, self.ws_bytes // (B * HKV * self.n_q * GROUPS * (self.Dd + 2) * 4)
        cut = n * B * HKV * R * self.Dd
        return self.ws[:cut].view(n, B * HKV, R, self.Dd), self.ws[cut:].view(n, B * HKV, R, 2)

    def call(self, q, w_host=None, extra=None, t_dev=True, mask=None, hpm=1):
        """The lengths call: window_len = w_host on the host (default: the window's), `extra` in the device counter (None: NULL),
        *T_device = t_used (t_dev False: NULL, the launch over the base alone).  mask: a device view [planes, rows, >= columns]."""
        c, p = self.c, lambda t: t.data_ptr() if t is not None else None
        c.out.fill_(NAN)
        c.lse.fill_(NAN)
        if extra is not None:
            self.extra.fill_(extra)
        T = T_CAP if t_dev else T_BASE
        m = (None, 0, 0, 1, 1) if mask is None else (mask.data_ptr(), mask.stride(0), mask.stride(1), mask.shape[1], hpm)
        err = self.L.mustafar_decode_multi_query_lengths(
            torch.cuda.current_stream().cuda_stream, ctypes.byref(c.kv), ctypes.byref(c.vv), T_BASE, p(self.kt) if t_dev else None,
            p(self.vt) if t_dev else None, T, B * HKV, GROUPS, self.n_q, q.data_ptr(), self.kw.data_ptr(), self.vw.data_ptr(), p(c.kn), p(c.vn),
            self.w_len if w_host is None else w_host, self.cap, c.out.data_ptr(), c.lse.data_ptr(), self.ws.data_ptr(),
            ctypes.c_float(math.sqrt(self.Dd)), self.Dd, *m, self.extra.data_ptr() if extra is not None else None,
            self.t_dev.data_ptr() if t_dev else None)
        assert err == 0
        return c.out, c.lse

    def call_fixed(self, q):
        """The fixed-length call over the same tables, T = the capacity (only meaningful at t_used == the capacity)."""
        c = self.c
        out, lse = torch.full_like(c.out, NAN), torch.full_like(c.lse, NAN)
        err = self.L.mustafar_decode_multi_query(
            torch.cuda.current_stream().cuda_stream, ctypes.byref(c.kv), ctypes.byref(c.vv), T_BASE, self.kt.data_ptr(), self.vt.data_ptr(),
            T_CAP, B * HKV, GROUPS, self.n_q, q.data_ptr(), self.kw.data_ptr(), self.vw.data_ptr(), c.kn.data_ptr(), c.vn.data_ptr(), self.w_len,
            self.cap, out.data_ptr(), lse.data_ptr(), self.ws.data_ptr(), ctypes.c_float(math.sqrt(self.Dd)), self.Dd)
        assert err == 0
        return out, lse

    def guard_untouched(self):
        rows = B * HKV * self.cap
        return bool((self.k_all[rows:] == SENTINEL).all()) and bool((self.v_all[rows:] == SENTINEL).all())


# ---- 1. decoy tables: blocks at or beyond *T_device are not read ----------------------------------------------------------------------------
@pytest.mark.parametrize("t_used", [256, 512, 768])
@pytest.mark.parametrize("n_q", [3, 8, 13])
@pytest.mark.parametrize("Dd", [64, 128])
def test_blocks_beyond_the_device_length_are_not_read(pkg, Dd, n_q, t_used):
    """T_base = 256, capacity 768, *T_device = 256, 512, 768.  R = 12: two blocks per run, no straddle; R = 32: three, run 1 straddles
    base -> extent and, at 256, the limit (run 2 at 512); R = 52: five, run 0 straddles the limit at 256 and run 1 at 512 -- read off the
    workspace size.  Needles on the
    edges of the base and of the extents in use, the window and the own rows: exact, with the host window length at its minimum and the
    rest in the device counter.  The slabs of a run with no block in use: weight zero.  Random data: the models.  At *T_device == T:
    the bits of the fixed-length call."""
    w0 = 5
    ntb = t_used // 64
    targets = [0, 63, 64, 255] + ([256, 319, t_used - 256, t_used - 1] if t_used > 256 else []) + [t_used, t_used + w0 - 1]
    pos = np.zeros((B, HKV * GROUPS, n_q), np.int64)
    k = 0
    for b, h, j in np.ndindex(*pos.shape):
        if (h + j) % 2 == 0:
            pos[b, h, j] = t_used + w0 + j
        else:
            pos[b, h, j] = targets[k % len(targets)]
            k += 1
    K, V, q, w = mq.needle_data(Dd, B, HKV, GROUPS, n_q, t_used + w0 + n_q, pos, t_used, seed=Dd + t_used + n_q)
    c = LenCall(pkg, K, V, t_used, n_q, cap=64)
    spans = c.spans()
    bpw = {3: 2, 8: 3, 13: 5}[n_q]
    assert spans[0] == (0, bpw) and len(spans) == -(-12 // bpw)
    straddle = [i for i, (b0, b1) in enumerate(spans) if b0 < ntb < b1]
    assert straddle == {(8, 256): [1], (8, 512): [2], (13, 256): [0], (13, 512): [1]}.get((n_q, t_used), [])   # (R = 12: none)
    out, lse = c.call(q, w_host=n_q, extra=w0)
    mq._assert_needles(out, lse, V, pos, t_used, GROUPS, Dd, w, f"D={Dd} R={n_q * GROUPS} *T={t_used}")
    o, ml = c.slabs()
    for i, (b0, _) in enumerate(spans):
        if b0 >= ntb:   # no block in use
            assert (o[i] == 0).all() and (ml[i, :, :, 0] == -math.inf).all() and (ml[i, :, :, 1] == 0).all(), f"run {i}: not a slab of weight zero"
        else:
            assert (ml[i, :, :, 1] > 0).all(), f"run {i} left no weight"
    assert c.guard_untouched()
    # random data against the models (a decoy read would be off by far more than any bound)
    K, V, q = mq._rand(B, HKV, t_used + w0 + n_q, GROUPS, n_q, Dd, seed=Dd + t_used + n_q + 1)
    c = LenCall(pkg, K, V, t_used, n_q, cap=64)
    out, lse = c.call(q, w_host=n_q + 2, extra=w0 - 2)
    mq._assert_models(out, lse, q, c.Kp, c.Vp, t_used + w0, GROUPS, f"D={Dd} R={n_q * GROUPS} *T={t_used}")
    if t_used == T_CAP:
        out, lse = out.clone(), lse.clone()
        out0, lse0 = c.call_fixed(q)
        assert torch.equal(mq._bits(out), mq._bits(out0)) and torch.equal(mq._bits(lse), mq._bits(lse0))


# ---- 2. the window length from the device ---------------------------------------------------------------------------------------------------
def _window_step(pkg, K, V, q, T, w, cap, n_q, Dd, extra_over=0):
    """The call at a window of `w` rows, eagerly (mq.Call) and with window_len = 57 on the host and the rest (+ extra_over) in the device
    counter, the windows of the second in a guarded allocation.  Returns (out, lse, eager out, eager lse, call, first)."""
    e = mq.Call(pkg, K[:, :, :T + w], V[:, :, :T + w], T, n_q, GROUPS, cap=cap)
    out0, lse0 = e.call(q)
    rows = B * HKV * cap
    k_all = torch.full((rows + GUARD, Dd), SENTINEL, dtype=torch.float16, device=DEV)
    v_all = torch.full_like(k_all, SENTINEL)
    d = mq.Call(pkg, K[:, :, :T + w], V[:, :, :T + w], T, n_q, GROUPS, cap=cap)
    kw, vw = k_all[:rows].view(B, HKV, cap, Dd), v_all[:rows].view(B, HKV, cap, Dd)
    kw.copy_(d.kw)
    vw.copy_(d.vw)
    extra = torch.tensor([w - 57 + extra_over], dtype=torch.int32, device=DEV)
    err = pkg[0].mustafar_decode_multi_query_lengths(
        torch.cuda.current_stream().cuda_stream, ctypes.byref(d.kv), ctypes.byref(d.vv), T, None, None, T, B * HKV, GROUPS, n_q, q.data_ptr(),
        kw.data_ptr(), vw.data_ptr(), d.kn.data_ptr(), d.vn.data_ptr(), 57, cap, d.out.data_ptr(), d.lse.data_ptr(), d.ws.data_ptr(),
        ctypes.c_float(math.sqrt(Dd)), Dd, None, 0, 0, 1, 1, extra.data_ptr(), None)
    assert err == 0
    torch.cuda.synchronize()
    # the window buffers bit for bit, every row outside [w - n_q, w) included; the guard rows as they were
    assert torch.equal(mq._bits(kw), mq._bits(e.kw)) and torch.equal(mq._bits(vw), mq._bits(e.vw)), f"w={w}: the windows differ from the eager call's"
    assert bool((k_all[rows:] == SENTINEL).all()) and bool((v_all[rows:] == SENTINEL).all()), f"w={w}: a guard row was written"
    return d.out, d.lse, out0, lse0, e


@pytest.mark.parametrize("cap", [72, 128])
@pytest.mark.parametrize("Dd", [64, 128])
def test_the_window_length_comes_from_the_device(pkg, Dd, cap):
    """window_len + counter walks 57 .. 72 at n_q = 8: across the chunk edge at 64 and through the rows that see nothing of the second
    chunk; then the capacity itself, and a counter that overshoots it by 5: the result of w = capacity, the guard rows untouched."""
    n_q, T = 8, 64
    K, V, q = mq._rand(B, HKV, T + cap, GROUPS, n_q, Dd, seed=Dd + cap)
    for w, over in [(w, 0) for w in range(57, 73)] + [(cap, 0), (cap, 5)]:
        out, lse, out0, lse0, e = _window_step(pkg, K, V, q, T, w, cap, n_q, Dd, extra_over=over)
        what = f"D={Dd} cap={cap} w={w}{' overshoot' if over else ''}"
        mq._assert_models(out, lse, q, e.Kp, e.Vp, T + w - n_q, GROUPS, what)
        mq._within_twice_the_bound(out, out0, q, e.Kp, e.Vp, T + w - n_q, GROUPS)


# ---- 3. the mask's window columns follow the tokens in use ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["left-pad", "tree"])
@pytest.mark.parametrize("Dd", [64, 128])
def test_mask_window_columns_sit_at_the_tokens_in_use(pkg, Dd, kind):
    """*T_device = 512 of a capacity of 768: window row w reads column 512 + w.  The columns 768 + w hold finfo.min -- a kernel that takes
    the capacity as the column base masks the whole window --, the columns between and behind hold NaN: never read."""
    n_q, t_used, w0, cap = 8, 512, 5, 64
    w_len = w0 + n_q
    K, V, q = mq._rand(B, HKV, t_used + w_len, GROUPS, n_q, Dd, seed=Dd + 3)
    c = LenCall(pkg, K, V, t_used, n_q, cap=cap)
    if kind == "left-pad":
        m = mm.left_padding([0, 300], t_used + w_len)             # 300: inside the extent in use
    else:
        gen = torch.Generator().manual_seed(Dd)
        m = mm.tree_mask(B, mm.random_tree(n_q, gen), t_used + w0, [[3, 255, 256, 300, 511], [0, 64, 400, t_used + 2]])
    phys = torch.full((B, m.shape[1], T_CAP + cap), NAN, dtype=torch.float16)
    phys[:, :, :t_used + w_len] = m
    phys[:, :, T_CAP:T_CAP + w_len] = mm.NEG
    dev = mm.housed(phys)
    out, lse = c.call(q, w_host=n_q, extra=w0, mask=dev, hpm=HKV)
    mask4 = mm.per_head(dev[:, :, :t_used + w_len], B, HKV * GROUPS, HKV * GROUPS)
    mm.assert_models(out, lse, q, c.Kp, c.Vp, t_used + w0, GROUPS, mask4, f"D={Dd} {kind}")


# ---- 4. the hook: one graph replayed through a speculative loop across two triggers --------------------------------------------------------
#      rejected drafts per round, cycled; a round asks for four tokens
REJECTS = [0, 1, 0, 3, 0, 0, 2, 0]
KINDS = [("arena", 128), ("ext64", 64), ("list", 128), ("list", 64)]


def _loop(attn, kind, K, V, q, Kd, Vd, qd, L0, rounds, replayed, pruned):
    """`rounds` rounds of decode_multi(4 tokens) + accept(rejected) from a prefill of L0 rows.  replayed: ONE captured graph of the call
    serves every round whose four tokens fit in front of a trigger point (a list cache, whose arrays a trigger replaces, is captured
    again behind each trigger); the others run eagerly with the tokens that fit.  Every round is checked against the models.  Returns
    (past, [(outputs of the kept tokens, compressed length, kv length) of every round], graph rounds, triggers, signature before,
    signature after)."""
    n_q, groups = 4, GROUPS
    past = mq._past(attn, K, V, L0)
    C0 = past[4]
    growing = kind != "list"
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    t_dev = torch.tensor([C0], dtype=torch.int32, device=DEV)
    gq, gk, gv = (torch.zeros((B, h, n_q, attn.head_dim), dtype=torch.float16, device=DEV) for h in (HKV * groups, HKV, HKV))
    lengths = dict(step_counter=counter, t_device=t_dev, t_capacity=C0 + 512) if growing else dict(step_counter=counter)
    graph = g_out = g_lse = None

    def capture():
        nonlocal graph, g_out, g_lse
        counter.zero_()
        warm = (past[0], past[1].clone(), past[2], past[3].clone(), past[4], past[5])
        attn.decode_multi(gq, gk, gv, warm, return_lse=True, **lengths)   # (module load and lazy state outside the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            g_out, g_lse, _ = attn.decode_multi(gq, gk, gv, past, return_lse=True, **lengths)

    sig = lambda p: (p[0].signature(), p[2].signature(), p[1].buf.data_ptr(), p[3].buf.data_ptr()) if growing else \
        (p[1].buf.data_ptr(), p[3].buf.data_ptr())
    if replayed:
        capture()
    before = sig(past)
    n, outs, on_graph, triggers = L0, [], 0, 0
    for i in range(rounds):
        fit = attn.fits_before_trigger(past, n_q)
        rej = min(REJECTS[i % len(REJECTS)], fit - 1)
        keep = fit - rej
        sl = slice(n - L0, n - L0 + keep)
        qs = torch.cat([q[:, :, sl], qd[:, :, :rej]], 2).contiguous()
        ks = torch.cat([K[:, :, n:n + keep], Kd[:, :, :rej]], 2)
        vs = torch.cat([V[:, :, n:n + keep], Vd[:, :, :rej]], 2)
        C = past[4]
        if replayed and fit == n_q:
            gq.copy_(qs); gk.copy_(ks); gv.copy_(vs)
            graph.replay()
            a, la = g_out.clone(), g_lse.clone()
            past = attn.advance(past, n_q)
            on_graph += 1
        else:
            a, la, past = attn.decode_multi(qs, ks, vs, past, return_lse=True)
        past = attn.accept(past, rejected=rej)
        counter.add_(keep)
        if past[4] != C:                      # the trigger ran (eagerly, inside accept): the windows slid, the cache grew
            triggers += 1
            t_dev.add_(256)
            counter.sub_(256)
            if replayed and not growing:
                capture()
        mq._assert_models(a[:, :, :keep], la[:, :, :keep], qs[:, :, :keep], *pruned[C], n, groups,
                          f"{kind} round {i} ({'graph' if replayed and fit == n_q else 'eager'}, kv {n}, compressed {C})")
        outs.append((a[:, :, :keep], C, n))
        n += keep
        assert past[5] == n and past[1].len == past[3].len == n - past[4]
    return past, outs, on_graph, triggers, before, sig(past)


@pytest.mark.parametrize("kind,Dd", KINDS, ids=[f"{k}-{d}" for k, d in KINDS])
def test_one_graph_through_a_speculative_loop_across_two_triggers(kind, Dd):
    """A prefill of 256 + 250 rows (38 rows short of the first trigger), rounds of four tokens with 0 .. 3 of them rejected until two
    triggers have run.  The replayed loop against the same loop run eagerly: every round within twice the model's bound of the other,
    the final caches and windows bit for bit, the caches' signatures and the windows' addresses as they were at the capture."""
    L0, rounds = 256 + 250, 100
    attn = mq._attn(kind, Dd=Dd)
    total = L0 + 4 * rounds
    K, V, q = mq._rand(B, HKV, total, GROUPS, total - L0, attn.head_dim, seed=Dd + 51)
    Kd, Vd, qd = mq._rand(B, HKV, 4, GROUPS, 4, attn.head_dim, seed=Dd + 52)
    pruned = {C: mq._pruned(attn, K, V, C) for C in (256, 512, 768)}
    pa, oa, on_graph, trig_a, before, after = _loop(attn, kind, K, V, q, Kd, Vd, qd, L0, rounds, True, pruned)
    pb, ob, _, trig_b, _, _ = _loop(mq._attn(kind, Dd=Dd), kind, K, V, q, Kd, Vd, qd, L0, rounds, False, pruned)
    assert trig_a == trig_b == 2 and pa[4] == pb[4] == 768 and pa[5] == pb[5]
    assert on_graph >= rounds - 8, f"only {on_graph} of {rounds} rounds ran on the graph"
    assert before == after, "a cache signature or a window address changed under the graph"
    for (a, C, n), (b, Cb, nb) in zip(oa, ob):
        assert (C, n, a.shape) == (Cb, nb, b.shape)
        mq._within_twice_the_bound(a, b, q[:, :, n - L0:n - L0 + a.shape[2]], *pruned[C], n, GROUPS)
    assert pa[1].len == pb[1].len and pa[3].len == pb[3].len
    assert torch.equal(mq._bits(pa[1].view()), mq._bits(pb[1].view())) and torch.equal(mq._bits(pa[3].view()), mq._bits(pb[3].view()))
    assert mq._same_cache(pa[0], pb[0]) and mq._same_cache(pa[2], pb[2])
