"""Operands of the ragged decode call (mustafar_ragged_set_sequences + mustafar_decode_ragged) for tests/test_gpu_ragged.py, built as
tests/test_gpu_multi_query.py builds its `Call`: the first T rows of a sequence oracle-pruned and converted through the package, extents
as device tables of views, every unused window row NaN, out / lse / the whole workspace pre-filled with NaN, table entries of extents not
in use all zero.  The float64 recipe of that file's `_model_ratios` is restated here (tests/exact_data.hook_model for out,
tests/partial_util.lse_model with lse_ratio for lse)."""
import ctypes
import math

import torch

from tests import exact_data as xd
from tests import partial_util as pu
from tests.hd64_util import DEV, S, _cache, oracle_prune

NAN = float("nan")
T_BASE = 256          # tokens of a base view; everything beyond it lies in 256-token extents


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def view_of(c):
    from mustafar_amd import _lib
    return _lib.CacheView(c[0].data_ptr(), c[2].data_ptr(), c[1].data_ptr(), c[3].data_ptr(), 0, 0, 0)


def write_views(table, first, caches):
    """Entries [first, first + len(caches)) of a device table of mustafar_cache_view <- the views of `caches` (strides 0, offsets
    relative to the extent)."""
    from mustafar_amd import _lib
    n = ctypes.sizeof(_lib.CacheView)
    raw = b"".join(ctypes.string_at(ctypes.byref(view_of(c)), n) for c in caches)
    table[first * n:first * n + len(raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)


class Seq:
    """One sequence of `Hkv` kv heads: K / V [1, Hkv, T + w_len, D], rows [0, T) compressed -- [0, 256) a base view, the rest extents of
    256 listed in device tables of `entries` entries (those not in use stay zero) --, rows [T, T + w_len - n_q) in windows of `cap`
    rows, the last n_q rows the call's new rows.  Nothing here changes after construction: calls run on copies of the windows."""

    def __init__(self, pkg, Dd, Hkv, groups, n_q, T, w_len, cap, seed, entries=None):
        L_, comp = pkg
        assert T % 256 == 0 and n_q <= w_len <= cap
        self.L, self.comp = L_, comp
        self.Dd, self.Hkv, self.groups, self.n_q, self.T, self.w_len, self.cap = Dd, Hkv, groups, n_q, T, w_len, cap
        g = torch.Generator(device=DEV).manual_seed(seed)
        Ltot = T + w_len
        self.K = torch.randn((1, Hkv, Ltot, Dd), generator=g, device=DEV).half()
        self.V = torch.randn((1, Hkv, Ltot, Dd), generator=g, device=DEV).half()
        self.q = torch.randn((1, Hkv * groups, n_q, Dd), generator=g, device=DEV).half()
        self.Kp, self.Vp = self.K.clone(), self.V.clone()
        self.T_base = min(T, T_BASE)
        n_ext = (T - self.T_base) // 256
        self.entries = max(entries or 0, n_ext)
        self.kt = torch.zeros(max(self.entries, 1) * 64, dtype=torch.uint8, device=DEV)
        self.vt = torch.zeros_like(self.kt)
        self.caches = []   # (keeps the arrays the views name)
        if T:
            self.Kp[:, :, :T], self.Vp[:, :, :T] = oracle_prune(self.K[:, :, :T], S), oracle_prune(self.V[:, :, :T], S)
            self.kc, self.vc = self.compress(0, self.T_base)
            self.kv, self.vv = view_of(self.kc), view_of(self.vc)
            for i in range(n_ext):
                self.list_extent(i)
        self.kw = torch.full((Hkv, cap, Dd), NAN, dtype=torch.float16, device=DEV)
        self.vw = torch.full_like(self.kw, NAN)
        w0 = w_len - n_q
        self.kw[:, :w0], self.vw[:, :w0] = self.K[0, :, T:T + w0], self.V[0, :, T:T + w0]
        self.kn, self.vn = self.K[:, :, Ltot - n_q:].contiguous(), self.V[:, :, Ltot - n_q:].contiguous()

    def compress(self, t0, t1):
        """Rows [t0, t1) of the pruned K / V as a pair of reference-layout caches of their own."""
        k = _cache(self.Kp[0, :, t0:t1].contiguous(), "key", self.comp)
        v = _cache(self.Vp[0, :, t0:t1].contiguous(), "value", self.comp)
        self.caches.append((k, v))
        return k, v

    def list_extent(self, i):
        """Tokens [256 + 256 i, 256 + 256 (i + 1)) become entry i of both tables."""
        k, v = self.compress(T_BASE + 256 * i, T_BASE + 256 * (i + 1))
        write_views(self.kt, i, [k])
        write_views(self.vt, i, [v])

    def stored_windows(self):
        """Copies of the windows with the new rows already in place."""
        kw, vw, w0 = self.kw.clone(), self.vw.clone(), self.w_len - self.n_q
        kw[:, w0:self.w_len], vw[:, w0:self.w_len] = self.kn[0], self.vn[0]
        return kw, vw

    def item(self, kw, vw, T=None, w_len=None):
        """The `mustafar_sequence` of this sequence over the windows `kw` / `vw` (default lengths: its own)."""
        from mustafar_amd import _lib
        T = self.T if T is None else T
        it = _lib.Sequence()
        if T:
            it.k_base, it.v_base = self.kv, self.vv
        if T > self.T_base:
            it.k_extents, it.v_extents = self.kt.data_ptr(), self.vt.data_ptr()
        it.k_window, it.v_window = kw.data_ptr(), vw.data_ptr()
        it.T_base, it.T, it.window_len, it.window_capacity = min(T, self.T_base), T, self.w_len if w_len is None else w_len, self.cap
        return it

    def solo(self):
        """mustafar_decode_multi_query on this sequence alone, on fresh copies of the windows -> (out [1, H, n_q, D], lse, kw, vw)."""
        kw, vw = self.kw.clone(), self.vw.clone()
        H = self.Hkv * self.groups
        ws_bytes = self.L.mustafar_decode_multi_query_workspace_bytes(self.T, self.cap, self.Hkv, self.groups, self.n_q, self.Dd)
        assert ws_bytes > 0
        ws = torch.full((ws_bytes // 4,), NAN, dtype=torch.float32, device=DEV)
        out = torch.full((1, H, self.n_q, self.Dd), NAN, dtype=torch.float16, device=DEV)
        lse = torch.full((1, H, self.n_q), NAN, dtype=torch.float32, device=DEV)
        ext = self.T > self.T_base
        err = self.L.mustafar_decode_multi_query(
            torch.cuda.current_stream().cuda_stream, ctypes.byref(self.kv) if self.T else None, ctypes.byref(self.vv) if self.T else None,
            self.T_base, self.kt.data_ptr() if ext else None, self.vt.data_ptr() if ext else None, self.T, self.Hkv, self.groups, self.n_q,
            self.q.data_ptr(), kw.data_ptr(), vw.data_ptr(), self.kn.data_ptr(), self.vn.data_ptr(), self.w_len, self.cap, out.data_ptr(),
            lse.data_ptr(), ws.data_ptr(), ctypes.c_float(math.sqrt(self.Dd)), self.Dd)
        assert err == 0
        return out, lse, kw, vw

    def model_ratios(self, out, lse):
        """max |out - hook_model| / bound and |lse - lse_model| / bound over the tokens: token j sees rows [0, T + w_len - n_q + j + 1) of
        Kp / Vp (pruned where compressed)."""
        first = self.T + self.w_len - self.n_q
        r_out = r_lse = 0.0
        for j in range(self.n_q):
            Lj = first + j + 1
            want, bound = xd.hook_model(self.q[:, :, j:j + 1], self.Kp[:, :, :Lj], self.Vp[:, :, :Lj], self.groups)
            r = (out[:, :, j:j + 1].double() - want).abs() / bound
            r_out = max(r_out, float(r.max()) if torch.isfinite(r).all() else float("inf"))
            want_l, bound_l = pu.lse_model(self.q[:, :, j:j + 1], self.Kp[:, :, :Lj], self.groups)
            r_lse = max(r_lse, pu.lse_ratio(lse[:, :, j], want_l, bound_l))
        return r_out, r_lse


class Batch:
    """A device table of `capacity` entries and the operands of mustafar_decode_ragged over it: q / k_new / v_new / out / lse of `capacity`
    slots, the workspace sized for (T_max, cap_max), all of it NaN until a call writes it."""

    def __init__(self, pkg, capacity, Dd, Hkv, groups, n_q, T_max, cap_max):
        from mustafar_amd import _lib
        self.L = pkg[0]
        self.n, self.Dd, self.Hkv, self.groups, self.n_q, self.T_max, self.cap_max = capacity, Dd, Hkv, groups, n_q, T_max, cap_max
        H = Hkv * groups
        self.table = torch.zeros(capacity * ctypes.sizeof(_lib.Sequence), dtype=torch.uint8, device=DEV)
        self.q = torch.zeros((capacity, H, n_q, Dd), dtype=torch.float16, device=DEV)
        self.kn = torch.zeros((capacity, Hkv, n_q, Dd), dtype=torch.float16, device=DEV)
        self.vn = torch.zeros_like(self.kn)
        self.out = torch.full((capacity, H, n_q, Dd), NAN, dtype=torch.float16, device=DEV)
        self.lse = torch.full((capacity, H, n_q), NAN, dtype=torch.float32, device=DEV)
        ws_bytes = self.L.mustafar_decode_ragged_workspace_bytes(T_max, cap_max, capacity, Hkv, groups, n_q, Dd)
        assert ws_bytes > 0
        self.ws = torch.full((ws_bytes // 4,), NAN, dtype=torch.float32, device=DEV)

    def set(self, first, items):
        """mustafar_ragged_set_sequences: entries [first, first + len(items)) <- items (None: an empty slot, all zero)."""
        from mustafar_amd import _lib
        arr = (_lib.Sequence * len(items))(*[it if it is not None else _lib.Sequence() for it in items])
        err = self.L.mustafar_ragged_set_sequences(torch.cuda.current_stream().cuda_stream, self.table.data_ptr(), first, len(items), arr,
                                                   self.Hkv, self.n_q, self.Dd)
        assert err == 0

    def load(self, slot, seq):
        """q and the new rows of `seq` into the operands of `slot`."""
        self.q[slot], self.kn[slot], self.vn[slot] = seq.q[0], seq.kn[0], seq.vn[0]

    def decode(self, out=None, lse=None, stored=False):
        """mustafar_decode_ragged over the whole table into out / lse (default: the batch's own, NaN before the call)."""
        out, lse = self.out if out is None else out, self.lse if lse is None else lse
        err = self.L.mustafar_decode_ragged(
            torch.cuda.current_stream().cuda_stream, self.table.data_ptr(), self.n, self.Hkv, self.groups, self.n_q, self.T_max, self.cap_max,
            self.q.data_ptr(), None if stored else self.kn.data_ptr(), None if stored else self.vn.data_ptr(), out.data_ptr(),
            lse.data_ptr(), self.ws.data_ptr(), ctypes.c_float(math.sqrt(self.Dd)), self.Dd)
        assert err == 0
        return out, lse


def run_slots(pkg, seqs, slots, stored=False):
    """One ragged call over `slots` (indices into `seqs`, None: an empty slot with every pointer NULL), each sequence on fresh copies of
    its windows -> (out, lse, {slot: (kw, vw)})."""
    s0 = seqs[0]
    b = Batch(pkg, len(slots), s0.Dd, s0.Hkv, s0.groups, s0.n_q, max(s.T for s in seqs), max(s.cap for s in seqs))
    wins, items = {}, []
    for slot, i in enumerate(slots):
        if i is None:
            items.append(None)
            continue
        s = seqs[i]
        wins[slot] = s.stored_windows() if stored else (s.kw.clone(), s.vw.clone())
        items.append(s.item(*wins[slot]))
        b.load(slot, s)
    b.set(0, items)
    out, lse = b.decode(stored=stored)
    torch.cuda.synchronize()
    return out, lse, wins
