"""The head_dim-64 compressed cache that grows by extents (MustafarConfig(hd64_extents=True)), and the head_dim-64 prefill compressed
from the raw rows (MustafarConfig(hd64_raw_prefill=True): `compress_raw_pair_hd64`, which shares the extent layout and the gather launch).

At D = 64 the cache is the reference's tuple `[bitmaps, idxs, nzs, nz_offset]`, and the reference's 256-token trigger re-copies all of
it (`reflayout.append_compressed`: a `torch.cat` per array and head), so every array moves and a captured decode graph dies with every
trigger.  `ExtentCache64` keeps one side (K or V) of one layer the way `CompressedArena` keeps it at D = 128 once extents are on:

  * the BASE is the reference-layout arrays of the prefill, exactly as the two-pass conversion makes them.  Nothing is ever appended
    to it in place, so it needs no spare room and no strides;
  * a trigger compresses its 256 window rows into a small cache of their own, an EXTENT (mustafar_trigger_compress_batch_hd: one launch
    per layer from the raw rows), and lists the extent's view in a DEVICE table of `MAX_EXTENTS` mustafar_cache_view entries that
    the extents form of the fused decode call reads (`decode_args` / `view_args`: the cache protocol of reflayout.py).  The table is created with the cache -- before any graph can name it (a table created
    inside a capture would live in the graph's pool and be zero-filled again by every replay) -- and an entry is written once;
  * the extents of ONE trigger of ALL layers are carved from one pooled allocation (`ExtentPool64`) together with the layers' status
    words `[flag, K lengths, V lengths]`, which one copy brings to the host.  Regions are housed tight -- the base's measured halfs per
    token + 4 %, as cache.py does at D = 128; a worst-case region would be as large as the dense rows -- and a layer whose flag shows
    bit 0 (a head outgrew its region: rows full of ties) is redone on its own at the measured size before any window slides.

`to_reference()` concatenates base and extents the way the model appends (`reflayout.append_compressed`): the same tensors, bit for bit,
that the tuple path holds after the same triggers.  `consolidate()` (a full table: 512 extents are 128 k generated tokens) builds the
same cache on the device: the reference-layout arrays at exact size from the lengths the host already holds (`base_used`, every
extent's `used`), and ONE mustafar_cache_gather_hd launch over base + table that copies bitmaps, shifts offsets and moves every head's
stream into place -- one copy of the cache, nothing read back, every address new, so a captured graph must be taken again.
`consolidate(via_reference=True)` keeps the route through `to_reference()` (a `torch.cat` of the whole cache per extent) for comparison.
The same launch ends a prefill compressed from the raw rows in 256-token chunks (`compress_raw_pair_hd64`, below).
"""
from __future__ import annotations

import ctypes
from typing import List, Optional

import torch

from . import _lib
from .compression import _compress, _offsets_mirror, _stream_ptr, hd64_staging_region, pieces_of   # (hd64_staging_region: also this module's name for it)
from .reflayout import FlatStreams, ListCache, StatusPool, _round_up, append_compressed

D = 64
EXT_TOKENS = 256
VIEW_BYTES = ctypes.sizeof(_lib.CacheView)


def _head_lengths(idx: torch.Tensor, heads: int) -> torch.Tensor:
    """Every head's stream length in halfs, on the host (the last offset entry of its row, half2 units)."""
    return (idx.view(heads, -1)[:, -1].to(torch.int64) * 2).cpu()


class Extent64:
    """One 256-token extent of one side: views into a pool's storage (which they keep alive) + the heads' stream lengths."""

    def __init__(self, storage: torch.Tensor, heads: int, region_halfs: int):
        self.storage, self.heads, self.region = storage, heads, region_halfs
        off = ExtentPool64.layout(heads, region_halfs)[0]
        self.bmp = storage[off["bmp"]:off["bmp"] + heads * 256 * 8].view(torch.int64).view(heads, 256)
        self.idx = storage[off["idx"]:off["idx"] + heads * 257 * 4].view(torch.int32).view(heads, 257)
        self.nz_offset = storage[off["nz_offset"]:off["nz_offset"] + heads * 4].view(torch.int32)
        self.nz = storage[off["nz"]:off["nz"] + heads * region_halfs * 2].view(torch.float16).view(heads, region_halfs)
        self.view = _lib.CacheView(self.bmp.data_ptr(), self.nz.data_ptr(), self.idx.data_ptr(), self.nz_offset.data_ptr(), 256, 257,
                                   region_halfs // 8)
        self.used: Optional[torch.Tensor] = None   # int64 [heads] on the host, set when the trigger's status has been read

    def reference(self) -> list:
        """[bitmaps, idxs, per-head streams, None]: what `_compress` returns for these 256 tokens (append_compressed reads the first three)."""
        return [self.bmp.reshape(-1), self.idx.reshape(-1), FlatStreams([self.nz[h, :int(self.used[h])] for h in range(self.heads)]), None]


class ExtentPool64(StatusPool):
    """ONE allocation for the 2 x n extents of one trigger of n layers (K, V per layer; one region size) and the layers' status words
    (reflayout.StatusPool).  Only the status words are initialised (zeroed): the compression launch writes every other word it or the
    decode launch reads."""

    def __init__(self, n_layers: int, heads: int, device, region_halfs: int):
        assert region_halfs > 0 and region_halfs % 8 == 0
        super().__init__(n_layers, heads, device)
        self.region = region_halfs
        _, self.ext_bytes = self.layout(heads, region_halfs)
        ne = 2 * n_layers
        self.buf = torch.empty(ne * self.ext_bytes + n_layers * self.status_words * 8, dtype=torch.uint8, device=device)
        self._adopt_status(self.buf[ne * self.ext_bytes:])

    @staticmethod
    def layout(heads: int, region_halfs: int):
        off, pos = {}, 0
        for name, size in (("bmp", heads * 256 * 8), ("idx", heads * 257 * 4), ("nz_offset", heads * 4), ("nz", heads * region_halfs * 2)):
            off[name] = pos
            pos = _round_up(pos + size, 256)
        return off, pos

    def extent(self, j: int) -> Extent64:   # j = 2 * layer + side
        return Extent64(self.buf[j * self.ext_bytes:(j + 1) * self.ext_bytes], self.heads, self.region)


class ExtentCache64:
    MAX_EXTENTS = 512   # entries of the device table (the extents form of the fused decode call takes at most 512)
    lse_reads_tables = True   # a call with an LSE reads the extents form even over the base alone (hook._call_decode)

    def __init__(self, base: list, which: str, heads: int, tokens: int):
        """base: the reference-layout `[bitmaps, idxs, FlatStreams, nz_offset]` of `tokens` tokens (a multiple of 256)."""
        assert which in ("key", "value") and tokens > 0 and tokens % 256 == 0
        self.base, self.which, self.heads, self.tokens = base, which, heads, tokens
        self.device = base[0].device
        self.base_used = _head_lengths(base[1], heads)
        self._base = ListCache(base, tokens)   # (kept: it holds the flat stream and the view of the base)
        self.base_view = self._base.view
        self.table = torch.zeros(self.MAX_EXTENTS * VIEW_BYTES, dtype=torch.uint8, device=self.device)
        self.extents: List[Extent64] = []

    @property
    def total_tokens(self) -> int:
        return self.tokens + EXT_TOKENS * len(self.extents)

    def view_ptr(self):
        return ctypes.byref(self.base_view)

    def bytes_in_use(self) -> int:
        """Bytes of the four arrays of the base and of every extent."""
        return self._base.bytes_in_use() + \
            sum(self.heads * (256 * 8 + 257 * 4 + 4) + int(e.used.sum()) * 2 for e in self.extents)

    def view_args(self, v_cache: "ExtentCache64", tables: bool):
        """`(k_view_ptr, v_view_ptr, T_base, k_table, v_table)`, the tables null unless `tables`, and the tensors to keep until the call
        is issued (none: the caches own everything named)."""
        kt, vt = (self.table.data_ptr(), v_cache.table.data_ptr()) if tables else (None, None)
        return (self.view_ptr(), v_cache.view_ptr(), self.tokens, kt, vt), ()

    def decode_args(self, v_cache: "ExtentCache64", tables: bool):
        """How this K cache and its V cache arrive at a fused decode call (hook._call_decode): `view_args` when `tables`, else the
        eight arrays of the two bases (the plain D = 64 launch: the base alone)."""
        return self.view_args(v_cache, True) if tables else (self._base.decode_args(v_cache._base)[0], ())

    def slot_ptr(self, i: int) -> int:
        return self.table.data_ptr() + i * VIEW_BYTES

    def signature(self) -> tuple:
        """Addresses a captured decode graph holds for this cache (extents are found through the table at run time)."""
        return (self.base[0].data_ptr(), self.base[1].data_ptr(), self.base_view.nz, self.tokens, self.table.data_ptr())

    def expected_region(self) -> int:
        """Halfs a 256-token extent is expected to need in its fullest head: the base's measured halfs per token + 4 % (cache.py:
        `_expected_append`), a little room for padding, a multiple of 8."""
        per_token = float(self.base_used.max()) / self.tokens
        return _round_up(int(EXT_TOKENS * per_token * 1.04) + 256, 8)

    # ---- the trigger of all layers -----------------------------------------------------------------------------------------------
    @staticmethod
    def append_extents(pairs, rows, kth_k: int, kth_v: int, window_len: int) -> None:
        """pairs: [(k_cache, v_cache), ...] one per layer; rows: [(k_buf, v_buf), ...] the window buffers [B, Hkv, cap, 64] with
        `window_len` valid rows.  Rows [0, 256) of every buffer become an extent of its cache; both windows slide by 256 rows in place.
        One library call issues every layer's compression, one copy brings every flag and length, a layer that overflowed is redone on
        its own at the measured size, and only then one call lists the extents in the tables and slides the windows."""
        n = len(pairs)
        if n == 0:
            return
        k0 = pairs[0][0]
        H, dev = k0.heads, k0.device
        for (kc, vc), (kr, vr) in zip(pairs, rows):
            if len(kc.extents) >= kc.MAX_EXTENTS or len(kc.extents) != len(vc.extents) or kc.tokens != vc.tokens or kc.heads != H or vc.heads != H:
                raise RuntimeError("ExtentCache64.append_extents: extent table full (consolidate() first) or K / V out of step")
            if kr.shape != vr.shape or kr.dtype != torch.float16 or kr.dim() != 4 or kr.shape[0] * kr.shape[1] != H or kr.shape[3] != D or \
                    kr.shape[2] < window_len or window_len < 256 or not kr.is_contiguous() or not vr.is_contiguous() or kr.shape != rows[0][0].shape:
                raise RuntimeError("ExtentCache64.append_extents expects contiguous fp16 [B, Hkv, rows >= window_len >= 256, 64] buffers of one shape")
        L = _lib.load()
        head_stride = rows[0][0].shape[2] * D
        region = max(max(kc.expected_region(), vc.expected_region()) for kc, vc in pairs)
        pool = ExtentPool64(n, H, dev, region)

        def item(it, i, p, j):
            (kc, vc), (kr, vr) = pairs[i], rows[i]
            ek, ev = p.extent(2 * j), p.extent(2 * j + 1)
            it.k_window, it.v_window = kr.data_ptr(), vr.data_ptr()
            it.k_dst, it.v_dst = ek.view, ev.view
            it.k_table_slot, it.v_table_slot = kc.slot_ptr(len(kc.extents)), vc.slot_ptr(len(vc.extents))
            it.k_head_total, it.v_head_total, it.overflow_flag = p.totals_ptr(2 * j), p.totals_ptr(2 * j + 1), p.flag_ptr(j)
            return ek, ev

        items = (_lib.TriggerItem * n)()
        made = [item(items[i], i, pool, i) for i in range(n)]
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(L.mustafar_trigger_compress_batch_hd(st, n, items, head_stride, H, 256, D, kth_k, kth_v, region, region, None),
                       "mustafar_trigger_compress_batch_hd")
            host = pool.read_status().clone()
            for i in range(n):
                if not int(host[i, 0]) & 1:
                    continue
                # a head outgrew its region: this layer alone, at the length the launch measured (the raw rows are still in place)
                need = _round_up(int(host[i, 1:].max()), 8)
                own = ExtentPool64(1, H, dev, need)
                one = (_lib.TriggerItem * 1)()
                made[i] = item(one[0], i, own, 0)
                _lib.check(L.mustafar_trigger_compress_batch_hd(st, 1, one, head_stride, H, 256, D, kth_k, kth_v, need, need, None),
                           "mustafar_trigger_compress_batch_hd")
                again = own.read_status()
                if int(again[0, 0]) & 0xffffffff:
                    raise RuntimeError("ExtentCache64.append_extents: the repeat at the measured size overflowed: this is a bug")
                host[i] = again[0]
                items[i] = one[0]
            _lib.check(L.mustafar_trigger_finish_batch_hd(st, n, items, head_stride, H, window_len, 256, D), "mustafar_trigger_finish_batch_hd")
        for i, ((kc, vc), (ek, ev)) in enumerate(zip(pairs, made)):
            ek.used, ev.used = host[i, 1:1 + H].clone(), host[i, 1 + H:1 + 2 * H].clone()
            kc.extents.append(ek)
            vc.extents.append(ev)

    # ---- back to the reference layout ----------------------------------------------------------------------------------------------
    def to_reference(self) -> list:
        """`[bitmaps, idxs, FlatStreams, nz_offset]` of base + extents, built the way the model appends (reflayout.append_compressed)."""
        ref, tokens = self.base, self.tokens
        for e in self.extents:
            ref = append_compressed(ref, e.reference(), self.heads, tokens, EXT_TOKENS, D)
            tokens += EXT_TOKENS
        return ref

    def consolidate(self, via_reference: bool = False) -> "ExtentCache64":
        """One base holding everything (module docstring): exact-size arrays, one gather launch over base + table; new addresses, a new
        and empty table.  via_reference: through `to_reference()` instead (the same bits)."""
        if not self.extents:
            return self
        if via_reference or self.base_view.nz is None:   # (a base without any stream: nothing for the launch to align on)
            return type(self)(self.to_reference(), self.which, self.heads, self.total_tokens)
        T, H, dev = self.total_tokens, self.heads, self.device
        used = self.base_used.clone()
        for e in self.extents:
            used += e.used
        offs = [0] + torch.cumsum(used, 0).tolist()
        if offs[-1] // 8 > 0xffffffff:
            raise RuntimeError("ExtentCache64.consolidate: the packed stream exceeds what nz_offset (uint4 units, 32 bits) can address")
        bmp = torch.empty((H * T,), dtype=torch.int64, device=dev)
        idx = torch.empty((H * (T + 1),), dtype=torch.int32, device=dev)
        packed = torch.empty((offs[-1],), dtype=torch.float16, device=dev)
        nz_offset = torch.tensor([o // 8 for o in offs[:-1]], dtype=torch.int32, device=dev)
        dst = _lib.CacheView(bmp.data_ptr(), packed.data_ptr(), idx.data_ptr(), nz_offset.data_ptr(), 0, 0, 0)
        with torch.cuda.device(dev):
            err = _lib.load().mustafar_cache_gather_hd(torch.cuda.current_stream(dev).cuda_stream, dst, self.base_view, self.tokens,
                                                       self.table.data_ptr(), len(self.extents), H, D)
        _lib.check(err, "mustafar_cache_gather_hd")
        return type(self)([bmp, idx, FlatStreams(pieces_of(packed, offs), flat=packed), nz_offset], self.which, H, T)


# ---- a prefill compressed from the RAW rows (MustafarConfig(hd64_raw_prefill=True)) ---------------------------------------------------------
HD64_MAX_RAW_TOKENS = 512 * 256   # mustafar_prefill_compress_hd / mustafar_cache_gather_hd take at most 512 chunks
hd64_prefill_repeats = 0          # compression launches repeated at the measured region size (rows with ties at the threshold)


def _prune_kth_hd64(x: torch.Tensor, kth: int) -> torch.Tensor:
    """prune_magnitude with the k-th-smallest index given (0: the rows are pruned already)."""
    xc = x.contiguous()
    if xc.data_ptr() % 16:
        xc = xc.clone()
    if kth <= 0:
        return xc
    out = torch.empty_like(xc)
    with torch.cuda.device(x.device):
        err = _lib.load().mustafar_prune_magnitude(_stream_ptr(x.device), xc.data_ptr(), out.data_ptr(), xc.numel() // 64, 64, kth)
    _lib.check(err, "mustafar_prune_magnitude")
    return out


def compress_raw_pair_hd64(k: torch.Tensor, v: torch.Tensor, tokens: int, kth_k: int, kth_v: int):
    """Raw K / V [B, Hkv, L, 64] fp16 -> the reference-layout caches `[bitmaps, idxs, FlatStreams, nz_offset]` of the first `tokens` rows
    of every head (a multiple of 256): what `compression._compress(prune_magnitude(x[:, :, :tokens]).reshape(B', -1, 64), which)` returns, tensor
    for tensor, without a pruned copy and with ONE read of the rows and ONE host wait:
      1. mustafar_prefill_compress_hd: every 256-token chunk of every head becomes an extent of its own in a staging allocation;
      2. one copy of the flag and the chunk lengths to pinned memory and one wait (the return type needs the sizes);
      3. mustafar_cache_gather_hd per side: the chunks, offsets shifted, into the exact-size arrays.
    A chunk whose rows tie at the threshold keeps more than the staging bound: flag bit 0, and the launch is repeated ONCE at the
    measured maximum (counted in `hd64_prefill_repeats`).  More than 131072 tokens: the prune + two-pass route."""
    global hd64_prefill_repeats
    if k.shape != v.shape or k.dim() != 4 or k.shape[3] != 64 or k.dtype != torch.float16 or v.dtype != torch.float16 or not k.is_cuda:
        raise RuntimeError("compress_raw_pair_hd64 expects two float16 [B, Hkv, L, 64] tensors of one shape on the GPU")
    B, H, L, D = k.shape
    if tokens <= 0 or tokens % 256 or tokens > L or not 0 <= kth_k <= 64 or not 0 <= kth_v <= 64:
        raise RuntimeError("compress_raw_pair_hd64: tokens must be a positive multiple of 256 within the rows, kth within [0, 64]")
    Bp, n, dev = B * H, tokens // 256, k.device
    if tokens > HD64_MAX_RAW_TOKENS:
        return (_compress(_prune_kth_hd64(k[:, :, :tokens], kth_k).reshape(Bp, -1, D), "key"),
                _compress(_prune_kth_hd64(v[:, :, :tokens], kth_v).reshape(Bp, -1, D), "value"))
    k = k if k.is_contiguous() and k.data_ptr() % 16 == 0 else k.contiguous().clone()   # (a transpose(1, 2) view of [B, L, H, 64])
    v = v if v.is_contiguous() and v.data_ptr() % 16 == 0 else v.contiguous().clone()
    Lb = _lib.load()
    words = 1 + 2 * n * Bp   # status: [flag | K lengths [n][B'] | V lengths [n][B']]
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        st = stream.cuda_stream
        host = _offsets_mirror(dev, words - 1)[0]   # (pinned int64 [words], this thread's: a call has read it before it returns)

        def launch(region_k: int, region_v: int):
            (ok_, kb), (ov_, vb) = ExtentPool64.layout(Bp, region_k), ExtentPool64.layout(Bp, region_v)
            buf = torch.empty((n * (kb + vb) + 2 * n * VIEW_BYTES + words * 8,), dtype=torch.uint8, device=dev)
            tables = buf.data_ptr() + n * (kb + vb)
            status = buf[n * (kb + vb) + 2 * n * VIEW_BYTES:].view(torch.int64)
            status[0] = 0
            views = []
            for base, off, region in ((buf.data_ptr(), ok_, region_k), (buf.data_ptr() + n * kb, ov_, region_v)):
                views.append(_lib.CacheView(base + off["bmp"], base + off["nz"], base + off["idx"], base + off["nz_offset"], 256, 257, region // 8))
            err = Lb.mustafar_prefill_compress_hd(st, k.data_ptr(), v.data_ptr(), L * D, Bp, tokens, D, kth_k, kth_v, views[0], views[1], kb, vb,
                                                  tables, tables + n * VIEW_BYTES, status.data_ptr() + 8, status.data_ptr() + 8 * (1 + n * Bp),
                                                  region_k, region_v, status.data_ptr())
            _lib.check(err, "mustafar_prefill_compress_hd")
            host.copy_(status, non_blocking=True)   # the ONE copy + wait: flag and every chunk's lengths
            stream.synchronize()
            return buf, tables

        buf, tables = launch(hd64_staging_region(kth_k), hd64_staging_region(kth_v))
        if int(host[0]) & 1:   # a (head, chunk) outgrew its region: once more, at the measured maximum (the raw rows are still in place)
            hd64_prefill_repeats += 1
            lens = host[1:].view(2, n * Bp)
            need_k, need_v = ((int(lens[i].max()) + 7) // 8 * 8 for i in range(2))
            buf, tables = launch(max(need_k, hd64_staging_region(kth_k)), max(need_v, hd64_staging_region(kth_v)))
            if int(host[0]) & 0xffffffff:
                raise RuntimeError("compress_raw_pair_hd64: the repeat at the measured size overflowed: this is a bug")
        lens = host[1:].view(2, n, Bp).sum(1)   # [side][head] halfs
        out = []
        for side in range(2):
            offs = [0] + torch.cumsum(lens[side], 0).tolist()
            if offs[-1] // 8 > 0xffffffff:
                raise RuntimeError("compress_raw_pair_hd64: the packed stream exceeds what nz_offset (uint4 units, 32 bits) can address")
            bitmaps = torch.empty((Bp, tokens), dtype=torch.int64, device=dev)
            accum = torch.empty((Bp, tokens + 1), dtype=torch.int32, device=dev)
            packed = torch.empty((offs[-1],), dtype=torch.float16, device=dev)
            nz_offset = torch.tensor([o // 8 for o in offs[:-1]], dtype=torch.int32, device=dev)
            room = packed if offs[-1] else torch.empty((8,), dtype=torch.float16, device=dev)   # (no stream at all: nothing is written)
            dst = _lib.CacheView(bitmaps.data_ptr(), room.data_ptr(), accum.data_ptr(), nz_offset.data_ptr(), 0, 0, 0)
            err = Lb.mustafar_cache_gather_hd(st, dst, None, 0, tables + side * n * VIEW_BYTES, n, Bp, D)
            _lib.check(err, "mustafar_cache_gather_hd")
            out.append([bitmaps, accum, FlatStreams(pieces_of(packed, offs), flat=packed), nz_offset])
        del buf   # (stream-ordered: the gather launches are queued in front of any reuse)
    return out[0], out[1]
