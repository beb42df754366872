"""The reference layout `[bitmaps, idxs, nzs(list per kv-head), nz_offset]` (models/llama_mustafar_kernel.py:445) and what every cache
kind shares: the lowest layer above `_lib` (it imports `torch`, `ctypes` and `._lib` only; compression.py, cache.py / cache64.py, hook.py
and partial.py build on it, in that order).

A cache of ANY kind arrives at a call of the C ABI through one protocol.  `ListCache` wraps the list (or None: nothing compressed yet);
`CompressedArena` and `ExtentCache64` have the same surface (`heads`, `tokens`, `total_tokens`, `extents`, `view_ptr()`, `bytes_in_use()`)
and answer the same two questions, each with the objects to keep alive until the call is issued:
    decode_args(v, tables)   a fused decode call (hook._call_decode): the eight array addresses, or the form below
    view_args(v, tables)     `(k_view_ptr, v_view_ptr, T_base, k_table, v_table)`, tables null unless `tables`: what
                             mustafar_decode_multi_query takes, and with `tables=False` mustafar_decode_shared_segment
"""
from __future__ import annotations

import ctypes
from typing import List, Optional

import torch

from . import _lib


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


class FlatStreams(list):
    """The reference's per-head list of packed-nz tensors.  `streams.flat` is the packed stream of all heads as ONE tensor --
    `torch.cat(streams)`, what the model does on every decode step (:274/:314), which costs nothing when the elements are the
    `StreamPiece`s that `convert_*_batched` returns (compression.py: the pieces of one buffer, in order, ARE that buffer)."""

    def __init__(self, per_head: List[torch.Tensor], flat: Optional[torch.Tensor] = None):
        super().__init__(per_head)
        self._flat = flat

    @property
    def flat(self) -> Optional[torch.Tensor]:
        if self._flat is None and len(self):
            self._flat = torch.cat(self)
        return self._flat


def nz_offset_from_idxs(idxs: torch.Tensor, heads: int) -> torch.Tensor:
    """model :329-331 / :423-425 without the per-head Python loop: nz_offset[i] = sum_{j<i} idxs[j][-1] // 4."""
    last = idxs.view(heads, -1)[:, -1].to(torch.int64) // 4
    off = torch.zeros(heads, dtype=torch.int32, device=idxs.device)
    if heads > 1:
        off[1:] = torch.cumsum(last, 0)[:-1].to(torch.int32)
    return off


def append_compressed(old: list, new: list, heads: int, old_tokens: int, new_tokens: int, head_dim: int) -> list:
    """Cache append of model :339-368 (K) / :372-390 (V): shift the new offsets by each head's old total, splice
    bitmaps/offsets per head, concatenate the streams per head, advance nz_offset.  Tensor ops only (the
    reference builds `last_elements` through a Python list of device scalars, :341)."""
    o_bmp, o_idx, o_nz, o_off = old
    n_bmp, n_idx, n_nz, _ = new
    tiles_per_token = head_dim // 64
    n_last = n_idx.view(heads, -1)[:, -1].to(torch.int64) // 4                      # :341-342
    off = o_off.clone()
    if heads > 1:
        off[1:] += torch.cumsum(n_last, 0)[:-1].to(torch.int32)                      # :343-344
    base = o_idx.view(heads, -1)[:, -1:]                                             # :352-353
    idx = torch.cat([o_idx.view(heads, -1)[:, :-1], n_idx.view(heads, -1) + base], dim=1).flatten()   # :356-360
    bmp = torch.cat([o_bmp.view(heads, old_tokens * tiles_per_token),
                     n_bmp.view(heads, new_tokens * tiles_per_token)], dim=1).flatten()               # :364
    per_head = [torch.cat([o_nz[b], n_nz[b]], dim=0) for b in range(heads)]                           # :368
    return [bmp, idx, FlatStreams(per_head), off]


def _flat_stream(c):
    """The packed stream of all heads of a reference-layout cache as one tensor: a FlatStreams' `.flat`, a plain tensor, or a plain
    list of per-head tensors, concatenated here."""
    nz = c[2]
    return nz.flat if hasattr(nz, "flat") else (nz if isinstance(nz, torch.Tensor) else torch.cat(list(nz)))


def _addr(t):
    return t.data_ptr() if t is not None and t.numel() else None


class ListCache:
    """A reference-layout cache `[bitmaps, idxs, nzs, nz_offset]` of `tokens` tokens -- or None with `tokens == 0`: nothing compressed
    yet -- as it arrives at a call (module docstring).  Made where a call is issued: a `past` keeps holding the plain list.  The flat
    stream (a FlatStreams' `.flat` as it is; a plain Python list of per-head tensors concatenated ONCE, here) and the
    `mustafar_cache_view`, made on first use, are kept."""
    extents = ()              # a list never grows by extents
    lse_reads_tables = False

    def __init__(self, ref: Optional[list], tokens: int):
        self.ref, self.tokens, self.total_tokens = ref, int(tokens), int(tokens)
        self.heads = int(ref[3].numel()) if ref is not None else 0
        self.flat = _flat_stream(ref) if ref is not None else None
        self._view = None

    @property
    def view(self) -> "_lib.CacheView":
        if self._view is None:   # (holds the flat stream's address: made once, with it)
            bmp, idx, _, off = self.ref
            self._view = _lib.CacheView(_addr(bmp), _addr(self.flat), _addr(idx), _addr(off), 0, 0, 0)
        return self._view

    def view_ptr(self):
        return ctypes.byref(self.view)

    def bytes_in_use(self) -> int:
        """Bytes of the four arrays."""
        if self.ref is None:
            return 0
        bmp, idx, _, off = self.ref
        return bmp.numel() * 8 + idx.numel() * 4 + off.numel() * 4 + (self.flat.numel() * 2 if self.flat is not None else 0)

    def decode_args(self, v: "ListCache", tables: bool = False):
        """The eight array addresses (bitmaps, stream, idxs, nz_offset of K, then of V) and the tensors to keep until the call is
        issued.  None (nothing compressed yet) and empty tensors become null addresses."""
        if self.ref is None:
            return (None,) * 8, ()
        k_c, v_c, kz, vz = self.ref, v.ref, self.flat, v.flat
        return (_addr(k_c[0]), _addr(kz), _addr(k_c[1]), _addr(k_c[3]), _addr(v_c[0]), _addr(vz), _addr(v_c[1]), _addr(v_c[3])), (kz, vz)

    def view_args(self, v: "ListCache", tables: bool = False):
        """The two kept views with `T_base = tokens` and null tables (a list has no extents), or all null for the empty cache."""
        if self.ref is None:
            return (None, None, 0, None, None), ()
        return (self.view_ptr(), v.view_ptr(), self.tokens, None, None), (self, v)


def as_cache(c, tokens: int):
    """`c` as it answers `decode_args` / `view_args`: a reference-layout list (or None) of `tokens` tokens wrapped, a cache object as it is."""
    return ListCache(c, tokens) if c is None or isinstance(c, (list, tuple)) else c


class StatusPool:
    """What the pooled allocations of one trigger of `n_layers` layers share (cache.ExtentPool at D 128, cache64.ExtentPool64 at D 64):
    the layers' status words on the device, int64 [n_layers][1 + 2 heads] = [flag in the low 4 bytes | K lengths | V lengths], and the
    pinned landing area ONE copy brings them to.  The storage around them is the subclass's."""

    def __init__(self, n_layers: int, heads: int, device):
        self.n, self.heads, self.device = n_layers, heads, device
        self.status_words = 1 + 2 * heads

    def _adopt_status(self, raw: torch.Tensor) -> None:
        """raw: the `n x status_words x 8` bytes of the subclass's allocation that hold the status words; zeroed here."""
        self.status = raw.view(torch.int64).view(self.n, self.status_words)
        self.status.zero_()
        self._host = torch.empty((self.n, self.status_words), dtype=torch.int64).pin_memory()

    def totals_ptr(self, j: int) -> int:       # extent j = 2 * layer + side
        return self.status.data_ptr() + ((j // 2) * self.status_words + 1 + (j % 2) * self.heads) * 8

    def flag_ptr(self, layer: int) -> int:
        return self.status.data_ptr() + layer * self.status_words * 8

    def read_status(self) -> torch.Tensor:
        """ONE copy into pinned memory + ONE wait."""
        self._host.copy_(self.status, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return self._host
